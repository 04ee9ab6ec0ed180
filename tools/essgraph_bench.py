#!/usr/bin/env python3
"""Per-call time of mcs_optimize_essential_graph on an MI355X (not part of any test; nothing is asserted: there is no earlier implementation to compare with).

Shapes: 100, 300 and 512 free keyframes (one more, fixed) on a circle, a spanning-tree edge and covisibility edges to the three keyframes before the parent per keyframe (covis=4 counts the parent), a loop with a rotation drift
of 0.03 rad, a translation drift of 0.4 and a scale drift of 4 % corrected on the last six keyframes; device kind (arrays resident) and host kind (through the
staging block), both through frontend.OptimizeEssentialGraphArrays, which in device kind places the arrays first; the median of --reps synchronised calls.  Printed with each: iterations and Levenberg trials of the run, the time per trial, and — from a
further run under mcs_ctx_enable_timing, which times the LAST trial of the call — that trial's time and the share of the solve (zeroing, assembly,
factorisation, substitutions) in it.  Next to them, as the known point, mcs_local_bundle_adjustment at 64 free keyframes (tests/lba_scenes.chain).  One JSON
line per shape."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import essgraph_scenes as S   # noqa: E402
import lba_scenes as LS       # noqa: E402
from lba_bench import lba_call   # noqa: E402
from sim3opt_bench import timed  # noqa: E402


def scene(n_free):
    K = n_free + 1
    return S.make(1, K, S._tail(K, 6, 0.03, 0.4, 1.04), [(K - 1, 0), (K - 2, 0)], [0], covis=4, n_points=20 * K, drift=0.002)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--free", type=int, nargs="*", default=[100, 300, 512])
    a = ap.parse_args()
    pkg = importlib.import_module("multicol-slam_amd")
    FE = importlib.import_module("multicol-slam_amd.frontend")
    ctx = pkg.Context(0)
    for n_free in a.free:
        pr = scene(n_free)
        row = dict(free=n_free, unknowns=7 * n_free, edges=len(pr.edge_i), points=len(pr.pos))
        for device in (True, False):
            kind = "device" if device else "host"
            out = {}

            def call():
                out["r"] = FE.OptimizeEssentialGraphArrays(*pr.arrays(), device=device, ctx=ctx)
            ms = timed(ctx, call, lambda: None, a.reps)
            d = out["r"]["diag"]
            trials = int(d["trials"].sum())
            row["essgraph_%s_ms" % kind] = ms
            if device:
                row.update(status=int(d["status"]), iters=int(d["iters"]), stop=int(d["stop"]), trials=trials, ms_per_trial=round(ms / max(trials, 1), 4))
                ctx.enable_timing(True)
                call()
                ctx.synchronize()
                trial, solve = ctx.kernel_ms("eg_trial"), ctx.kernel_ms("eg_solve")
                ctx.enable_timing(False)
                row.update(last_trial_ms=round(trial, 4), solve_ms=round(solve, 4), solve_share=round(solve / trial, 3))
        print(json.dumps(row), flush=True)
    pr = LS.chain(64)
    row = dict(lba_free=64, edges=pr.n_edges, points=pr.n_points)
    for device in (True, False):
        call, reset, dg, keep = lba_call(pkg, FE, ctx, pr, device)
        ms = timed(ctx, call, reset, a.reps)
        trials = int(sum(sum(r) for r in dg.trials))
        row["lba_%s_ms" % ("device" if device else "host")] = ms
        if device:
            row.update(iters=list(dg.iters), trials=trials, ms_per_trial=round(ms / max(trials, 1), 4))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
