#!/usr/bin/env python3
"""Per-call time of mcs_local_bundle_adjustment on an MI355X (not part of any test; nothing is asserted: there is no earlier implementation to compare with).

Shapes: 10 keyframes (8 free) x 2 000 points x about 20 000 edges, and 30 free + 30 fixed keyframes x 6 000 points x about 60 000 edges; 3 Lafida cameras,
0.5 px noise, 2 % gross outliers; device kind (arrays resident) and host kind (through the staging block); the median of --reps synchronised calls, every
repetition from the same start.  Printed with each: iterations and Levenberg trials of the run, the number of stream synchronisations the call makes (one per
trial, one per pass, one at the start), the time per trial, and — as the cost of one pass over as many edges — mcs_pose_optimization on one frame with that
many edges in the same kind.  One JSON line per shape.  The per-phase kernel times are not split out here: run the tool under a kernel trace for them."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lba_scenes as S        # noqa: E402
import poseopt_scenes as PS   # noqa: E402
from sim3opt_bench import pose_call, timed   # noqa: E402


def big_scene(seed, n_free, n_fixed, n_points, per_point):
    rng = np.random.default_rng(900 + seed)
    nk = n_free + n_fixed
    seen = [sorted(rng.choice(nk, per_point, replace=False).tolist()) for _ in range(n_points)]
    return S.make(seed, [0] * n_free + [1] * n_fixed, n_free, seen, nr=3, noise=0.5, n_outliers=n_points * per_point // 50)


def lba_call(pkg, FE, ctx, pr, device):
    cap, L = pkg._capi, pkg.lib()
    mem = FE._DEVICE if device else FE._HOST
    nr = len(pr.cams)
    ocs = np.frombuffer((cap.Ocam * nr)(*[cap.make_ocam(c) for c in pr.cams]), np.uint8).copy()
    g = dict(pose=pr.kf_pose.copy(), fixed=pr.kf_fixed, t=np.zeros((pr.n_local, 3)), pos=pr.pos.copy(), first=pr.pt_first, ekf=pr.edge_kf, ecam=pr.edge_cam,
             key=S.keys_of(pr, cap), Mc=np.ascontiguousarray(pr.Mc_min), ocs=ocs, sig=pr.inv_sigma2, es=np.zeros(pr.n_edges, np.uint8), ps=np.zeros(pr.n_points, np.uint8))
    g = {k: mem.put(v) for k, v in g.items()}
    fresh = (mem.put(pr.kf_pose.copy()), mem.put(pr.pos.copy()))
    dg = cap.LbaDiag()

    def reset():
        if device:
            FE._hip().hipMemcpy(g["pose"].ptr, fresh[0].ptr, pr.kf_pose.nbytes, 3)
            FE._hip().hipMemcpy(g["pos"].ptr, fresh[1].ptr, pr.pos.nbytes, 3)
        else:
            g["pose"][:] = pr.kf_pose
            g["pos"][:] = pr.pos

    def call():
        pkg.check(L.mcs_local_bundle_adjustment(ctx.h, pr.n_kfs, pr.n_local, mem.ptr(g["pose"]), mem.ptr(g["fixed"]), mem.ptr(g["t"]), pr.n_points, mem.ptr(g["pos"]),
                                                mem.ptr(g["first"]), pr.n_edges, mem.ptr(g["ekf"]), mem.ptr(g["ecam"]), mem.ptr(g["key"]), None, None, mem.ptr(g["Mc"]),
                                                mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(pr.inv_sigma2), pr.std_recon, None, mem.kind, mem.ptr(g["es"]),
                                                mem.ptr(g["ps"]), C.byref(dg)))
    return call, reset, dg, (g, fresh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    pkg = importlib.import_module("multicol-slam_amd")
    FE = importlib.import_module("multicol-slam_amd.frontend")
    ctx = pkg.Context(0)
    for n_free, n_fixed, n_points, per_point in ((8, 2, 2000, 10), (30, 30, 6000, 10)):
        pr = big_scene(0, n_free, n_fixed, n_points, per_point)
        row = dict(keyframes=pr.n_kfs, free=n_free, points=pr.n_points, edges=pr.n_edges)
        for device in (True, False):
            kind = "device" if device else "host"
            call, reset, dg, keep = lba_call(pkg, FE, ctx, pr, device)
            ms = timed(ctx, call, reset, a.reps)
            trials = int(sum(sum(r) for r in dg.trials))
            row["lba_%s_ms" % kind] = ms
            if device:
                row.update(status=dg.status, iters=list(dg.iters), trials=trials, erased=list(dg.n_erased), waits=trials + 3, ms_per_trial=round(ms / max(trials, 1), 4))
            pp = PS.scene(0, min(pr.n_edges, 65000), 3, n_outliers=pr.n_edges // 50)
            pcall, preset, pkeep = pose_call(pkg, FE, ctx, [pp], device)
            row["pose_optimization_%s_ms" % kind] = timed(ctx, pcall, preset, a.reps)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
