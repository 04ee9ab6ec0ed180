"""(MI355X) mcs_covis_update_reference and mcs_covis_update_connections at 100 / 1 000 / 4 000 keyframes x 3 000 features, device-kind (inputs and outputs
resident; the timed window ends in a synchronisation).  Reports the median wall time per call and, from a run of its own with event timing on the context,
the time of k_covis_count and its row bytes / time next to the 8 TB/s HBM peak (the kernel reads every live distinct row once; the gathers of mult[] hit
a table of max_points ints and are not counted).  NO time here is a pass criterion.  --compare adds the route the library had before: the local list built
on the host (tests/covis_model.py's order, with numpy), the per-point arrays gathered on the host and everything staged through a host-kind
mcs_search_local_points — only the list building and the gathers are timed, the search is the same on both routes.
Prints one JSON line per shape."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("multicol-slam_amd")
import gpu_common as G      # noqa: E402
from covis_pack import Dev  # noqa: E402

PEAK_TBS = 8.0


def build(nkf, nfeat, npoints, seed=1):
    """keyframes over sliding windows of 4 * nfeat points, 30 % NULL, 10 % repeats, 5 % of the points bad"""
    rng = np.random.default_rng(seed)
    d = Dev(pkg, G, nkf, nfeat, npoints, False)
    win = min(npoints, 4 * nfeat)
    rows = []
    for k in range(nkf):
        lo = int((npoints - win) * k / max(nkf - 1, 1))
        row = rng.integers(lo, lo + win, nfeat).astype(np.int32)
        row[rng.random(nfeat) < 0.3] = -1
        rep = np.flatnonzero(rng.random(nfeat) < 0.1)
        row[rep] = row[rng.integers(0, nfeat, len(rep))]
        assert d.set_keyframe(k + 1, row) == 0
        rows.append(row)
    bad = np.flatnonzero(rng.random(npoints) < 0.05).astype(np.int32)
    assert d.set_points_bad(bad) == 0
    lo = (npoints - win) // 2
    frame = rng.integers(lo, lo + win, nfeat).astype(np.int32)
    frame[rng.random(nfeat) < 0.3] = -1
    return d, rows, frame, bad


def median_ms(fn, reps, warm=3):
    t = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def host_list(rows, frame, bad_mask):
    """the local list as a host would build it with numpy: votes, local keyframes, first occurrences in visiting order"""
    npoints = len(bad_mask)
    f = frame[frame >= 0]
    mult = np.bincount(f[~bad_mask[f]], minlength=npoints)
    local = []
    for r in rows:
        u = np.unique(r[r >= 0])
        if mult[u].sum() > 4:
            local.append(r)
    if not local:
        return np.zeros(0, np.int64)
    cat = np.concatenate(local)
    cat = cat[cat >= 0]
    cat = cat[~bad_mask[cat]]
    _, first = np.unique(cat, return_index=True)
    return cat[np.sort(first)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--compare", action="store_true")
    a = ap.parse_args()
    ctx, L = G.ctx(), pkg.lib()
    for nkf in a.keyframes:
        npoints = max(4 * a.features, nkf * a.features // 8)
        d, rows, frame, bad = build(nkf, a.features, npoints)
        S, cap = d.slots(), npoints
        fp, t = G.DevBuf(frame), G.DevBuf(np.zeros(3))
        o = [G.DevBuf(np.zeros(S, np.int64)), G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(S)), G.DevBuf(np.zeros(1, np.int32)), G.DevBuf(np.zeros(1, np.int64)),
             G.DevBuf(np.zeros(cap, np.int32)), G.DevBuf(np.zeros(1, np.int32))]

        def ref():
            assert L.mcs_covis_update_reference(d.h, fp.ptr, len(frame), t.ptr, cap, 1, *[x.ptr for x in o]) == 0
            assert L.mcs_ctx_synchronize(ctx.h) == 0
        q = np.array([nkf // 2 + 1], np.int64)
        oc = [G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32)), G.DevBuf(np.zeros(S, np.int64)), G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32))]

        def con():
            assert L.mcs_covis_update_connections(d.h, 1, q.ctypes.data, 1, *[x.ptr for x in oc]) == 0
            assert L.mcs_ctx_synchronize(ctx.h) == 0
        res = dict(keyframes=nkf, features=a.features, points=npoints, update_reference_ms=median_ms(ref, a.reps), update_connections_ms=median_ms(con, a.reps))
        res.update(n_local=int(o[3].read()[0]), n_points=int(o[6].read()[0]), n_ordered=int(oc[4].read()[0]))
        ctx.enable_timing(True)
        ks = []
        for _ in range(5):
            ref()
            ks.append(ctx.kernel_ms("covis_count"))
        ctx.enable_timing(False)
        row_bytes = sum((len(r) + 3) // 4 * 16 for r in rows)
        res.update(covis_count_ms=float(np.median(ks)), row_bytes=row_bytes, covis_count_TBs=row_bytes / (np.median(ks) * 1e-3) / 1e12, peak_TBs=PEAK_TBS)
        if a.compare:
            bad_mask = np.zeros(npoints, bool)
            bad_mask[bad] = True
            tables = [np.zeros((npoints, 3)), np.zeros((npoints, 3)), np.zeros(npoints), np.zeros(npoints), np.zeros((npoints, 32), np.uint8), np.zeros((npoints, 32), np.uint8)]

            def host():
                lst = host_list(rows, frame, bad_mask)
                return [tb[lst] for tb in tables]
            res["host_list_and_gathers_ms"] = median_ms(host, max(3, a.reps // 4), warm=1)
            assert len(host_list(rows, frame, bad_mask)) == res["n_points"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
