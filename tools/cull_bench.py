"""(MI355X) mcs_covis_cull_keyframes for 20 and 80 listed keyframes and mcs_covis_cull_points for 2 000 recent points on stores of 100 / 1 000 / 4 000
keyframes x 3 000 features, device-kind (outputs resident; the timed window ends in a synchronisation).  Next to each: mcs_covis_update_connections for one
keyframe on the same store, which walks the same rows (k_covis_count) and is the yardstick for the wide pass.  From a run of its own with event timing on
the context: the wide pass k_cull_observe, its row bytes (16 bytes of ids + 4 bytes of octaves per four entries) / time next to the 8 TB/s HBM peak, and the
serial chain k_cull_chain.  The timed calls list every keyframe with not_erase set, so that the store stays as it is and every repetition does the same work
(the chain then puts the keyframe's observations back where a culled one would flag its points: the same walk over the distinct row); one call without
not_erase at the end reports what the culling does on this store.  NO time here is a pass criterion.  Prints one JSON line per shape."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
pkg = importlib.import_module("multicol-slam_amd")
import gpu_common as G                       # noqa: E402
from covis_bench import PEAK_TBS, median_ms  # noqa: E402
from cull_pack import CullDev                # noqa: E402


def build(nkf, nfeat, npoints, seed=1):
    """rows as in covis_bench.build (sliding windows over the points, 30 % NULL, 10 % repeats, 5 % of the points bad) but denser — windows of 2 * nfeat points,
    about eleven observers per point — so that KeyFrameCulling has something to cull; octaves: a base level per keyframe in 2 .. 4 and a spread of one level
    either way"""
    rng = np.random.default_rng(seed)
    d = CullDev(pkg, G, nkf, nfeat, npoints, False)
    win = min(npoints, 2 * nfeat)
    rows = []
    for k in range(nkf):
        lo = int((npoints - win) * k / max(nkf - 1, 1))
        row = rng.integers(lo, lo + win, nfeat).astype(np.int32)
        row[rng.random(nfeat) < 0.3] = -1
        rep = np.flatnonzero(rng.random(nfeat) < 0.1)
        row[rep] = row[rng.integers(0, nfeat, len(rep))]
        assert d.set_keyframe(k + 1, row) == 0
        assert d.set_octaves(k + 1, np.clip(rng.integers(2, 5) + rng.integers(-1, 2, nfeat), 0, 7)) == 0
        rows.append(row)
    assert d.set_points_bad(np.flatnonzero(rng.random(npoints) < 0.05).astype(np.int32)) == 0
    return d, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--listed", type=int, nargs="*", default=[20, 80])
    ap.add_argument("--recent", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    ctx, L = G.ctx(), pkg.lib()
    for nkf in a.keyframes:
        npoints = max(2 * a.features, nkf * a.features // 16)
        d, rows = build(nkf, a.features, npoints)
        S = d.slots()
        mid = nkf // 2 + 1
        q = np.array([mid], np.int64)
        oc = [G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32)), G.DevBuf(np.zeros(S, np.int64)), G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32))]

        def con():
            assert L.mcs_covis_update_connections(d.h, 1, q.ctypes.data, 1, *[x.ptr for x in oc]) == 0
            assert L.mcs_ctx_synchronize(ctx.h) == 0
        res = dict(keyframes=nkf, features=a.features, points=npoints, update_connections_ms=median_ms(con, a.reps))
        row_bytes = sum((len(r) + 3) // 4 * 20 for r in rows)
        cap = npoints
        for nl in a.listed:
            nl = min(nl, nkf)
            ids = np.arange(mid - nl // 2, mid - nl // 2 + nl, dtype=np.int64).clip(1, nkf)      # the listed keyframes: the neighbours of the middle one
            ids = np.unique(ids)
            keep = np.ones(len(ids), np.uint8)
            o = [G.DevBuf(np.zeros(len(ids), np.int32)) for _ in range(3)] + [G.DevBuf(np.zeros(cap, np.int32)), G.DevBuf(np.zeros(1, np.int32))]

            def cull(ne=keep):
                assert L.mcs_covis_cull_keyframes(d.h, len(ids), ids.ctypes.data, None if ne is None else ne.ctypes.data, cap, 1, *[x.ptr for x in o]) == 0
                assert L.mcs_ctx_synchronize(ctx.h) == 0
            res["cull_keyframes_%d_ms" % nl] = median_ms(cull, a.reps)
            ctx.enable_timing(True)
            wide, chain = [], []
            for _ in range(5):
                cull()
                wide.append(ctx.kernel_ms("cull_observe")); chain.append(ctx.kernel_ms("cull_chain"))
            ctx.enable_timing(False)
            res.update({"cull_observe_%d_ms" % nl: float(np.median(wide)), "cull_chain_%d_ms" % nl: float(np.median(chain)),
                        "cull_observe_%d_TBs" % nl: row_bytes / (np.median(wide) * 1e-3) / 1e12,
                        "would_cull_%d" % nl: int((o[0].read() == 2).sum())})
        # MapPointCulling: recent points that stay (found == visible, first keyframe == current), so that every repetition sees the same store
        rng = np.random.default_rng(2)
        n = min(a.recent, npoints)
        pid = G.DevBuf(rng.permutation(npoints)[:n].astype(np.int32))
        one, first, ov = G.DevBuf(np.ones(n, np.int32)), G.DevBuf(np.full(n, nkf, np.int64)), G.DevBuf(np.zeros(n, np.int32))

        def points():
            assert L.mcs_covis_cull_points(d.h, nkf, n, pid.ptr, one.ptr, one.ptr, first.ptr, 1, ov.ptr) == 0
            assert L.mcs_ctx_synchronize(ctx.h) == 0
        res["cull_points_%d_ms" % n] = median_ms(points, a.reps)
        res.update(row_bytes=row_bytes, peak_TBs=PEAK_TBS)
        cull(None)                                                                                    # the real thing, once
        res.update(culled=int((o[0].read() == 1).sum()), bad_points=int(o[4].read()[0]))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
