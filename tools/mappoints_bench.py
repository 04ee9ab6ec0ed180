"""(MI355X) mcs_covis_update_points on stores of 100 / 1 000 / 4 000 keyframes x 3 000 features with 32-byte descriptors: 2 000 and
20 000 listed points, once with the store's typical segments (about eight entries per point) and once with a tail of 16 hub points of 129 .. 2 000 entries
among them.  Device-kind, outputs resident; the timed window ends in a synchronisation.  Per case:
  the whole call (median and the 10 % / 90 % quantiles of the repetitions);
  from runs of their own with event timing on the context: every kernel of the call (mp_count, mp_fill: the two passes over the rows; mp_sort; mp_normal;
  mp_collect: both phases and the scan between them; mp_distinct: k_distinct) and the row bytes / time of the two streaming passes next to the 8 TB/s HBM peak;
  k_covis_count on the SAME store (mcs_covis_update_connections for the middle keyframe, tools/covis_bench.py's figure): it streams the distinct rows of the
  same layout, without the per-entry lookup hit rate and the atomics of the new passes;
  the route a caller has without the call, on the same store: the rows brought to the host, the segments and the normals in numpy, the descriptor choice
  through a host-kind mcs_distinctive_descriptors;
  the share of k_distinct's time that belongs to segments beyond its LDS limit of 128 rows: the call with and without the hub tail.
NO time here is a pass criterion.  Prints one JSON line per case."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
pkg = importlib.import_module("multicol-slam_amd")
FE = importlib.import_module("multicol-slam_amd.frontend")
import gpu_common as G                       # noqa: E402
from covis_bench import PEAK_TBS             # noqa: E402

DIM, NLEVELS, HUBS = 32, 8, 16
SCALES = np.cumprod([1.0] + [float(np.float32(1.2))] * (NLEVELS - 1))
KERNELS = ("mp_count", "mp_fill", "mp_sort", "mp_normal", "mp_collect", "mp_distinct")


def build(nkf, nfeat, npoints, seed=1):
    """rows as in covis_bench.build (sliding windows of 4 * nfeat points, 30 % NULL, 10 % repeats, 5 % of the points bad); hub point j (ids npoints - HUBS ..)
    overwrites one feature of L_j random keyframes, L_j from 129 to min(2 000, nkf) in equal ratios.  Descriptors: one random block, XORed with the slot."""
    rng = np.random.default_rng(seed)
    st = FE.cCovisibility(nkf, nfeat, npoints, ctx=G.ctx())
    win = min(npoints - HUBS, 4 * nfeat)
    rows = np.zeros((nkf, nfeat), np.int32)
    for k in range(nkf):
        lo = int((npoints - HUBS - win) * k / max(nkf - 1, 1))
        row = rng.integers(lo, lo + win, nfeat).astype(np.int32)
        row[rng.random(nfeat) < 0.3] = -1
        rep = np.flatnonzero(rng.random(nfeat) < 0.1)
        row[rep] = row[rng.integers(0, nfeat, len(rep))]
        rows[k] = row
    top = min(2000, nkf)
    hub_len = np.unique(np.round(np.exp(np.linspace(np.log(min(129, top)), np.log(top), HUBS))).astype(int))
    hubs = []
    for j, L in enumerate(hub_len):
        p = npoints - HUBS + j
        rows[rng.permutation(nkf)[:L], j] = p                    # feature j of L keyframes
        hubs.append(p)
    base = rng.integers(0, 256, (nfeat, DIM), dtype=np.uint8)
    t = rng.normal(0, 2, (nkf, 3))
    for k in range(nkf):
        st.SetKeyFrame(k + 1, rows[k])
        st.SetOctaves(k + 1, np.clip(rng.integers(2, 5) + rng.integers(-1, 2, nfeat), 0, NLEVELS - 1))
        st.SetDescriptors(k + 1, base ^ np.uint8(k & 255))
    st.SetPose(range(1, nkf + 1), t)
    st.SetPointsBad(np.flatnonzero(rng.random(npoints - HUBS) < 0.05))
    return st, rows, base, t, hubs, hub_len.tolist()


def quantiles_ms(fn, reps, warm=3):
    ts = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            ts.append(1e3 * (time.perf_counter() - t0))
    return [float(np.quantile(ts, q)) for q in (0.5, 0.1, 0.9)]


def host_route(ctx, rows_dev, base, t, ids, pos, nfeat):
    """today's route for the same list: rows to the host, segments and normals in numpy (vectorised: not the ordered chain), the choice on the device"""
    L = pkg.lib()
    rows = rows_dev.read()
    flat = rows.ravel()
    sel = np.flatnonzero(np.isin(flat, ids))
    pts = flat[sel]
    order = np.lexsort((sel, pts))                               # by point, then slot and feature
    sel, pts = sel[order], pts[order]
    uniq, counts = np.unique(pts, return_counts=True)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    slot = sel // nfeat
    where = np.searchsorted(np.sort(ids), pts)
    d = pos[np.argsort(ids, kind="stable")][where] - t[slot]
    unit = d / np.sqrt((d * d).sum(axis=1))[:, None]
    head = np.ones(len(sel), bool)
    head[1:] = (pts[1:] != pts[:-1]) | (slot[1:] != slot[:-1])
    seg = np.repeat(np.arange(len(uniq)), counts)
    normal = np.zeros((len(uniq), 3))
    np.add.at(normal, seg[head], unit[head])
    normal /= np.bincount(seg[head], minlength=len(uniq))[:, None]
    D = np.ascontiguousarray(base[sel % nfeat] ^ (slot & 255).astype(np.uint8)[:, None])
    best = np.zeros(len(uniq), np.int32)
    pkg._capi.check(L.mcs_distinctive_descriptors(ctx.h, D.ctypes.data, None, DIM, DIM, offsets.ctypes.data, len(uniq), 0, best.ctypes.data))
    return normal, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, nargs="*", default=[100, 1000, 4000])
    ap.add_argument("--features", type=int, default=3000)
    ap.add_argument("--listed", type=int, nargs="*", default=[2000, 20000])
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    ctx, L = G.ctx(), pkg.lib()
    for nkf in a.keyframes:
        npoints = max(2 * a.features, nkf * a.features // 16) + HUBS
        st, rows, base, t, hubs, hub_len = build(nkf, a.features, npoints)
        row_bytes = nkf * ((a.features + 3) // 4) * 16               # every live row once, 16 bytes per four entries
        rows_dev = G.DevBuf(rows)
        q = np.array([nkf // 2 + 1], np.int64)
        S = st.slots()
        oc = [G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32)), G.DevBuf(np.zeros(S, np.int64)), G.DevBuf(np.zeros(S, np.int32)), G.DevBuf(np.zeros(1, np.int32))]
        ctx.enable_timing(True)
        ks = []
        for _ in range(5):
            assert L.mcs_covis_update_connections(st.h, 1, q.ctypes.data, 1, *[x.ptr for x in oc]) == 0
            ks.append(ctx.kernel_ms("covis_count"))
        ctx.enable_timing(False)
        count_ms = float(np.median(ks))
        rng = np.random.default_rng(3)
        observed = np.unique(rows[rows >= 0])
        observed = observed[observed < npoints - HUBS]
        for n in a.listed:
            n = min(n, len(observed))
            plain = rng.permutation(observed)[:n].astype(np.int32)
            res = dict(keyframes=nkf, features=a.features, points=npoints, listed=n, row_bytes=row_bytes, covis_count_ms=count_ms,
                       covis_count_TBs=row_bytes / (count_ms * 1e-3) / 1e12, peak_TBs=PEAK_TBS, hub_rows=hub_len)
            for tail in (False, True):
                ids = plain.copy()
                if tail:
                    ids[:len(hubs)] = hubs
                pos = rng.normal(0, 3, (n, 3))
                ref = rng.integers(1, nkf + 1, n).astype(np.int64)
                d = [G.DevBuf(x) for x in (ids, pos, ref, SCALES)]
                o = [G.DevBuf(np.zeros((n, 3))), None, None, G.DevBuf(np.zeros(n)), G.DevBuf(np.zeros(n)), G.DevBuf(np.zeros((n, DIM), np.uint8)), None,
                     G.DevBuf(np.zeros(n, np.int32)), G.DevBuf(np.zeros(n, np.int64)), G.DevBuf(np.zeros(n, np.int32)), G.DevBuf(np.zeros(n, np.int32))]

                def call():
                    assert L.mcs_covis_update_points(st.h, n, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, NLEVELS, 1, *[None if x is None else x.ptr for x in o]) == 0
                    assert L.mcs_ctx_synchronize(ctx.h) == 0
                tag = "hubs" if tail else "plain"
                res["call_%s_ms" % tag] = quantiles_ms(call, a.reps)
                ctx.enable_timing(True)
                ker = {k: [] for k in KERNELS}
                for _ in range(5):
                    call()
                    for k in KERNELS:
                        ker[k].append(ctx.kernel_ms(k))
                ctx.enable_timing(False)
                for k in KERNELS:
                    res["%s_%s_ms" % (k, tag)] = float(np.median(ker[k]))
                for k in ("mp_count", "mp_fill"):
                    res["%s_%s_TBs" % (k, tag)] = row_bytes / (res["%s_%s_ms" % (k, tag)] * 1e-3) / 1e12
                nd = o[7].read()
                res["rows_%s" % tag] = int(nd.sum())
                res["longest_%s" % tag] = int(nd.max())
                res["host_route_%s_ms" % tag] = quantiles_ms(lambda: host_route(ctx, rows_dev, base, t, ids, pos, a.features), 3, warm=1)
            res["distinct_beyond_lds_share"] = max(0.0, 1.0 - res["mp_distinct_plain_ms"] / max(res["mp_distinct_hubs_ms"], 1e-9))
            print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
