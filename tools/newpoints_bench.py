"""(MI355X) cLocalMapping::CreateNewMapPoints on the device (mcs_create_new_map_points): the time of the whole neighbour chain for 5 and 20 neighbours at
3 x 1000 and 8 x 2000 features, next to
  (a) mcs_search_triangulation_sweep over the same pairs: what the searches cost when they may run as ONE batch (they may not: the loop is sequential);
  (b) the same neighbours as separate mcs_search_triangulation calls, each followed by a download of its matches (the host would triangulate there).
Device-resident inputs and outputs, medians over warm calls, each ending in a synchronisation.  The small size is checked against tests/newpoints_model.py
before it is timed.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/newpoints_bench.py`."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("multicol-slam_amd")
import gpu_common as G        # noqa: E402
import newpoints_model as M   # noqa: E402
import newpoints_pack as P    # noqa: E402


def median_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def run(ctx, nr_cams, per_cam, n_neigh, reps, check):
    cap, L = pkg._capi, pkg.lib()
    clutter = per_cam // 6
    kf1, nb = M.make_scene(100 + nr_cams + n_neigh, nr_cams=nr_cams, n_points=int(1.05 * nr_cams * (per_cam - clutter)), n_neigh=n_neigh, clutter=clutter)
    ns, n1, dim, nr = len(nb), kf1.n, kf1.desc.shape[1], kf1.nr
    mem = P.Mem(G, True)
    g1 = P.geom(pkg, mem, kf1, False)
    s1 = P.desc_set(pkg, mem, kf1, g1)
    g2, s2 = (cap.KfGeom * ns)(), (cap.DescSet * ns)()
    for s, kf in enumerate(nb):
        g2[s] = P.geom(pkg, mem, kf, True)
        s2[s] = P.desc_set(pkg, mem, kf, g2[s])
    outs = P.Outputs(pkg, mem, ns, n1)
    pm, rm = mem.out(np.full(ns * n1, -9, np.int32))
    pn, _ = mem.out(np.zeros(ns, np.int32))
    pf, _ = mem.out(np.zeros(ns, np.int32))
    pb, _ = mem.out(np.zeros(ns))
    pd, _ = mem.out(np.zeros(ns))
    ps, _ = mem.out(np.zeros(ns, np.uint8))
    pv, rv = mem.out(np.zeros(n1, np.uint8))

    def chain():
        pkg.check(L.mcs_create_new_map_points(ctx.h, ns, C.byref(g1), C.byref(s1), g2, s2, None, 0, dim, 16, 0, M.COS_THRESH, M.MAX_DIST, 1, pm, pn, pf, pb, pd, ps,
                                              pv, C.byref(outs.o)))
        ctx.synchronize()

    chain()
    got = outs.read()
    m12, v1 = rm(), rv().astype(bool)
    taken = np.zeros(n1, bool)
    for s, g in enumerate(got):   # self-consistency at every size
        m = m12[s * n1:(s + 1) * n1]
        assert not taken[m >= 0].any() and np.array_equal(g["idx1"], np.flatnonzero(g["verdict"] == 1))
        taken[g["idx1"]] = True
    assert np.array_equal(v1, ~kf1.has_mp & ~taken)
    if check:
        want, wv1 = M.create_new_map_points(kf1, nb)
        for s, (g, w) in enumerate(zip(got, want)):
            g.update(match12=m12[s * n1:(s + 1) * n1])
            P.compare(g, w, "neighbour %d" % s, with_search=False)
            assert np.array_equal(g["match12"], w["match12"])
        assert np.array_equal(v1, wv1)
    t_chain = median_ms(chain, reps)

    # (a) one batched sweep over the same pairs (sets padded to one size, E from the model's ComputeE)
    nmax = max(k.n for k in nb)
    d2, v2, c2, r2 = np.zeros((ns * nmax, dim), np.uint8), np.zeros(ns * nmax, np.uint8), np.zeros(ns * nmax, np.int32), np.zeros((ns * nmax, 3))
    for s, k in enumerate(nb):
        lo = s * nmax
        d2[lo:lo + k.n], v2[lo:lo + k.n], c2[lo:lo + k.n], r2[lo:lo + k.n] = k.desc, ~k.has_mp, k.cam, k.rays
    t = cap.DescSet(mem.p(d2), None, mem.p(v2), mem.p(c2), nmax, dim)
    pr2 = mem.p(r2)
    E = mem.p(np.ascontiguousarray(np.stack([M.essential_matrices(kf1, k) for k in nb])))

    def sweep():
        pkg.check(L.mcs_search_triangulation_sweep(ctx.h, ns, C.byref(s1), 0, C.byref(t), nmax, g1.rays, pr2, E, 9 * nr * nr, nr, dim, 16, 1, pm, pn, pf))
        ctx.synchronize()

    t_sweep = median_ms(sweep, reps)

    # (b) one search per neighbour, matches downloaded in between
    host = np.zeros(n1, np.int32)
    hip = G.hip()

    def separate():
        for s in range(ns):
            pkg.check(L.mcs_search_triangulation(ctx.h, 1, C.byref(s1), 0, C.byref(s2[s]), 0, g1.rays, g2[s].rays, E + 8 * 9 * nr * nr * s, nr, dim, 16, 1, pm, pn, pf))
            ctx.synchronize()
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), pm, n1 * 4, 2) == 0

    t_sep = median_ms(separate, reps)
    return dict(cams=nr_cams, features=n1, neighbours=ns, accepted=int(sum(len(g["idx1"]) for g in got)), chain_ms=round(t_chain, 3), sweep_ms=round(t_sweep, 3),
                separate_ms=round(t_sep, 3), checked=bool(check))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small-only", action="store_true")
    a = ap.parse_args()
    ctx = G.ctx()
    for nr_cams, per_cam in ((3, 1000),) if a.small_only else ((3, 1000), (8, 2000)):
        for nn in (5, 20):
            print(json.dumps(run(ctx, nr_cams, per_cam, nn, a.reps, check=nr_cams * per_cam <= 4000)), flush=True)
