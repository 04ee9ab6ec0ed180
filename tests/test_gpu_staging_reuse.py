"""-m gpu: host-kind calls of DIFFERENT entry points share one staging block per context (csrc/mcs_host.h, struct Staging).  Back to back on one
context, in an order and with sizes that make the block regrow between them and again in a second round with larger inputs, every call must return what
the same call returns on a fresh context: nothing of an earlier call's layout, mirror contents or capacity may leak into a later one.

round 1: mcs_search_kf_kf (small) -> mcs_create_new_map_points (host kind, 3 cameras x 5 neighbours) -> mcs_window_match -> mcs_distinctive_descriptors
         -> the first search again
round 2: a larger search -> mcs_create_new_map_points (8 cameras x 20 neighbours: the largest block) -> a larger window match -> the searches again
Equality only; nothing here is meant to fail."""
import ctypes as C
import importlib

import numpy as np
import pytest

import newpoints_model as M
import newpoints_pack as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


def descriptors(rng, n, dim=32):
    """n rows and n noisy copies of them (so the searches accept something), with learned-mask stand-ins"""
    a = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    b = a.copy()
    flip = rng.random((n, dim)) < 0.04
    b[flip] ^= rng.integers(1, 256, int(flip.sum()), dtype=np.uint8)
    b = b[rng.permutation(n)]
    ma = rng.integers(0, 256, (n, dim), dtype=np.uint8) | 0x0F
    mb = rng.integers(0, 256, (n, dim), dtype=np.uint8) | 0x0F
    return a, ma, b, mb


def search_job(seed, n):
    rng = np.random.default_rng(seed)
    a, ma, b, mb = descriptors(rng, n)

    def run(mcs, ctx):
        cap = mcs._capi
        q = cap.DescSet(cap.np_ptr(a), cap.np_ptr(ma), None, None, n, 32)
        t = cap.DescSet(cap.np_ptr(b), cap.np_ptr(mb), None, None, n, 32)
        m12, nm, fb = np.full(n, -9, np.int32), np.full(1, -9, np.int32), np.full(1, -9, np.int32)
        mcs.check(mcs.lib().mcs_search_kf_kf(ctx.h, 1, C.byref(q), 0, C.byref(t), 0, 32, 0.8, 16, cap.MEM_HOST, cap.np_ptr(m12), cap.np_ptr(nm), cap.np_ptr(fb)))
        assert int(nm[0]) > n // 4, int(nm[0])
        return [m12, nm, fb]
    return run


def window_job(seed, n):
    """n probes around the features of a synthetic one-camera frame, descriptors as in search_job"""
    rng = np.random.default_rng(seed)
    cap = importlib.import_module("multicol-slam_amd._capi")
    pd, pm, fd, fm = descriptors(rng, n)
    keys = np.zeros(n, cap.KP_DTYPE)
    keys["x"], keys["y"] = rng.uniform(20, 620, n), rng.uniform(20, 460, n)
    keys["octave"] = rng.integers(0, 8, n)
    keys["angle"] = rng.uniform(0, 360, n)
    x = keys["x"].astype(np.float64) + rng.normal(0, 2.0, n)
    y = keys["y"].astype(np.float64) + rng.normal(0, 2.0, n)
    r = np.full(n, 40.0)
    lo, hi = np.zeros(n, np.int32), np.full(n, 7, np.int32)
    cam = np.zeros(n, np.int32)
    w, h = np.array([640], np.int32), np.array([480], np.int32)
    sc = 1.2 ** np.arange(8)

    def run(mcs, ctx):
        p = cap.np_ptr
        asg = np.zeros(n, np.uint8)
        match, nm = np.full(n, -9, np.int32), np.full(1, -9, np.int32)
        pr = cap.WindowProbes(p(x), p(y), p(r), p(lo), p(hi), p(cam), p(pd), p(pm), n, 32, None)
        fv = cap.FrameView(p(keys), p(fd), p(fm), p(cam), p(asg), n, 32, 1, p(w), p(h), p(sc), 8)
        mcs.check(mcs.lib().mcs_window_match(ctx.h, C.byref(pr), C.byref(fv), cap.WINDOW_RATIO, 0.8, 32, cap.MEM_HOST, p(match), p(nm)))
        assert int(nm[0]) > 0
        return [match, nm, asg]
    return run


def distinct_job(seed, npoints):
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 9, npoints)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    rows = int(off[-1])
    dd = rng.integers(0, 256, (rows, 32), dtype=np.uint8)
    mm = rng.integers(0, 256, (rows, 32), dtype=np.uint8)

    def run(mcs, ctx):
        cap = mcs._capi
        best = np.full(npoints, -9, np.int32)
        mcs.check(mcs.lib().mcs_distinctive_descriptors(ctx.h, cap.np_ptr(dd), cap.np_ptr(mm), 32, 32, cap.np_ptr(off), npoints, cap.MEM_HOST, cap.np_ptr(best)))
        return [best]
    return run


def chain_job(G, **scene):
    kf1, nb = M.make_scene(**scene)

    def run(mcs, ctx):
        res, v1 = P.chain(mcs, ctx, G, kf1, nb, device=False)
        out = [v1]
        for r in res:
            out += [np.asarray(r[k]) for k in sorted(r)]
        return out
    return run


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and P.same_bits(a, b)
    return a.shape == b.shape and np.array_equal(a, b)


def test_different_host_kind_calls_share_one_block(G):
    mcs = G.mcs
    # approximate block per job (staged inputs + outputs), which is what makes it regrow (a grown block holds 1.5 x the need that grew it):
    # search 600: 0.08 MB -> chain 3 x 5 (6 keyframes, 6 600 features in all): 1.2 MB, regrows -> window 1500, distinct 700, search 600: well below, fit;
    # search 6000: 0.8 MB, fits -> chain 8 x 20 (21 keyframes, 61 000 features): 11 MB, regrows -> window 9000 (a few MB) and the searches fit.
    # When changing sizes keep the first search the smallest and each chain several times larger than everything before it.
    s_small, s_large = search_job(1, 600), search_job(2, 6000)
    jobs = [("search small", s_small), ("chain 3 x 5", chain_job(G, seed=11, nr_cams=3, n_points=900, n_neigh=5)), ("window", window_job(3, 1500)),
            ("distinct", distinct_job(4, 700)), ("search small again", s_small),
            ("search large", s_large), ("chain 8 x 20", chain_job(G, seed=12, nr_cams=8, n_points=2400, n_neigh=20)), ("window large", window_job(5, 9000)),
            ("search small, third time", s_small), ("search large again", s_large)]
    shared = mcs.Context(0)
    got = [run(mcs, shared) for _, run in jobs]
    shared.close()
    for (name, run), g in zip(jobs, got):
        fresh = mcs.Context(0)
        want = run(mcs, fresh)
        fresh.close()
        assert len(g) == len(want), name
        for k, (a, b) in enumerate(zip(g, want)):
            assert same(a, b), (name, k)
