"""-m gpu: the device Sim3 RANSAC (mcs_sim3_*, src/cSim3Solver.cpp) against the line-by-line model of tests/sim3_model.py: draws, picks, per-hypothesis
inlier counts and masks bit for bit (outside the pairs the model flags as within 1e-9 of their threshold), the hypothesis doubles to 1e-9, and every
output of every iterate() call."""
import ctypes as C
import importlib

import numpy as np
import pytest

import sim3_model as M
from hostile_sim3 import compare_hypotheses, run_rounds   # the comparisons shared with the hostile suite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    FE = importlib.import_module("multicol-slam_amd.frontend")
    return dict(G=G, FE=FE, pkg=G.mcs, cams=G.cams3())


class Batch:
    """mcs_sim3_create over the pairs of sim3_model.make_pair (raw ABI: the parity tests drive the library without keyframe objects)"""

    def __init__(self, pkg, ctx, cams, M_c, pairs, params, seed, draws=None):
        L = pkg.lib()
        nr, ns = len(cams), len(pairs)
        self.L, self.pairs = L, pairs
        Mc = np.ascontiguousarray(np.stack(M_c).reshape(nr, 16))
        ocs = (pkg._capi.Ocam * nr)(*[pkg.make_ocam(c) for c in cams])
        off = np.zeros(ns + 1, np.int32)
        off[1:] = np.cumsum([len(p["index1"]) for p in pairs])
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in pairs]), dt)
        self.n1 = np.array([p["mN1"] for p in pairs], np.int32)
        arrs = dict(Mt=np.ascontiguousarray(np.stack([p["M_t_inv"] for p in pairs]), np.float64),
                    MtMc=np.ascontiguousarray(np.stack([p["MtMc_inv"] for p in pairs]), np.float64), X=cat("Xw", np.float64), cam=cat("cam", np.int32),
                    sig=cat("sigma2", np.float64), idx=cat("index1", np.int32), p=np.array([q[0] for q in params], np.float64),
                    mi=np.array([q[1] for q in params], np.int32), mx=np.array([q[2] for q in params], np.int32),
                    dr=None if draws is None else np.ascontiguousarray(np.concatenate([np.asarray(d, np.int32).reshape(-1) for d in draws])))
        self.keep = (Mc, ocs, off, arrs)
        pp = pkg.np_ptr
        self.h = C.c_void_p()
        pkg.check(L.mcs_sim3_create(ctx.h, nr, pp(Mc), ocs, ns, pp(self.n1), pp(off), pp(arrs["Mt"]), pp(arrs["MtMc"]), pp(arrs["p"]), pp(arrs["mi"]),
                                    pp(arrs["mx"]), pp(arrs["X"]), pp(arrs["cam"]), pp(arrs["sig"]), pp(arrs["idx"]), C.c_uint64(seed), pp(arrs["dr"]),
                                    C.byref(self.h)))
        self.pkg = pkg

    def __del__(self):
        self.L.mcs_sim3_destroy(self.h)

    def iterate(self, n):
        ns = len(self.pairs)
        pp = self.pkg.np_ptr
        nit = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (ns,)), np.int32)
        succ, nm, ni, T = np.zeros(ns, np.uint8), np.zeros(ns, np.uint8), np.zeros(ns, np.int32), np.full((ns, 16), -7.0)
        vb = np.zeros(int(self.n1.sum()), np.uint8)
        self.pkg.check(self.L.mcs_sim3_iterate(self.h, pp(nit), pp(succ), pp(nm), pp(ni), pp(T), pp(vb)))
        out, o = [], 0
        for k in range(ns):
            out.append((bool(succ[k]), bool(nm[k]), vb[o:o + self.n1[k]].astype(bool), int(ni[k]), T[k].reshape(4, 4) if succ[k] else None))
            assert succ[k] or (T[k] == -7.0).all()   # `result` untouched without success
            o += self.n1[k]
        return out

    def info(self):
        ns = len(self.pairs)
        n, mx, it = np.zeros(ns, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
        pp = self.pkg.np_ptr
        self.pkg.check(self.L.mcs_sim3_info(self.h, pp(n), pp(mx), pp(it)))
        return n, mx, it

    def hypotheses(self, s, first, count):
        N = len(self.pairs[s]["index1"])
        pp = self.pkg.np_ptr
        picks, cnt, hyp, inl = np.zeros((count, 3), np.int32), np.zeros(count, np.int32), np.zeros((count, 45)), np.zeros((count, N), np.uint8)
        self.pkg.check(self.L.mcs_sim3_hypotheses(self.h, s, first, count, pp(picks), pp(cnt), pp(hyp), pp(inl)))
        return picks, cnt, hyp, inl.astype(bool)


def pairs_for(rng, M_c, sizes, fracs):
    return [M.make_pair(rng, M_c, n, inlier_frac=f) for n, f in zip(sizes, fracs)]


def test_every_hypothesis_equals_the_model(env):
    G, pkg, cams = env["G"], env["pkg"], env["cams"]
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(11)
    sizes = [3, 4, 15, 16, 50, 300, 1000, 3000]
    fracs = [1.0, 0.75, 0.9, 0.5, 0.6, 0.4, 0.3, 0.6]
    pairs = pairs_for(rng, M_c, sizes, fracs)
    params = [(0.98, 3, 300)] * len(pairs)
    b = Batch(pkg, G.ctx(), cams, M_c, pairs, params, seed=99)
    n, mx, _ = b.info()
    assert n.tolist() == sizes
    near = 0
    for s, p in enumerate(pairs):
        m = M.model_of(p, cams, M_c)
        m.SetRansacParameters(*params[s])
        assert mx[s] == m.mRansacMaxIts
        near += compare_hypotheses(m, M.generated_draws(99, s, sizes[s]), b.hypotheses(s, 0, 300), 0, 300, "solver %d" % s)
    print("near-threshold pairs:", near)


def test_iteration_budget_at_12282(env):
    G, pkg, cams = env["G"], env["pkg"], env["cams"]
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(12)
    pairs = pairs_for(rng, M_c, [12281, 12282], [0.5, 0.5])
    b = Batch(pkg, G.ctx(), cams, M_c, pairs, [(0.98, 15, 300)] * 2, seed=5)
    assert b.info()[1].tolist() == [300, 1]
    m = M.model_of(pairs[1], cams, M_c)
    m.SetRansacParameters(0.98, 15, 300)
    compare_hypotheses(m, M.generated_draws(5, 1, 12282), b.hypotheses(1, 0, 4), 0, 4, "12282")
    out = b.iterate([0, 50])
    e = m.iterate(50, M.generated_draws(5, 1, 12282))
    assert out[1][:2] == e[:2] and out[1][3] == e[3] and np.array_equal(out[1][2], e[2])
    assert b.info()[2].tolist() == [0, m.mnIterations] and (out[1][0] or out[1][1])


def loop_pairs(rng, M_c):
    return pairs_for(rng, M_c, [14, 15, 16, 40, 120, 400, 900, 3000], [1.0, 1.0, 0.2, 0.5, 0.15, 0.3, 0.05, 0.4])


def test_loop_closer_rounds_and_odd_call_sizes(env):
    G, pkg, cams = env["G"], env["pkg"], env["cams"]
    M_c = M.rig_poses(3)
    pairs = loop_pairs(np.random.default_rng(13), M_c)
    ns = len(pairs)
    params = [(0.98, 15, 300)] * ns
    results = []
    for sizes in ([50], [1, 5, 7, 300], [7], [300]):
        b = Batch(pkg, G.ctx(), cams, M_c, pairs, params, seed=2024)
        models = []
        for s, p in enumerate(pairs):
            m = M.model_of(p, cams, M_c)
            m.SetRansacParameters(*params[s])
            models.append(m)
        draws = [M.generated_draws(2024, s, len(p["index1"])) for s, p in enumerate(pairs)]
        calls = run_rounds(b, models, draws, sizes)
        results.append((calls, [m.mnIterations for m in models], [m.mnBestInliers for m in models]))
        assert b.info()[2].tolist() == [m.mnIterations for m in models]
    print("calls per pattern:", [r[0] for r in results])


def test_caller_draws_including_degenerate_ones(env):
    G, pkg, cams = env["G"], env["pkg"], env["cams"]
    M_c = M.rig_poses(3)
    rng = np.random.default_rng(14)
    pairs = pairs_for(rng, M_c, [20, 64], [1.0, 0.5])
    pairs[0]["Xw"][19] = pairs[0]["Xw"][18]   # duplicate points: picks (19, 19, 18) give a NaN hypothesis
    pairs[0]["cam"][19] = pairs[0]["cam"][18]
    d0 = rng.integers(0, 20, (300, 3))
    d0[:4] = [[19, 19, 19], [0, 0, 0], [19, 19, 0], [5, 5, 5]]
    d1 = rng.integers(0, 64, (300, 3))
    params = [(0.98, 15, 300), (0.98, 15, 300)]
    b = Batch(pkg, G.ctx(), cams, M_c, pairs, params, seed=0, draws=[d0, d1])
    models = []
    for s, p in enumerate(pairs):
        m = M.model_of(p, cams, M_c)
        m.SetRansacParameters(*params[s])
        models.append(m)
    got = b.hypotheses(0, 0, 300)
    assert list(got[0][0]) == [19, 19, 18] and np.isnan(got[2][0, :12]).all() and got[1][0] == 0
    compare_hypotheses(models[0], M.table_draws(d0), got, 0, 300, "draws 0")
    compare_hypotheses(models[1], M.table_draws(d1), b.hypotheses(1, 0, 300), 0, 300, "draws 1")
    run_rounds(b, models, [M.table_draws(d0), M.table_draws(d1)], [50])


def test_eight_camera_batch_at_16000(env):
    G, pkg, cams = env["G"], env["pkg"], env["cams"]
    cams8 = [cams[c % 3] for c in range(8)]
    M_c = M.rig_poses(8)
    rng = np.random.default_rng(15)
    pairs = pairs_for(rng, M_c, [16000, 16000], [0.6, 0.3])
    params = [(0.98, 15, 300), (0.99, 300, 300)]
    b = Batch(pkg, G.ctx(), cams8, M_c, pairs, params, seed=77)
    assert b.info()[1].tolist() == [1, 300]   # the int conversion of SetRansacParameters: one iteration from N = 12 282 at (0.98, 15)
    for s in range(2):
        m = M.model_of(pairs[s], cams8, M_c)
        m.SetRansacParameters(*params[s])
        for first in (0, 150, 290):
            compare_hypotheses(m, M.generated_draws(77, s, 16000), b.hypotheses(s, first, 10), first, 10, "16000/%d" % s)


def test_end_to_end_loop_candidate(env):
    """DetectLoopCandidates -> SearchByBoW(KF, KF) -> cSim3Solver on the Lafida rig: the second keyframe sees the same multi-frame, its pose and map
    points are the first's moved by a known similarity; a quarter of its map points are moved elsewhere and must be rejected."""
    import gzip
    import os
    import shutil
    import tempfile
    G, FE = env["G"], env["FE"]
    io = importlib.import_module("multicol-slam_amd.io")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "voc.yml")
    with gzip.open(os.path.join(root, "tests", "golden", "small_orb_omni_voc_9_6.yml.gz"), "rb") as src, open(path, "wb") as dst:
        shutil.copyfileobj(src, dst)
    voc = FE.cORBVocabulary(io.load_vocabulary(path), ctx=G.ctx())
    shutil.rmtree(tmp)
    cams = env["cams"]
    M_c = M.rig_poses(3)
    models = [FE.cCamModelGeneral_.from_dict(c, G.synth.mirror_mask(c)) for c in cams]
    rng = np.random.default_rng(16)
    Mt1 = M.random_pose(rng)
    s_true, S = 1.7, M.random_pose(rng, 0.3)
    # rig 2's pose so that the rig frames satisfy X1c = s * X2c (same images, same rays): world points of KF2 = Sim(world points of KF1)
    rig1 = FE.cMultiCamSys_(models, M_c, Mt1)
    Mt2 = S @ Mt1
    rig2 = FE.cMultiCamSys_(models, M_c, Mt2)
    ex = FE.mdBRIEFextractorOct(1000, 1.2, 8, 25, 0, 0, 32, 20, False, 2, True, True, 32, ctx=G.ctx())
    imgs = G.synth.synth_multiframe(0, cams)
    F1 = FE.cMultiFrame(imgs, 0.0, [ex] * 3, voc, rig1, 0)
    F2 = FE.cMultiFrame(imgs, 0.04, [ex] * 3, voc, rig2, 1)
    others = [FE.cMultiFrame(G.synth.synth_multiframe(f, cams), 0.04 * f, [ex] * 3, voc, rig1, f) for f in (5, 9)]
    for F in [F1, F2] + others:
        F.ComputeBoW()
    K1, K2 = FE.cMultiKeyFrame(F1), FE.cMultiKeyFrame(F2)
    Ko = [FE.cMultiKeyFrame(F) for F in others]
    # map points along each keypoint's ray: X1c = M_c[cam] * (depth * ray); KF2's world point gives X2c = X1c / s in rig 2
    n = F1.totalN
    depth = rng.uniform(2.0, 6.0, n)
    moved = rng.random(n) < 0.25
    for i in range(n):
        c = int(F1.keypoint_to_cam[i])
        Xcam = depth[i] * np.asarray(F1.mvKeysRays[i], np.float64)
        X1c = M_c[c][:3, :3] @ Xcam + M_c[c][:3, 3]
        X2c = X1c / s_true
        if moved[i]:   # half its distance sideways (about 27 degrees off its ray, far beyond the 3 - 11 px thresholds)
            v = rng.normal(size=3)
            r = X2c / np.linalg.norm(X2c)
            v -= (v @ r) * r
            X2c = X2c + 0.5 * np.linalg.norm(X2c) * v / np.linalg.norm(v)
        mp1 = FE.cMapPoint(Mt1[:3, :3] @ X1c + Mt1[:3, 3])
        mp2 = FE.cMapPoint(Mt2[:3, :3] @ X2c + Mt2[:3, 3])
        mp1.AddObservation(K1, i)
        mp2.AddObservation(K2, i)
        K1.mvpMapPoints[i], K2.mvpMapPoints[i] = mp1, mp2
    db = FE.cMultiKeyFrameDatabase(voc, ctx=G.ctx())
    for k in [K1] + Ko:
        db.add(k)
    cands = db.DetectLoopCandidates(K2, 0.0, [])
    assert K1 in cands
    matcher = FE.cORBmatcher(0.75, True, 32, True, ctx=G.ctx())
    nmatches, vpMatches12 = matcher.SearchByBoW(K2, K1)   # current keyframe first, as cLoopClosing::ComputeSim3 does
    assert nmatches >= 15
    solver = FE.cSim3Solver(K2, K1, vpMatches12, rig2, ctx=G.ctx(), seed=3)
    solver.SetRansacParameters(0.98, 15, 300)
    for _ in range(20):
        ok, nomore, vb, ni, T = solver.iterate(50)
        if ok or nomore:
            break
    assert ok and ni > 15
    # X2c(K2) = s' R' X1c(K1) + t' with s' = 1 / s_true, R' = I, t' = 0
    assert abs(solver.GetEstimatedScale() - 1.0 / s_true) < 1e-6
    assert np.abs(solver.GetEstimatedRotation() - np.eye(3)).max() < 1e-6 and np.abs(solver.GetEstimatedTranslation()).max() < 1e-6
    idx = [i for i, mp in enumerate(vpMatches12) if mp is not None]
    assert not any(vb[i] and moved[i] for i in idx)          # every pair with a moved point is rejected
    assert sum(vb[i] for i in idx if not moved[i]) >= 0.8 * sum(1 for i in idx if not moved[i])
