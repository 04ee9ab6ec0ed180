"""The scenes of the OptimizeSim3 tests (tests/test_sim3opt_cpu.py, tests/test_gpu_sim3opt*.py) and the packing of a sim3opt_model.Problem into the arguments of
mcs_sim3_optimize.  Every seed below was found by a search over the MODEL (tools/sim3opt_seed_search.py prints the table): the scene must show the property
its test is about.  The CPU test derives the tolerance from these scenes and asserts which of them keep every decision further from its edge than that."""
import ctypes as C
import importlib
import math

import numpy as np

import poseopt_model as PM
import sim3opt_model as M

T = 256   # kSim3OptThreads (csrc/mcs_sim3opt.h): the stride of a thread's correspondences
BATCH = 64   # kSim3OptBatch: problems per launch


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def hom(R, t):
    Mh = np.eye(4)
    Mh[:3, :3], Mh[:3, 3] = R, t
    return Mh


def rig(nr):
    """cameras and M_c [nr][4][4]: the Lafida rig for nr <= 3, else its cameras in turn on a ring"""
    import test_io_formats as TI
    synth = importlib.import_module("multicol-slam_amd.synth")
    cams = synth.lafida_cameras()
    if nr <= 3:
        return cams[:nr], np.stack([PM.cayley2hom(np.array(c, np.float64)) for c in TI.CAYLEY[:nr]])
    return [cams[c % 3] for c in range(nr)], np.stack([hom(rot([0.1, 1.0, 0.05], 2 * math.pi * c / nr), [0.1 * math.cos(c), 0.01 * c, 0.1 * math.sin(c)])
                                                       for c in range(nr)])


def scene(seed, n, nr=3, noise=0.5, n_outliers=0, start=0.02, angle=0.3, std_sim=4.0, outlier_px=25.0, nlevels=8):
    """Two keyframes that see the same n physical points, each in its own map: P1 = S12 * P2 in the rig frames.  obs = projection + noise (float32), the
    weights are GetInvSigma2(octave1) and GetSigma2(octave2) as the reference passes them, the start is the true S12 times a small Sim3.
    angle: the rotation of the true S12 (above 2.1 its trace is negative)."""
    rng = np.random.default_rng(seed)
    cams, Mc = rig(nr)
    inv_Mc = [PM.inv_mat(m) for m in Mc]
    ax = rng.normal(0, 1, 3)
    R_true, t_true, s_true = rot(ax, angle), rng.normal(0, 0.3, 3), float(np.exp(rng.normal(0, 0.1)))
    S_true = M.sim3_from_rts(R_true, t_true, s_true)
    S_inv = M.sim3_inverse(S_true)
    Mt = [hom(rot(rng.normal(0, 1, 3), rng.uniform(0, 0.5)), rng.normal(0, 1.0, 3)) for _ in range(2)]
    Xw, cam, obs, w = np.zeros((n, 2, 3)), np.zeros((n, 2), np.int32), np.zeros((n, 2, 2)), np.zeros((n, 2))
    sigma2 = (1.2 ** np.arange(nlevels)) ** 2
    octave = np.zeros((n, 2), np.int32)
    for i in range(n):
        c1 = int(rng.integers(0, nr))
        th, ph, r = rng.uniform(0.35, 1.0), rng.uniform(0, 2 * np.pi), rng.uniform(1.5, 6.0)
        pc = np.array([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th), 1.0])
        P1 = (Mc[c1] @ pc)[:3]
        P2 = np.array(M.sim3_map(S_inv, [float(v) for v in P1]))
        c2 = int(np.argmax([(inv_Mc[c] @ np.append(P2, 1.0))[2] / np.linalg.norm((inv_Mc[c] @ np.append(P2, 1.0))[:3]) for c in range(nr)]))
        Xw[i, 0], Xw[i, 1] = (Mt[0] @ np.append(P1, 1.0))[:3], (Mt[1] @ np.append(P2, 1.0))[:3]
        cam[i] = [c1, c2]
        octave[i] = [rng.integers(0, nlevels), rng.integers(0, nlevels)]
        w[i] = [1.0 / sigma2[octave[i, 0]], sigma2[octave[i, 1]]]                # GetInvSigma2(octave1), GetSigma2(octave2)
    pr = M.Problem(Xw, cam, obs, w, Mc, cams, [PM.inv_mat(m) for m in Mt], R_true, t_true, s_true, std_sim)
    if n:
        idx = np.arange(n)
        P1, P2 = M.rig_points(pr, idx)
        e = M.errors(pr, S_true, S_inv, idx, P1, P2, inv_Mc)     # obs = 0: e = -projection
        o = -e + rng.normal(0, noise, (n, 2, 2))
        if n_outliers:
            bad = rng.choice(n, n_outliers, replace=False)
            o[bad, rng.integers(0, 2, n_outliers)] += rng.normal(0, outlier_px, (n_outliers, 2))
        pr.obs = o.astype(np.float32).astype(np.float64)
    d = np.concatenate([rng.normal(0, start * 0.3, 3), rng.normal(0, start, 3), rng.normal(0, start * 0.3, 1)])
    S0 = M.sim3_mul(M.sim3_exp(d), S_true)
    pr.R12, pr.t12, pr.s12 = M.quat_to_mat(S0[0]), np.array(S0[1]), S0[2]
    pr.true = M.sim3_vec(S_true)
    pr.octave, pr.sigma2, pr.Mt = octave, sigma2, np.stack(Mt)
    return pr


# name -> kwargs of scene().  Sizes: 0 / 2 the under-three path, 3 the smallest that optimises twice, 63 / 64 / 65 the wave boundary, T - 1 / T / T + 1 and
# 2 T + 1 the stride boundary; rigs of 1, 3 and 32 cameras.
FAR = dict(std_sim=100.0, start=2.0, outlier_px=3000.0)   # a wide Huber bound and a far start: round one uses its 5 iterations, so round two runs
SIZES = {
    "n0": dict(seed=0, n=0, nr=3),
    "n2": dict(seed=0, n=2, nr=3),
    "n3": dict(seed=0, n=3, nr=1, **FAR),
    "n63": dict(seed=1, n=63, nr=3, n_outliers=4, **FAR),
    "n64": dict(seed=0, n=64, nr=1, n_outliers=4, **FAR),
    "n65": dict(seed=5, n=65, nr=32, n_outliers=4, **FAR),
    "n255": dict(seed=3, n=T - 1, nr=3, n_outliers=20, **FAR),
    "n256": dict(seed=0, n=T, nr=3, n_outliers=20, **FAR),
    "n257": dict(seed=2, n=T + 1, nr=3, n_outliers=20, **FAR),
    "n513": dict(seed=4, n=2 * T + 1, nr=3, n_outliers=40, **FAR),
}
# one scene per path; what each shows is asserted in tests/test_sim3opt_cpu.py
PATHS = {
    "nbad0": dict(seed=0, n=40, nr=3, **FAR),                                          # no correspondence is bad: round two may run 5 iterations
    "nbad": dict(seed=1, n=6, nr=3, n_outliers=2, std_sim=100.0, start=1.0, outlier_px=3000.0),   # some are: 10, and round two needs more than 5
    "return0": dict(seed=0, n=5, nr=3, n_outliers=3, outlier_px=60.0),                 # fewer than 3 left after round one
    "dead_round_two": dict(seed=2, n=40, nr=3, n_outliers=3),                          # the default bound: round one ends on the gain test
    "far_start": dict(seed=40, n=40, nr=3, n_outliers=3, std_sim=100.0, start=3.0, outlier_px=3000.0),   # Levenberg rejects trials on the way
    "tiny_step": dict(seed=1, n=40, nr=3, noise=1e-4, start=1e-6),                     # the first step has |sigma| < 1e-5 and theta < 1e-5
    "negative_trace": dict(seed=0, n=40, nr=3, n_outliers=3, angle=2.9),               # Quaterniond(R) through its other cases
}
ALL = {**SIZES, **PATHS}


def build(name):
    return scene(**ALL[name])


_model_cache = {}


def model(name, reverse=False, seed=None, fix=()):
    """the model's result for a named scene, computed once and shared (callers do not modify it)"""
    key = (name, reverse, seed, tuple(sorted(fix)))
    if key not in _model_cache:
        _model_cache[key] = M.optimize(build(name), reverse=reverse, fix=fix, lm=M.EXACT if seed is None else M.Libm(seed))
    return _model_cache[key]


SEEDS = range(8)


def value(m, what):
    return m.S12 if what == "S12" else np.array([m.lam if what == "lam" else m.chi2])


def spread(name, what="S12"):
    """the model's own uncertainty on a scene: the largest relative difference of S12 (or of the final lambda, or of the last chi2) between the plain run and
    the run with reversed edge sums and the runs under the eight perturbation seeds (sim3opt_model.ULP)"""
    base = value(model(name), what)
    rel = M.rel_spread if what == "S12" else lambda a, b: float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)))
    return max([rel(base, value(model(name, reverse=True), what))] + [rel(base, value(model(name, seed=s), what)) for s in SEEDS])


_bound = {}


def bound(what="S12"):
    """what the device may differ by: twice the largest spread over every scene of the table (its tree of partial sums is a third ordering)"""
    if what not in _bound:
        _bound[what] = 2.0 * max(spread(n, what) for n in ALL)
    return _bound[what]


def stable(name):
    """whether the runs that measure the spread took the same decisions as the plain run"""
    m = model(name)
    for o in [model(name, reverse=True)] + [model(name, seed=s) for s in SEEDS]:
        if not (np.array_equal(o.keep, m.keep) and o.iters == m.iters and o.stop == m.stop and np.array_equal(o.trials, m.trials) and o.n_inliers == m.n_inliers):
            return False
    return True


def enqueue(pkg, ctx, problems, device, with_R=True, with_diag=True):
    """mcs_sim3_optimize over a list of problems that share the rig -> (the call's code, a function that reads the outputs: list of dicts S12, R12, keep,
    n_inliers, diag).  In device kind nothing is read before that function is called."""
    cap = pkg._capi
    fe = importlib.import_module("multicol-slam_amd.frontend")
    mem = fe._DEVICE if device else fe._HOST
    L = pkg.lib()
    npb, p0 = len(problems), problems[0]
    nr = len(p0.Mc)
    ocs = (cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams])
    g = dict(Mc=p0.Mc.reshape(nr, 16), ocs=np.frombuffer(ocs, np.uint8).copy(), Mt=np.array([p.Mt_inv for p in problems]).reshape(npb, 32),
             std=np.array([p.std_sim for p in problems], np.float64), R=np.array([p.R12 for p in problems]).reshape(npb, 9),
             t=np.array([p.t12 for p in problems]).reshape(npb, 3), s=np.array([p.s12 for p in problems], np.float64), S=np.full((npb, 8), -7.0),
             Ro=np.zeros((npb, 9)), nin=np.full(npb, -7, np.int32), diag=np.zeros(npb, cap.SIM3OPT_DIAG_DTYPE))
    g = {k: mem.put(np.ascontiguousarray(v)) for k, v in g.items()}
    per = [dict(Xw=mem.put(p.Xw.reshape(-1)), cam=mem.put(p.cam.astype(np.int32).reshape(-1)), obs=mem.put(p.obs.reshape(-1)), w=mem.put(p.w.reshape(-1)),
                keep=mem.put(np.full(max(p.n, 1), 9, np.uint8))) for p in problems]
    pr = (cap.Sim3OptProblem * npb)(*[cap.Sim3OptProblem(*[mem.ptr(q[k]) if p.n else None for k in ("Xw", "cam", "obs", "w")], p.n) for q, p in zip(per, problems)])
    outs = (C.c_void_p * npb)(*[mem.ptr(q["keep"]) for q in per])
    rc = L.mcs_sim3_optimize(ctx.h, npb, pr, mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["Mt"]), mem.ptr(g["std"]), mem.ptr(g["R"]), mem.ptr(g["t"]),
                             mem.ptr(g["s"]), mem.kind, mem.ptr(g["S"]), mem.ptr(g["Ro"]) if with_R else None, outs, mem.ptr(g["nin"]),
                             mem.ptr(g["diag"]) if with_diag else None)

    def read():
        r = {k: mem.read(g[k]) for k in ("S", "Ro", "nin", "diag")}
        return [dict(S12=r["S"][i], R12=r["Ro"][i].reshape(3, 3), keep=mem.read(per[i]["keep"])[:problems[i].n], n_inliers=int(r["nin"][i]), diag=r["diag"][i])
                for i in range(npb)]
    return rc, read


def run_library(pkg, ctx, problems, device, **kw):
    """enqueue() and read: the list of dicts, or the error code"""
    rc, read = enqueue(pkg, ctx, problems, device, **kw)
    return rc if rc != 0 else read()


# ---------------------------------------------------------------------------------------------- keyframe stand-ins (frontend.OptimizeSim3, the C++ facade)
class MapPoint:
    def __init__(self, X, bad=False, kf=None, idx=-1):
        self.X, self.bad, self.kf, self.idx = np.asarray(X, np.float64), bad, kf, idx

    def GetWorldPos(self):
        return self.X

    def isBad(self):
        return self.bad

    def GetIndexInKeyFrame(self, kf):
        return [self.idx] if kf is self.kf and self.idx >= 0 else []


class KeyFrame:
    """what OptimizeSim3 reads of a cMultiKeyFrame"""

    def __init__(self, camSystem, keys, k2c, sigma2):
        self.camSystem, self.mvKeys, self.keypoint_to_cam, self.mvpMapPoints = camSystem, keys, np.asarray(k2c, np.int32), []
        self.mvLevelSigma2, self.mvInvLevelSigma2 = [float(v) for v in sigma2], [1.0 / float(v) for v in sigma2]

    def GetMapPointMatches(self):
        return self.mvpMapPoints

    def GetKeyPoint(self, i):
        return self.mvKeys[i]

    def GetSigma2(self, level):
        return self.mvLevelSigma2[level]

    def GetInvSigma2(self, level):
        return self.mvInvLevelSigma2[level]


def keyframes(pr, make_rig, kp_dtype, seed=0):
    """Two keyframe stand-ins and vpMatches1 whose surviving correspondences are exactly those of `pr`, in its order, among five entries the pointer tests of
    :117-156 drop (no match, no point on side 1, a bad point on either side, a match keyframe 2 does not observe).  Keyframe 2's features are a permutation of
    keyframe 1's, and the cameras are stored so that the reference's CROSSED lookups (keypoint_to_cam1[i2], keypoint_to_cam2[i]) give pr.cam: a wrapper that
    looks each camera up by its own side's index gets other cameras.  make_rig(M_t) -> a camSystem.  -> (pKF1, pKF2, vpMatches1, feature index of each
    correspondence, the indices the filter drops)"""
    rng = np.random.default_rng(100 + seed)
    n1 = pr.n + 5
    drop = sorted(rng.choice(n1, 5, replace=False).tolist())
    at = [i for i in range(n1) if i not in drop]
    perm = rng.permutation(n1)
    k1, k2 = np.zeros(n1, kp_dtype), np.zeros(n1, kp_dtype)
    c1, c2 = rng.integers(0, len(pr.Mc), n1).astype(np.int32), rng.integers(0, len(pr.Mc), n1).astype(np.int32)
    for k, i in enumerate(at):
        k1["x"][i], k1["y"][i], k1["octave"][i] = pr.obs[k, 0, 0], pr.obs[k, 0, 1], pr.octave[k, 0]
        k2["x"][perm[i]], k2["y"][perm[i]], k2["octave"][perm[i]] = pr.obs[k, 1, 0], pr.obs[k, 1, 1], pr.octave[k, 1]
        c1[perm[i]], c2[i] = pr.cam[k, 0], pr.cam[k, 1]           # crossed, as the reference reads them
    kf1, kf2 = KeyFrame(make_rig(pr.Mt[0]), k1, c1, pr.sigma2), KeyFrame(make_rig(pr.Mt[1]), k2, c2, pr.sigma2)
    matches = []
    for i in range(n1):
        if i in drop:
            kind = drop.index(i)
            kf1.mvpMapPoints.append(None if kind == 1 else MapPoint(rng.normal(0, 1, 3), bad=kind == 2))
            matches.append(None if kind == 0 else MapPoint(rng.normal(0, 1, 3), bad=kind == 3, kf=kf2, idx=-1 if kind == 4 else int(perm[i])))
        else:
            k = at.index(i)
            kf1.mvpMapPoints.append(MapPoint(pr.Xw[k, 0]))
            matches.append(MapPoint(pr.Xw[k, 1], kf=kf2, idx=int(perm[i])))
    return kf1, kf2, matches, at, drop
