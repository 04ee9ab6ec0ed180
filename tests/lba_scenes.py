"""The scenes of the LocalBundleAdjustment tests (tests/test_lba_cpu.py, tests/test_gpu_lba*.py) and the packing of an lba_model.Problem into the arguments of
mcs_local_bundle_adjustment.  Every seed below was found by a search over the MODEL (tools/lba_seed_search.py prints the table): the scene must show the path
its test is about and keep every decision at least lba_model.MARGIN from its edge.  The tests assert both again, on the model."""
import importlib

import numpy as np

import lba_model as LM
from poseopt_scenes import rig


def make(seed, kf_fixed, n_local, seen, nr=3, noise=0.5, n_outliers=0, start=0.01, pt_start=0.02, nlevels=8, extra_obs=None):
    """kf_fixed [n_kfs]; seen: per point the list of keyframes that observe it, in the reference's order (a keyframe listed twice holds the point at two
    features, of two cameras).  Keys = projection at the true estimate + noise (float32); free keyframes and all points start off the truth."""
    rng = np.random.default_rng(seed)
    cams, Mc = rig(nr)
    nk, P = len(kf_fixed), len(seen)
    true_pose = np.concatenate([rng.normal(0, 0.05, (nk, 3)), rng.normal(0, 0.4, (nk, 3))], 1)
    dirs = rng.normal(0, 1, (P, 3))
    true_pos = dirs / np.linalg.norm(dirs, axis=1)[:, None] * rng.uniform(2.0, 6.0, (P, 1))
    first, ekf, ecam = [0], [], []
    for ks in seen:
        used = {}
        for k in ks:
            c = int(rng.integers(0, nr))
            while c in used.get(k, ()):
                c = (c + 1) % nr
            used.setdefault(k, []).append(c)
            ekf.append(k)
            ecam.append(c)
        first.append(len(ekf))
    E = len(ekf)
    octave = rng.integers(0, nlevels, E).astype(np.int32)
    inv_sigma2 = 1.0 / (1.2 ** np.arange(nlevels)) ** 2
    pr = LM.Problem(true_pose, kf_fixed, n_local, true_pos, first, ekf, ecam, np.zeros((E, 2), np.float32), octave, Mc, cams, inv_sigma2, 2.0)
    ept, _ = pr.edge_point()
    e = LM.evaluate(pr, true_pose, true_pos, np.arange(E), ept, jac=False)      # xy = 0: e = -(u, v)
    xy = -e + rng.normal(0, noise, (E, 2))
    if n_outliers:
        bad = rng.choice(E, n_outliers, replace=False)
        xy[bad] += rng.normal(0, 40.0, (n_outliers, 2))
    pr.xy = xy.astype(np.float32)
    free = np.asarray(kf_fixed) == 0
    pr.kf_pose[free] += np.concatenate([rng.normal(0, start * 0.3, (int(free.sum()), 3)), rng.normal(0, start, (int(free.sum()), 3))], 1)
    pr.pos += rng.normal(0, pt_start, (P, 3))
    if extra_obs is not None:
        deg = np.diff(pr.pt_first)
        pr.total_obs = (deg + np.asarray(extra_obs)).astype(np.int32)
    return pr


def pair(seed=0, **kw):
    return make(seed, [1, 0], 2, [[0, 1]] * 12, nr=2, **kw)


def window(seed=0, **kw):
    rng = np.random.default_rng(500 + seed)
    seen = [sorted(rng.choice(6, 5, replace=False).tolist()) for _ in range(60)]
    return make(seed, [0, 0, 0, 0, 1, 1], 4, seen, nr=3, noise=0.5, n_outliers=6, **kw)


def slow(seed=0, **kw):
    rng = np.random.default_rng(600 + seed)
    seen = [sorted(rng.choice(5, 4, replace=False).tolist()) for _ in range(40)]
    return make(seed, [0, 0, 0, 1, 1], 3, seen, nr=3, noise=0.5, n_outliers=3, start=0.25, pt_start=0.3, **kw)


def twice(seed=0, **kw):
    """a point at two features of one keyframe (points 0, 1), a point with one edge (2), a point seen only by fixed keyframes (3), and ordinary ones"""
    seen = [[0, 0, 1, 2], [0, 1, 1, 3], [1], [2, 3]] + [[0, 1, 2, 3]] * 10 + [[0, 1]] * 4
    return make(seed, [0, 0, 1, 1], 2, seen, nr=3, **kw)


def split(seed=0, **kw):
    """two free keyframes that share no point: S has no off-diagonal block"""
    return make(seed, [0, 0, 1, 1], 2, [[0, 2, 3]] * 10 + [[1, 2, 3]] * 10, nr=2, **kw)


def hub(seed=0, **kw):
    """point 0 is held by 24 keyframes at three features each: 72 edges on one point"""
    rng = np.random.default_rng(700 + seed)
    seen = [[k for k in range(24) for _ in range(3)]] + [sorted(rng.choice(24, 4, replace=False).tolist()) for _ in range(120)]
    return make(seed, [0] * 20 + [1] * 4, 20, seen, nr=3, **kw)


def long_row(seed=0, **kw):
    """keyframe 0 holds 1025 edges"""
    rng = np.random.default_rng(800 + seed)
    seen = [[0, 2] + ([1] if rng.random() < 0.3 else []) + ([3] if rng.random() < 0.5 else []) for _ in range(1025)]
    return make(seed, [0, 0, 1, 1], 2, [sorted(s) for s in seen], nr=3, n_outliers=20, **kw)


def chain(n_free, seed=0, **kw):
    """n_free free keyframes in a chain, 8 points shared by each keyframe and the next (the last one's with a fixed keyframe); every point is also held by
    one of the two fixed keyframes, which keeps the chain well conditioned"""
    fixed = [0] * n_free + [1, 1]
    seen = [sorted({g, g + 1, n_free + (g + q) % 2}) for g in range(n_free) for q in range(8)]
    return make(seed, fixed, n_free, seen, nr=2, noise=0.3, **kw)


SCENES = {
    "pair": (pair, dict(seed=1)),
    "window": (window, dict(seed=0)),
    "slow": (slow, dict(seed=1)),
    "twice": (twice, dict(seed=0)),
    "split": (split, dict(seed=0)),
    "hub": (hub, dict(seed=0)),
    "long_row": (long_row, dict(seed=0)),
    "cap": (chain, dict(n_free=64, seed=0)),
}


def build(name):
    fn, kw = SCENES[name]
    return fn(**kw)


_model_cache = {}


def model(name, reverse=False, flag=None):
    """the model's result for a named scene, computed once and shared (callers do not modify it).  flag: None = NULL, else the caller's flag at entry"""
    key = (name, reverse, flag)
    if key not in _model_cache:
        f = None if flag is None else [bool(flag)]
        m = LM.optimize(build(name), stop_flag=f, reverse=reverse)
        m.flag_out = None if f is None else bool(f[0])
        _model_cache[key] = m
    return _model_cache[key]


def spread(name):
    """largest difference of the final poses and points between the model's sums in index order and in reversed order"""
    a, b = model(name), model(name, reverse=True)
    return max(float(np.abs(a.kf_pose - b.kf_pose).max()), float(np.abs(a.pos - b.pos).max()))


def keys_of(pr, cap):
    k = np.zeros(pr.n_edges, cap.KP_DTYPE)
    k["x"], k["y"], k["octave"] = pr.xy[:, 0], pr.xy[:, 1], pr.octave
    return k


def run_library(pkg, ctx, pr, device, flag=None, with_t=True):
    """mcs_local_bundle_adjustment through frontend.LocalBundleAdjustmentArrays -> its dict, or the error code"""
    fe = importlib.import_module("multicol-slam_amd.frontend")
    try:
        return fe.LocalBundleAdjustmentArrays(pr.kf_pose, pr.kf_fixed, pr.n_local, pr.pos, pr.pt_first, pr.edge_kf, pr.edge_cam, keys_of(pr, pkg._capi), pr.Mc_min,
                                              pr.cams, pr.inv_sigma2, pr.std_recon, total_obs=pr.total_obs, bad_obs=pr.bad_obs, stop_flag=flag, device=device,
                                              ctx=ctx, with_t=with_t)
    except pkg._capi.McsError as err:
        return err.code
