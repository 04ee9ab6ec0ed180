"""The scenes of the essential-graph tests (tests/test_essgraph_cpu.py, tests/test_gpu_essgraph.py) with their seeds (tools/essgraph_seed_search.py found them).

A scene is a trajectory on a circle whose estimate drifts, a loop between its last keyframe and an early one, the correction `D` of the last few keyframes
(CorrectedSim3 = Scw * D, NonCorrectedSim3 = Scw as it was, as cLoopClosing::CorrectLoop propagates them), and the edge list in the reference's order: the
LoopConnections edges (kind 0) first, then per keyframe its spanning-tree edge, its earlier loop edges and its covisibility edges (kind 1)."""
import importlib

import numpy as np

import essgraph_model as M

# Every decision of a scene's model run, in every run of the spread, stays at least this far (relative) from its edge.  rho and the gain are formed from chi2
# sums behind a solve: 1e-3, twenty times the largest spread a scene may have (MAX_SPREAD; twice that is the 1e-4 the tolerance may never exceed).  A branch
# of exp / log, a quaternion case and an LU pivot are decided on quantities of ONE evaluation at the current estimates, which move between the runs as the
# estimates do: at least 1e-5 AND at least twice the scene's own spread (measure() applies the second part).  A scene of 150 keyframes takes some 10^6 LU
# pivot decisions per run, among them those of wild rejected trials: a wider fixed margin leaves no seed.
MARGIN = dict(rho=1e-3, gain=1e-3, branch=1e-5, quat=1e-5, pivot=1e-5)
LOCAL = ("branch", "quat", "pivot")
MAX_SPREAD = 5e-5


def margin_ratio(m):
    """the smallest decision margin of a model result in units of its MARGIN: at least 1 for a scene that may be used"""
    return min(m.margins.m[k] / MARGIN[k] for k in MARGIN)


RUNS = [dict(reverse=False, seed=None), dict(reverse=True, seed=None)] + [dict(reverse=False, seed=s) for s in range(1, 9)]


def _rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)


def make(seed, K, corrected, loops, fixed, covis=2, old_loops=(), dup=False, isolated=None, n_points=40, drift=0.004, extra_edges=()):
    """corrected: {keyframe: (angle, translation scale, s)} — the correction D of that keyframe; loops: [(i, j)] LoopConnections (i the corrected side);
    old_loops: [(i, l)] with l < i, GetLoopEdges of earlier closures; isolated: a keyframe that gets no edge at all"""
    rng = np.random.default_rng(seed)
    Rwc, twc = np.eye(3), np.zeros(3)
    Scw = np.zeros((K, 8))
    for k in range(K):
        if k:
            step = _rot([0.1 * rng.normal(), 1.0, 0.1 * rng.normal()], 2 * np.pi / max(K, 12) + drift * rng.normal())
            twc = twc + Rwc @ (np.array([1.0, 0.0, 0.05 * rng.normal()]) * (1.0 + 3 * drift * k / K))
            Rwc = Rwc @ step
        Rcw = Rwc.T
        Scw[k] = M.sim3_vec(M.sim3_from_rts(Rcw.reshape(9), -Rcw @ twc, 1.0))
    Snc, has_nc = Scw.copy(), np.zeros(K, np.uint8)
    for k, (ang, tr, s) in corrected.items():
        D = M.sim3_from_rts(_rot(rng.normal(0, 1, 3), ang).reshape(9), tr * rng.normal(0, 1, 3), float(s))
        Scw[k] = M.sim3_vec(M.sim3_mul(M.sim3_of(Snc[k]), D))
        has_nc[k] = 1
    kf_fixed = np.zeros(K, np.uint8)
    kf_fixed[list(fixed)] = 1
    ei, ej, kind = [], [], []
    for a, b in loops:
        ei.append(a), ej.append(b), kind.append(0)
    parent = {}
    chain = [k for k in range(K) if k != isolated]
    for n, k in enumerate(chain):
        if n:
            parent[k] = chain[n - 1]
    for k in chain:
        if k in parent:
            ei.append(k), ej.append(parent[k]), kind.append(1)
        for a, l in old_loops:
            if a == k:
                ei.append(k), ej.append(l), kind.append(1)
        for c in range(2, covis + 1):
            n = chain.index(k) - c
            if n >= 0:
                ei.append(k), ej.append(chain[n]), kind.append(1)
        if dup:
            for a, b in loops:
                if a == k and b < k:                             # the loop pair is covisible as well: a second, parallel edge (kind 1)
                    ei.append(a), ej.append(b), kind.append(1)
    for a, b, c in extra_edges:
        ei.append(a), ej.append(b), kind.append(c)
    pos = rng.normal(0, 3, (n_points, 3))
    ref = rng.integers(0, K, n_points).astype(np.int32)
    ref[::7] = -1
    return M.Problem(Scw, Snc, has_nc, kf_fixed, ei, ej, kind, pos, ref)


def _tail(K, n, ang, tr, s):
    return {k: (ang, tr, s) for k in range(K - n, K)}


def chain6(seed):
    return make(seed, 6, _tail(6, 2, 0.02, 0.15, 1.02), [(5, 0)], [0], covis=1)


def dup(seed):
    return make(seed, 6, _tail(6, 2, 0.02, 0.15, 1.02), [(5, 0)], [0], covis=1, dup=True)


def isolated(seed):
    return make(seed, 7, _tail(7, 2, 0.02, 0.15, 0.98), [(6, 0)], [0], covis=1, isolated=3)


def fixed_mid(seed):
    return make(seed, 8, _tail(8, 2, 0.02, 0.15, 1.02), [(7, 3)], [3], covis=2)


def scale(seed):
    return make(seed, 9, {5: (0.2, 0.1, 1.0), 6: (1e-3, 0.1, 1.07), 7: (0.3, 0.2, 0.93), 8: (0.3, 0.2, 0.93)}, [(8, 0), (7, 0)], [0], covis=2)


def panels(seed):
    return make(seed, 12, _tail(12, 3, 0.02, 0.2, 1.03), [(11, 0), (10, 0)], [0], covis=2)


def big(seed):
    return make(seed, 150, _tail(150, 6, 0.03, 0.4, 1.04), [(149, 3), (149, 4), (148, 3)], [3], covis=3, old_loops=[(90, 20)], n_points=300, drift=0.002)


def identity(seed):
    """nothing to correct, and in numbers whose products are exact (unit rotations, whole translations): every residual is exactly 0, so b = 0, x = 0 and
    rho = 0 / 1e-3 = 0 — solve() returns Terminate behind one trial of iteration 0 in any arithmetic.  Its decisions sit ON their edges by construction;
    the margin rule does not apply to it"""
    pr = make(seed, 6, {}, [(5, 0)], [0], covis=1)
    pr.Scw[:] = 0.0
    pr.Scw[:, 3] = pr.Scw[:, 7] = 1.0
    pr.Scw[:, 4:7] = [[k, 2 * k, -k] for k in range(6)]
    pr.Snc[:] = pr.Scw
    return pr


SCENES = {
    "chain6": (chain6, 6),
    "dup": (dup, 0),
    "isolated": (isolated, 2),
    "fixed_mid": (fixed_mid, 0),
    "scale": (scale, 0),
    "panels": (panels, 1),
    "big": (big, 8),
    "identity": (identity, 0),
}


def build(name, seed=None):
    fn, s = SCENES[name]
    return fn(s if seed is None else seed)


_cache = {}


def _run(job):
    name, run = job
    r = RUNS[run]
    return M.optimize(build(name), lm=M.Libm(r["seed"]), reverse=r["reverse"])


def model(name, run=0):
    """the model's result for a named scene under RUNS[run], computed once and shared (callers do not modify it)"""
    if (name, run) not in _cache:
        _cache[(name, run)] = _run((name, run))
    return _cache[(name, run)]


FIELDS = ("Scw_out", "pose", "kf_t", "pos")


def rel(a, b):
    """largest difference of two arrays relative to the larger one's largest entry"""
    return float(np.abs(a - b).max() / max(np.abs(a).max(), np.abs(b).max(), 1e-300)) if np.size(a) else 0.0


def differences(a, b):
    d = {k: rel(getattr(a, k), getattr(b, k)) for k in FIELDS}
    d["lam"], d["chi2"] = abs(a.lam - b.lam) / max(abs(b.lam), 1e-300), abs(a.chi2 - b.chi2) / max(abs(b.chi2), 1e-300)
    return d


def measure(results):
    """(spread, margin, decisions agree) of one scene's runs: the largest relative difference of an output, lambda or chi2 from the first run's; the smallest
    decision margin over all runs in units of MARGIN; whether every run took the same decisions"""
    base = results[0]
    same = all(r.status == base.status and r.iters == base.iters and r.stop == base.stop and r.trials == base.trials and r.branches == base.branches
               and r.pivots == base.pivots for r in results)
    if base.status != M.EG_OK or not same:
        return float("inf"), 0.0, same
    spread = max(max(differences(r, base).values()) for r in results[1:])
    local = min(r.margins.m[k] for r in results for k in LOCAL)
    return spread, min(min(margin_ratio(r) for r in results), local / max(2.0 * spread, 1e-300)), same


def spread(name):
    """measure() of a named scene's ten runs.  A scene of 50 keyframes or more computes the runs it lacks side by side, in fresh interpreters that load the
    model alone (no GPU): each takes seconds."""
    missing = [(name, k) for k in range(len(RUNS)) if (name, k) not in _cache]
    if len(missing) > 1 and len(build(name).Scw) >= 50:
        import concurrent.futures
        import multiprocessing
        import os
        keep = os.environ.get("OPENBLAS_NUM_THREADS")
        os.environ["OPENBLAS_NUM_THREADS"] = "1"               # read by the children's numpy as it loads: ten runs side by side, one thread each
        try:
            with concurrent.futures.ProcessPoolExecutor(max_workers=len(missing), mp_context=multiprocessing.get_context("spawn")) as ex:
                for job, res in zip(missing, ex.map(_run, missing)):
                    _cache[job] = res
        finally:
            if keep is None:
                del os.environ["OPENBLAS_NUM_THREADS"]
            else:
                os.environ["OPENBLAS_NUM_THREADS"] = keep
    return measure([model(name, k) for k in range(len(RUNS))])


def run_library(pkg, ctx, pr, device):
    """mcs_optimize_essential_graph through frontend.OptimizeEssentialGraphArrays -> its dict, or the error code"""
    fe = importlib.import_module("multicol-slam_amd.frontend")
    try:
        return fe.OptimizeEssentialGraphArrays(*pr.arrays(), device=device, ctx=ctx)
    except pkg._capi.McsError as err:
        return err.code
