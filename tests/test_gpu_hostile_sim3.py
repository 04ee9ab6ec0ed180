"""-m gpu: the device Sim3 RANSAC (csrc/mcs_sim3.hip) against the model on the hostile scenes of tests/hostile_sim3.py, under the one rule of DESIGN.md
section 7: picks, counts and masks bit for bit outside the pairs the model flags as within 1e-9 of their threshold, the hypothesis doubles to 1e-9 relative,
NaN patterns and infinities equal; every output of every iterate() call, and mcs_sim3_best after every call.  tests/test_sim3_hostile_cpu.py asserts on the
model that every scene reaches what it is there for and that no scene driven through iterate() holds a flagged pair."""
import numpy as np
import pytest

import hostile_sim3 as T
from test_gpu_sim3 import Batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs)


class Device(Batch):
    """a scene of the table on the device, with the calls the plain parity tests do not make"""

    def __init__(self, env, sc):
        self.sc = sc
        super().__init__(env["pkg"], env["G"].ctx(), sc["cams"], sc["M_c"], sc["pairs"], sc["params"], sc["seed"], draws=sc["draws"])

    def set_params(self, params):
        pp = self.pkg.np_ptr
        p, mi, mx = np.array([q[0] for q in params], np.float64), np.array([q[1] for q in params], np.int32), np.array([q[2] for q in params], np.int32)
        self.pkg.check(self.L.mcs_sim3_set_ransac_parameters(self.h, pp(p), pp(mi), pp(mx)))

    def best(self):
        ns, pp = len(self.pairs), self.pkg.np_ptr
        R, t, s, T12 = np.full((ns, 9), -7.0), np.full((ns, 3), -7.0), np.full(ns, -7.0), np.full((ns, 16), -7.0)
        bi, it = np.full(ns, -7, np.int32), np.full(ns, -7, np.int32)
        self.pkg.check(self.L.mcs_sim3_best(self.h, pp(R), pp(t), pp(s), pp(T12), pp(bi), pp(it)))
        return R, t, s, T12, bi, it

    def iterate_without(self, n, inliers, T12):
        """mcs_sim3_iterate with inliers and / or T12 NULL -> (success, no_more, n_inliers[, T12][, inliers])"""
        ns, pp = len(self.pairs), self.pkg.np_ptr
        nit = np.ascontiguousarray(np.broadcast_to(np.asarray(n, np.int32), (ns,)), np.int32)
        succ, nm, ni, Tm = np.zeros(ns, np.uint8), np.zeros(ns, np.uint8), np.zeros(ns, np.int32), np.full((ns, 16), -7.0)
        vb = np.zeros(int(self.n1.sum()), np.uint8)
        self.pkg.check(self.L.mcs_sim3_iterate(self.h, pp(nit), pp(succ), pp(nm), pp(ni), pp(Tm) if T12 else None, pp(vb) if inliers else None))
        return succ.astype(bool), nm.astype(bool), ni, Tm, vb.astype(bool)


def check_scene(env, sc, count=None, sizes=None, unit=1.0, label=""):
    """mcs_sim3_hypotheses of every solver's first `count` iterations (all it is allowed by default), then iterate() rounds of `sizes` on a fresh batch"""
    b = Device(env, sc)
    models = T.models_of(sc)
    n, mx, _ = b.info()
    assert n.tolist() == [m.N for m in models] and mx.tolist() == [m.mRansacMaxIts for m in models]
    near = 0
    for s, m in enumerate(models):
        k = m.mRansacMaxIts if count is None else min(count, m.mRansacMaxIts)
        if k:
            near += T.compare_hypotheses(m, T.draws_of(sc, s), b.hypotheses(s, 0, k), 0, k, "%s solver %d" % (label, s), unit=unit)
    if sizes:
        b = Device(env, sc)
        models = T.models_of(sc)
        T.run_rounds(b, models, [T.draws_of(sc, s) for s in range(len(models))], sizes)
        assert b.info()[2].tolist() == [m.mnIterations for m in models]
        T.compare_best(b.best(), models, label)
    return near


def test_exact_triples(env):
    """group A: the exact-arithmetic degeneracies of computeT — NaN by 0 * inf, w == 0, a double top eigenvalue whose axis depends on every pivot tie"""
    assert check_scene(env, T.exact_scene(), sizes=[1, 4, 60], label="A") == 0


@pytest.mark.parametrize("factor", T.SCALE_FACTORS)
def test_world_scale(env, factor):
    """group B: the Jacobi solver's absolute stopping rule leaves it unrotated at 1e-9 and half-converged at 1e-7 and 1e-6: every operation of jacobi4 in
    the reference's order, or the answer differs outright.  Lengths are compared in units of the factor"""
    assert check_scene(env, T.scale_scene(factor), sizes=[7], unit=factor, label="B %g" % factor) == 0


def test_non_finite_points(env):
    """group C, per hypothesis only: NaN patterns and infinities of the 45 doubles equal, the poisoned pairs never inliers, everything else as usual"""
    sc = T.poison_scene()
    b = Device(env, sc)
    m = T.models_of(sc)[0]
    got = b.hypotheses(0, 0, T.POISON_ITERATIONS)
    T.compare_hypotheses(m, T.draws_of(sc, 0), got, 0, T.POISON_ITERATIONS, "C")
    assert not got[3][:, list(T.POISONED)].any()


def test_threshold_pairs(env):
    """group D, per hypothesis only: the pairs bisected to 1e-7 relative of their threshold are outside the band and decided as the model decides them"""
    sc = T.threshold_scene()
    b = Device(env, sc)
    m = T.models_of(sc)[0]
    got = b.hypotheses(0, 0, 4)
    near = T.compare_hypotheses(m, T.draws_of(sc, 0), got, 0, 4, "D")
    inside = [i for i, _, _, rel in T.THRESHOLD_TARGETS if rel == 0.0]
    assert near == 4 * len(inside)
    for i, _, _, rel in T.THRESHOLD_TARGETS:
        if rel != 0.0:
            assert (got[3][:, i] == (rel < 0)).all(), (i, rel)
    print("pairs inside the band, device / model:", got[3][0, inside].astype(int), m.evaluate(0, T.draws_of(sc, 0))[2][inside].astype(int))


@pytest.mark.parametrize("name", list(T.projection_rigs()))
def test_hostile_projection(env, name):
    """group E: the inlier test's projection under stretched, sheared, corner-principal-point, flipped and short / long / constant polynomial cameras, with
    transferred points on a camera axis (the 1e-14 branch), behind a camera and at grazing incidence"""
    assert check_scene(env, T.projection_scene(name), sizes=[5, 40], label="E " + name) == 0


def test_sigma_edges(env):
    """group F: thresholds 0 (never an inlier), 1 and 9.21e15"""
    assert check_scene(env, T.sigma_scene(), sizes=[40], label="F") == 0


def test_sigma2_the_reference_cannot_convert_is_refused(env):
    """mcs_sim3_create refuses 9.210 sigma^2 that is NaN, negative or >= 2^64 on the host, before anything is launched; just below 2^64 is accepted"""
    sc = T.sigma_scene()
    for v in T.REFUSED_SIGMA2:
        for side in (0, 1):
            pair = dict(sc["pairs"][0], sigma2=sc["pairs"][0]["sigma2"].copy())
            pair["sigma2"][37, side] = v
            with pytest.raises(env["pkg"].McsError):
                Device(env, dict(sc, pairs=[pair]))
    pair = dict(sc["pairs"][0], sigma2=sc["pairs"][0]["sigma2"].copy())
    pair["sigma2"][37] = (T.LARGEST_SIGMA2, 0.0)
    ok = dict(sc, pairs=[pair])
    assert check_scene(env, ok, count=4, label="largest sigma2") == 0


def test_mask_word_sizes(env):
    """group G: N = 3, 63, 64, 65, 127, 128, 129 in one batch"""
    assert check_scene(env, T.word_scene(), sizes=[7, 1, 40], label="G words") == 0


def test_130_solvers(env):
    """group G: more solvers than one k_sim3_scan block, an empty solver in the middle, one below minInliers, slot totals that are no multiple of 4"""
    sc = T.many_scene()
    assert check_scene(env, sc, count=3, sizes=list(T.MANY_CALLS), label="G many") == 0


def test_one_and_32_cameras(env):
    assert check_scene(env, T.one_camera_scene(), sizes=[40], label="G 1 camera") == 0
    assert check_scene(env, T.many_camera_scene(), sizes=[40], label="G 32 cameras") == 0


def test_null_outputs(env):
    """group G: inliers = NULL and T12 = NULL change nothing else"""
    sc = T.word_scene()
    want = Device(env, sc).iterate_without(40, True, True)
    assert want[0].any()
    for inliers, T12 in ((False, True), (True, False), (False, False)):
        got = Device(env, sc).iterate_without(40, inliers, T12)
        assert all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))
        assert np.array_equal(got[3], want[3]) if T12 else (got[3] == -7.0).all()
        assert np.array_equal(got[4], want[4]) if inliers else not got[4].any()


def test_state_with_caller_draws(env):
    """group H: the script of hostile_sim3.STATE_SCRIPT_DRAWS in lockstep — the NaN best hypothesis after the first call, SetRansacParameters mid-run
    (a higher minInliers, minInliers > N, back again) and the refused calls, which must leave the state untouched"""
    sc = T.exact_scene()
    _, near, refusals = T.drive_state(sc, T.STATE_SCRIPT_DRAWS, Device(env, sc))
    assert near == 0 and refusals == 2


def test_state_with_generated_draws(env):
    sc = T.state_scene()
    _, near, _ = T.drive_state(sc, T.STATE_SCRIPT_SEED, Device(env, sc))
    assert near == 0
