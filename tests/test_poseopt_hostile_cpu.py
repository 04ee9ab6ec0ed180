"""CPU: the model of cOptimizer::PoseOptimization (tests/poseopt_model.py) on every scene of tests/hostile_poseopt.py, no device.  Each scene shows the
property it is in the table for (so a re-seeded scene cannot pass vacuously), the groups meet their floors, every scene that EXCUSED does not name keeps its
decisions poseopt_model.MARGIN from their edges, the hostile projections equal the oracle's (and the reference's) bit for bit, the Jacobian holds against a
central difference on the stretched cameras and the scaled worlds, the margin metric is never NaN, and the first evaluation's screen is the decided
one."""
import ctypes as C
import math

import numpy as np
import pytest

import hostile_poseopt as H
import poseopt_model as PM
import poseopt_scenes as S
from test_poseopt_cpu import REF_SO, have_ref

T, NB, ITS, NOT_RUN = PM.STOP_TRIALS, PM.STOP_NBAD, PM.STOP_ITERATIONS, PM.STOP_NOT_RUN


def _unchanged(m, pr):
    return m.pose.tobytes() == pr.pose0.tobytes()


def _nonfinite(m, pr):
    return (m.status == PM.POSE_NONFINITE and _unchanged(m, pr) and m.n_inliers == m.nInitial == 65 and m.share == 0.0 and not m.outlier.any()
            and m.iters == [0, 0] and m.stop == [NOT_RUN, NOT_RUN] and m.lam == 0.0 and m.chi2 == 0.0)


def _far(m, pr):   # rejected trials, every edge flagged by the first pass, round two never starts
    return (m.status == 0 and m.trials[0].max() >= 4 and (m.trials[0] > 1).sum() >= 2 and m.n_active == [65, 0] and m.iters == [10, 0] and m.stop[1] == NOT_RUN
            and m.n_inliers == 0 and m.outlier.sum() == 65)


def _special_at_start(pr):   # the camera-frame points of the lattice scenes' special features at the start pose
    inv = PM.rig_from_min(pr.pose0, pr.Mc_min)[1][0]
    X = pr.pos[pr.points[pr.special]]
    return np.stack([((inv[r, 0] * X[:, 0] + inv[r, 1] * X[:, 1]) + inv[r, 2] * X[:, 2]) + inv[r, 3] for r in range(3)], 1)


def _ten_rejected_trials_twice(m, pr):
    return (m.status == 0 and m.iters == [1, 1] and m.stop == [T, T] and m.trials[0, 0] == 10 == m.trials[1, 0] and m.failed_solves == 0 and _unchanged(m, pr)
            and m.lam > 1e30 and 0 < m.n_inliers < 65)


WANT = {
    "A.weights_zero": lambda m, pr: (m.status == 0 and m.iters == [1, 1] and m.stop == [T, T] and m.trials[0, 0] == 10 == m.trials[1, 0] and m.failed_solves == 20
                                     and _unchanged(m, pr) and m.n_inliers == m.nInitial == 65 and m.lam == 0.0 and m.chi2 == 0.0 and m.n_active == [65, 65]),
    "A.weight_negative": lambda m, pr: (m.status == 0 and m.iters == [10, 10] and m.stop == [ITS, ITS] and m.trials.max() == 7 and m.failed_solves >= 10
                                        and m.chi2 < 0 and 0 < m.n_active[1] < 65),
    "A.accepted_failure": lambda m, pr: m.status == 0 and m.accepted_failed == 1 and m.failed_solves >= 10 and m.iters == [10, 10] and 0 < m.n_inliers < 65,
    "A.far3": _far, "A.far10": _far,
    "A.far30": lambda m, pr: _far(m, pr) and m.stop[0] == NB,
    "A.absorb": lambda m, pr: m.status == 0 and m.iters[0] == 1 and m.trials[0, 0] == 1 and m.stop[0] == T and m.outlier[pr.edges()[7]] == 1 and m.iters[1] > 0,
    "B.huber_0": lambda m, pr: (m.status == 0 and m.iters == [1, 0] and m.stop == [T, NOT_RUN] and m.trials[0, 0] == 10 and m.failed_solves == 10 and m.n_inliers == 0
                                and m.outlier.sum() == 65 and _unchanged(m, pr) and m.lam == 0.0),
    "B.huber_1e-300": lambda m, pr: m.status == 0 and m.n_inliers == 0 and m.iters[0] > 1 and 0 < m.chi2 < 1e-290 and not _unchanged(m, pr),
    "B.huber_1e-3": lambda m, pr: m.status == 0 and m.n_inliers == 0 and m.iters[0] > 1,
    "B.huber_1e6": lambda m, pr: m.status == 0 and m.n_inliers == 65 and not m.outlier.any() and m.stop[0] == PM.STOP_GAIN,
    "B.huber_-1": lambda m, pr: m.status == 0 and m.n_inliers == 0 and m.failed_solves > 0 and m.trials.max() >= 5 and m.chi2 < 0,
    "B.huber_1e200": _nonfinite, "B.huber_inf": _nonfinite, "B.huber_nan": _nonfinite,
    "C.weight_inf": _nonfinite, "C.weight_1e308": _nonfinite, "C.weight_nan": _nonfinite,
    "C.weight_1e300": lambda m, pr: m.status == 0 and m.iters[1] > 0 and m.chi2 < 100 and m.outlier[pr.edges()[pr.octave[pr.edges()] == 3]].all(),
    "C.weight_1e-300": lambda m, pr: m.status == 0 and not m.outlier[pr.edges()[pr.octave[pr.edges()] == 3]].any() and m.n_inliers > 50,
    "C.levels_1": lambda m, pr: m.status == 0 and len(pr.inv_sigma2) == 1 and m.n_inliers > 50,
    "C.levels_max": lambda m, pr: m.status == 0 and len(pr.inv_sigma2) == H.MAX_LEVELS and pr.octave[pr.edges()].max() == H.MAX_LEVELS - 1 and m.n_inliers > 50,
    "D.axis_front": lambda m, pr: (m.status == 0 and np.array_equal(_special_at_start(pr), [[0.0, 0.0, 2.0]]) and m.lam > 1e12 and not _unchanged(m, pr)
                                   and m.outlier[pr.special[0]] == 0),
    "D.axis_behind": lambda m, pr: np.array_equal(_special_at_start(pr), [[0.0, 0.0, -2.0]]) and _ten_rejected_trials_twice(m, pr),
    "D.centre": lambda m, pr: np.array_equal(_special_at_start(pr), [[0.0, 0.0, 0.0]]) and _ten_rejected_trials_twice(m, pr),
    "D.grazing": lambda m, pr: (m.status == 0 and len(pr.special) == 5 and (np.abs(_special_at_start(pr)[:, 2]) <= 1e-12).all()
                                and len(set(np.sign(_special_at_start(pr)[:, 2]))) == 3 and m.n_inliers > 50),
    "D.stretched": lambda m, pr: (m.status == 0 and sorted(set(pr.cam[pr.edges()].tolist())) == list(range(7)) and m.n_inliers > 100
                                  and sorted(len(c["invP"]) for c in pr.cams)[::6] == [1, H.MAX_POLY]),
    "E.scale_1e-6": lambda m, pr: m.status == 0 and m.iters[1] > 0 and np.abs(pr.pos).max() < 1e-4,
    "E.scale_1e4": lambda m, pr: m.status == 0 and m.iters[1] > 0 and np.abs(pr.pos).max() > 1e4,
    "E.scale_1e8": lambda m, pr: m.status == 0 and m.n_inliers > 40 and np.abs(pr.pos).max() > 1e8 and np.abs(m.pose[3:]).max() > 1e6,
    "E.point_1e154": lambda m, pr: m.status == 0 and np.isfinite(m.pose).all() and math.isfinite(m.chi2) and m.outlier[pr.edges()[11]] == 1,
    "E.point_1e200": lambda m, pr: m.status == 0 and np.isfinite(m.pose).all() and math.isfinite(m.chi2) and m.outlier[pr.edges()[11]] == 1,
    "E.point_overflow": _nonfinite,
    "E.cayley50": lambda m, pr: m.status == 0 and m.iters[0] == 10 and m.n_inliers == 0 and m.n_active[1] == 0,
    "E.three_cameras": lambda m, pr: (m.status == 0 and len(set(pr.points[pr.special].tolist())) == 1 and sorted(pr.cam[pr.special].tolist()) == [0, 1, 2]
                                      and not m.outlier[pr.special].any()),
    "F.late_trial": lambda m, pr: (m.status == 0 and m.late_nonfinite[0] == 0 and m.late_nonfinite[1] >= 5 and math.isfinite(m.chi2) and math.isfinite(m.lam)
                                   and np.isfinite(m.pose).all() and m.trials[0].max() >= 4),
    "G.one_camera": lambda m, pr: m.status == 0 and len(pr.Mc_min) == 1 and m.n_inliers > 50,
    "G.cameras32": lambda m, pr: m.status == 0 and len(pr.Mc_min) == 32 and m.nInitial == 200 and m.n_inliers > 150,
    "G.cap_tail": lambda m, pr: m.status == 0 and pr.n == 65536 and m.nInitial == 65 and pr.edges().min() >= 65536 - 512 and m.n_inliers == 60,
    "G.cap_stride": lambda m, pr: m.status == 0 and pr.n == 65536 and m.nInitial == 65 and (pr.edges() % 512 == 0).all() and m.n_inliers == 60,
}


def test_the_table_and_its_excused_list():
    assert sorted(WANT) == sorted(H.SCENES)
    g = H.groups()
    assert sorted(g) == list("ABCDEFG")
    assert set(H.EXCUSED) <= set(H.SCENES) and set(H.NONFINITE) <= set(H.SCENES)
    assert 5 * len(H.EXCUSED) <= len(H.SCENES)                              # at most one scene in five
    for names in g.values():
        assert not set(names) <= set(H.EXCUSED), names                     # never every scene of a group
    for n in H.SCENES:
        assert len(H.build(n).edges()) <= 200


@pytest.mark.parametrize("name", sorted(H.SCENES))
def test_scene_shows_its_property(name):
    m, pr = H.model(name), H.build(name)
    assert m.nInitial == len(pr.edges())
    assert (m.status == PM.POSE_NONFINITE) == (name in H.NONFINITE)
    assert WANT[name](m, pr), (name, m.status, m.iters, m.stop, m.trials.tolist(), m.n_inliers, m.failed_solves, m.n_active, m.lam, m.chi2)


def test_group_floors():
    ms = [H.model(n) for n in H.SCENES]
    assert any(m.trials.max() >= 5 for m in ms)
    assert any(m.failed_solves > 0 for m in ms) and any(m.accepted_failed > 0 for m in ms)
    for why in (PM.STOP_TRIALS, PM.STOP_NBAD, PM.STOP_ITERATIONS):
        assert any(m.status == 0 and m.stop[0] == why for m in ms), why
    assert sum(m.iters[1] > 1 for m in ms) >= 3                             # round two iterating
    assert sum(m.status == 0 and m.n_active == [65, 0] for m in ms) >= 3    # round two skipped because the first pass flagged every edge
    assert any(m.trials[r, i] > 1 for m in ms for r in range(2) for i in range(10) if m.status == 0 and m.stop[r] != PM.STOP_TRIALS)


@pytest.mark.parametrize("name", sorted(H.SCENES))
def test_decisions_are_off_their_edges_and_the_spread_is_under_its_cap(name):
    m = H.model(name)
    assert not math.isnan(m.margin)
    if name in H.EXCUSED:
        assert m.margin < PM.MARGIN and m.flag_margin >= PM.MARGIN, (m.margin, m.flag_margin)      # excused, and its flags are still decided
    else:
        assert m.margin >= PM.MARGIN, m.margin            # else: re-seed the scene (tools/poseopt_seed_search.py --hostile) or excuse it, never loosen this
    assert 100.0 * H.spread(name) <= 1e-6, H.spread(name)


def test_the_build_pass_candidate_of_group_f_depends_on_the_summation_order():
    """why group F pins no run with a non-finite BUILD pass (hostile_poseopt's docstring): the one the search found gives another result with reversed sums"""
    pr = H.late(9, 0.02)
    a, b = PM.optimize(pr), PM.optimize(pr, reverse=True)
    assert a.status == b.status == 0 and a.late_nonfinite[0] > 0 and a.failed_solves != b.failed_solves
    assert np.abs(a.pose - b.pose).max() > 1e-3 and a.n_inliers != b.n_inliers


def test_absorption_is_exact():
    """the argument of the module docstring, on the numbers: every other edge's robust chi2 sums to less than half an ulp of the absorbing edge's"""
    pr = H.build("A.absorb")
    idx = pr.edges()
    e = PM.residual(pr, pr.pose0, idx)
    w = pr.inv_sigma2[pr.octave[idx]]
    c2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
    d = 1.345 * pr.huber
    r0 = np.where(c2 <= d * d, c2, 2 * np.sqrt(c2) * d - d * d)
    big = r0.max()
    assert big > 1e38 and np.sort(r0)[:-1].sum() < 0.25 * np.spacing(big)
    assert r0.sum() == r0[::-1].sum() == big


# ---------------------------------------------------------------------------------------------- the projections, pinned to something other than the model
GEOMETRY = ("D.axis_front", "D.axis_behind", "D.centre", "D.grazing", "D.stretched", "E.point_1e154", "E.point_1e200", "E.scale_1e8", "E.cayley50")


@pytest.mark.parametrize("name", GEOMETRY)
def test_hostile_projection_equals_the_oracle_bit_for_bit(oracle, name):
    pr, m = H.build(name), H.model(name)
    idx = pr.edges()
    for pose in (pr.pose0, m.pose):
        uv, _ = oracle.world_to_cam(PM.rig_from_min(pose, pr.Mc_min)[1], pr.cams, None, pr.pos[pr.points[idx]], pr.cam[idx])
        with np.errstate(over="ignore"):                    # x * x + y * y of the 1e154 and 1e200 points
            u, v = PM.project(pr, pose, idx)
        assert np.array_equal(u, uv[:, 0], equal_nan=True) and np.array_equal(v, uv[:, 1], equal_nan=True)
        assert np.isfinite(u).all() and np.isfinite(v).all()


@have_ref
@pytest.mark.parametrize("name", GEOMETRY)
def test_hostile_projection_equals_the_reference_code_bit_for_bit(name):
    import oracle_lib as O
    ref = C.CDLL(REF_SO)
    ref.ref_cayley2hom.argtypes = [C.c_void_p, C.c_void_p]
    ref.ref_world_to_cam.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(O.Ocam), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    pr, m = H.build(name), H.model(name)
    idx = pr.edges()
    nr, n = len(pr.Mc_min), len(idx)
    for pose in (pr.pose0, m.pose):
        hom = lambda c6: (lambda M: (ref.ref_cayley2hom(np.ascontiguousarray(c6, np.float64).ctypes.data, M.ctypes.data), M)[1])(np.zeros((4, 4)))
        M_t, M_c = hom(pose), np.stack([hom(q) for q in pr.Mc_min])
        uv, fl, inv = np.zeros((n, 2)), np.zeros(n, np.uint8), np.zeros((nr, 4, 4))
        oc = (O.Ocam * nr)(*[O.make_ocam(c) for c in pr.cams])
        pts, pc = np.ascontiguousarray(pr.pos[pr.points[idx]]), np.ascontiguousarray(pr.cam[idx])
        assert ref.ref_world_to_cam(M_t.ctypes.data, M_c.ctypes.data, oc, None, nr, pts.ctypes.data, pc.ctypes.data, n, uv.ctypes.data, fl.ctypes.data,
                                    inv.ctypes.data) == 0
        assert np.array_equal(inv, PM.rig_from_min(pose, pr.Mc_min)[1])
        with np.errstate(over="ignore"):
            e = PM.residual(pr, pose, idx)
        z = pr.xy[idx].astype(np.float64)
        assert np.array_equal(e[:, 0], z[:, 0] - uv[:, 0]) and np.array_equal(e[:, 1], z[:, 1] - uv[:, 1])


# ---------------------------------------------------------------------------------------------- the Jacobian
@pytest.mark.parametrize("name", ["D.stretched", "E.scale_1e-6", "E.scale_1e4", "E.scale_1e8", "G.cameras32"])
def test_jacobian_against_a_central_difference(name):
    """the bound construction of test_poseopt_cpu.test_jacobian_against_a_central_difference (truncation h^2/6 |e'''| from third differences plus rounding
    eps |e| / h, asserted with its 10x margin), with the steps of a translation component scaled by the world: h = 1e-6 * scale, g = 1e-3 * scale.  No
    point of these scenes is on the constant branch."""
    pr = H.build(name)
    scale = H.SCENES[name][1].get("factor", 1.0)
    idx = pr.edges()
    pose = pr.pose0
    J = PM.jacobian(pr, pose, idx)
    assert np.isfinite(J).all()
    for k in range(6):
        s = scale if k >= 3 else 1.0
        h, g = 1e-6 * s, 1e-3 * s
        d = np.zeros(6)
        d[k] = 1.0
        num = (PM.residual(pr, pose + h * d, idx) - PM.residual(pr, pose - h * d, idx)) / (2 * h)
        third = (PM.residual(pr, pose + 2 * g * d, idx) - 2 * PM.residual(pr, pose + g * d, idx) + 2 * PM.residual(pr, pose - g * d, idx)
                 - PM.residual(pr, pose - 2 * g * d, idx)) / (2 * g ** 3)
        est = h * h / 6 * np.abs(third).max() + 2.2e-16 * 1e3 / h
        assert np.abs(J[:, :, k] - num).max() <= 10 * est, (name, k, np.abs(J[:, :, k] - num).max(), est)
    assert np.abs(J[:, :, :3]).max() > 100.0


def test_jacobian_on_the_constant_branch():
    """norm == 0 -> 1e-14 is a constant: with n = 1e-14, q = -z / n, D is exactly d(uu, vv)/d(x, y) = rho / n on the diagonal (the x / norm, y / norm factors)
    through the affine part, and d/dz = 0 because x / n == y / n == 0; finite for a point in front, behind and at the centre"""
    cams, _ = S.rig(1)
    cam = cams[0]
    for z in (2.0, -2.0, 0.0):
        D = PM.d_world_to_img(cam, np.array([0.0]), np.array([0.0]), np.array([z]))[0]
        rho = PM._horner(cam["invP"], PM._atan(np.array([-z / 1e-14])))[0]
        a = (1.0 / 1e-14) * rho                          # d uu / dx = d vv / dy; the cross terms and d/dz vanish
        want = np.array([[a * cam["c"], a * cam["d"], 0.0], [a * cam["e"], a, 0.0]])
        assert np.isfinite(D).all() and np.array_equal(D, want), (z, D, want)
        assert abs(a) > 1e10                                # rho / 1e-14: what makes lambda of the axis scenes so large


# ---------------------------------------------------------------------------------------------- the two findings
def test_margin_metric_is_never_nan():
    """an infinite threshold is infinitely far from a finite chi2; against a threshold of 0 the distance is the chi2 itself"""
    c2 = np.array([0.5, 3.0, 7.0])
    assert PM.threshold_margin(c2, math.inf) == math.inf and PM.threshold_margin(c2, 1.809025e400) == math.inf
    assert PM.threshold_margin(np.array([1.0, math.inf]), math.inf) == 0.0
    assert PM.threshold_margin(c2, 0.0) == 0.5
    assert PM.threshold_margin(c2, 2.0) == 0.5 == float(np.min(np.abs(c2 - 2.0) / 2.0))        # unchanged where the threshold is finite and positive
    for name in H.groups()["B"] + H.groups()["C"]:
        m = H.model(name)
        assert not math.isnan(m.margin) and not math.isnan(m.flag_margin), name
    assert H.model("B.huber_0").margin > 0.0


@pytest.mark.parametrize("what", ["weight", "huber", "weight_inf", "huber_inf", "huber_1e200", "weight_1e308", "unused_level"])
def test_nonfinite_weight_or_multiplier_is_not_optimised(what):
    """the first evaluation's screen covers every edge's weight, the Huber pair and the reduced sums.  Before, a NaN weight or multiplier ran both
    rounds to status 0 with lambda = chi2 = NaN (and twenty flags set at the start pose)."""
    pr = H.base(1)
    pr.inv_sigma2 = pr.inv_sigma2.copy()
    if what.startswith("weight"):
        pr.inv_sigma2[3] = {"weight": np.nan, "weight_inf": np.inf, "weight_1e308": 1e308}[what]
    elif what == "unused_level":
        pr.octave[pr.octave == 7] = 6
        pr.inv_sigma2[7] = np.nan                      # no edge reads it: not screened, and the result is the control's with that level moved
    else:
        pr.huber = {"huber": np.nan, "huber_inf": np.inf, "huber_1e200": 1e200}[what]
    m = PM.optimize(pr)
    if what == "unused_level":
        assert m.status == PM.POSE_OK and math.isfinite(m.lam) and m.n_inliers > 50
        return
    assert m.status == PM.POSE_NONFINITE and m.pose.tobytes() == pr.pose0.tobytes() and not m.outlier.any() and m.n_inliers == 65 and m.share == 0.0
    assert m.iters == [0, 0] and m.lam == 0.0 and m.chi2 == 0.0
    assert np.array_equal(m.MtMc_inv, PM.rig_from_min(pr.pose0, pr.Mc_min)[1])


def test_one_level_table_of_hostile_weights():
    """the six distinct problems of hostile_poseopt.weight_interleaved: decisions off their edges, the controls untouched by the hostile levels they avoid,
    the negative level failing solves, the 1e300 level flagged, the 1e-300 level never flagged"""
    seen = {}
    for kind, p in H.weight_interleaved(12):
        if kind not in seen:
            seen[kind] = (p, PM.optimize(p))
    assert sorted(seen) == ["control1", "control2", "control3", "level3_1", "level5_2", "level6_3"]
    for kind, (p, m) in seen.items():
        assert m.status == 0 and m.margin >= PM.MARGIN, (kind, m.margin)
        assert np.array_equal(p.inv_sigma2[list(H.HOSTILE_LEVELS)], list(H.HOSTILE_LEVELS.values()))
        e = p.edges()
        if kind.startswith("control"):
            assert m.n_inliers >= 60 and m.failed_solves == 0 and not np.isin(p.octave[e], list(H.HOSTILE_LEVELS)).any()
    assert seen["level3_1"][1].failed_solves >= 10 and seen["level3_1"][1].trials.max() >= 5
    for kind, lv, flagged in (("level5_2", 5, False), ("level6_3", 6, True)):
        p, m = seen[kind]
        on = m.outlier[p.edges()][p.octave[p.edges()] == lv]
        assert len(on) >= 5 and on.all() == flagged and on.any() == flagged


def test_interleaved_calls_share_one_rig():
    """what lets one call hold them: every member of an interleaved call is built on the control's rig, cameras and level weights"""
    c = H.base(1)
    for n in H.BATCH_SIZES:
        prs = H.interleaved(n)
        assert len(prs) == n and sum(name is None for name, _ in prs) == (n + 1) // 2
        for name, p in prs:
            assert np.array_equal(p.Mc_min, c.Mc_min) and np.array_equal(p.inv_sigma2, c.inv_sigma2) and p.cams == c.cams, name
    assert set(H.INTERLEAVED) <= set(H.SCENES) and {n[0] for n in H.INTERLEAVED} == set("ABE")
    assert [n for n, _ in H.huber_batch()][1:-1] == ["B.huber_" + k for k in H.HUBERS]
