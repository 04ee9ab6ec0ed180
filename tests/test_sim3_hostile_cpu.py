"""CPU checks of the hostile Sim3 suite (tests/hostile_sim3.py): the model states every scene of the table (IEEE divisions, C++ NaN comparisons, no
exception), is unchanged on finite inputs, and every group reaches what it is there for — the floors below hold on the model alone, so a scene cannot pass
tests/test_gpu_hostile_sim3.py vacuously.  The refusals of mcs_sim3_create are checked in the GPU file: the library tests its context argument first."""
import os

import numpy as np
import pytest

import hostile_sim3 as T
import sim3_model as M

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_model_hypotheses_seed2101.npy")


def evaluated(sc, s=0, count=None):
    """[(picks, hypothesis, inliers, near)] of solver s's first `count` iterations (all it is allowed by default), computed once"""
    def make():
        m = T.models_of(sc)[s]
        n = m.mRansacMaxIts if count is None else count
        return m, [m.evaluate(k, T.draws_of(sc, s)) for k in range(n)]
    return T._once(("evaluated", id(sc), s, count), make)


def near_of(ev):
    return sum(int(e[3].sum()) for e in ev)


# ---- the model itself ----------------------------------------------------------------------------------------------------------------------------------
def test_model_is_bit_identical_on_finite_inputs():
    """the 45 doubles of 20 hypotheses of one make_pair scene, recorded before the model's divisions were made IEEE"""
    import gpu_common
    cams, M_c = gpu_common.cams3(), M.rig_poses(3)
    m = M.model_of(M.make_pair(np.random.default_rng(2101), M_c, 40, inlier_frac=0.7), cams, M_c)
    dr = M.generated_draws(2101, 0, 40)
    got = np.stack([M.hyp_vector(m.hypothesis(k, dr)[1]) for k in range(20)])
    want = np.load(GOLDEN)
    assert want.shape == (20, 45) and np.isfinite(want).all()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_model_divides_and_compares_as_ieee():
    nan, inf = float("nan"), float("inf")
    assert np.isnan(M._div(0.0, 0.0)) and M._div(1.0, 0.0) == inf and M._div(-1.0, 0.0) == -inf and np.isnan(M._div(inf, inf))
    assert np.isnan(M.cv_hypot(nan, 1.0))       # `a > b` false, `b > 0` true: b * sqrt(1 + NaN)
    assert M.cv_hypot(1.0, nan) == 0.0          # both comparisons false: OpenCV's hypot returns 0
    assert M.cv_hypot(inf, inf) != M.cv_hypot(inf, inf)   # inf / inf
    # a NaN pivot: `fabs(p) <= eps` is false, the rotation is made with NaN factors; `mv < val` is false with a NaN on either side, so the search keeps its
    # first candidate.  The loop ends at a pivot that is an exact 0 (a rotation zeroes its own pivot) or at the n * n * 30 cap
    info = {}
    A = [[1.0, nan, 0.0, 0.0], [nan, 2.0, 0.0, 0.0], [0.0, 0.0, 3.0, 0.5], [0.0, 0.0, 0.5, 4.0]]
    W, V = M.jacobi_eigen(A, info)
    assert 1 <= info["rotations"] <= 480 and np.isnan(W).any()
    # a zero matrix and an exact diagonal: no rotation, the identity eigenvectors
    for A in ([[0.0] * 4 for _ in range(4)], np.diag([1.0, 4.0, 2.0, 3.0]).tolist()):
        W, V = M.jacobi_eigen(A, info)
        assert info["rotations"] == 0 and W == sorted(W, reverse=True) and sorted(map(tuple, V)) == sorted(map(tuple, np.eye(4).tolist()))
    for bad in ([[nan] * 3] * 3, [[inf, 0, 0], [0, 1, 0], [0, 0, 1]], [[1e200, 0, 0], [0, 1e200, 0], [0, 0, 1e200]], [[0.0] * 3] * 3):
        h = M.compute_t(bad, np.eye(3).tolist())    # no exception; 1e200: the products overflow
        assert not np.isfinite(M.hyp_vector(h)).all()
    assert np.isnan(M.rodrigues([inf, 0.0, 0.0])).any()       # cos / sin of an infinity


def test_thresholds_refuse_what_the_library_refuses():
    for v in T.REFUSED_SIGMA2:
        with pytest.raises(ValueError):
            M.max_error(v)
    assert M.max_error(T.LARGEST_SIGMA2) < 2.0 ** 64 and M.max_error(0.0) == 0.0 and M.max_error(-0.0) == 0.0
    sc = T.sigma_scene()
    for v in (float("nan"), -1.0):
        pair = dict(sc["pairs"][0], sigma2=sc["pairs"][0]["sigma2"].copy())
        pair["sigma2"][5, 1] = v
        with pytest.raises(ValueError):
            M.model_of(pair, sc["cams"], sc["M_c"])


def test_angle_perturbation_is_a_last_place_change():
    """compute_t(ang_ulps=1) is the model's own sensitivity to the libm behind atan2: on a well-conditioned triple one ulp of the angle moves R by ~1e-16"""
    P2 = [[1.0, -1.0, 0.0], [0.0, 1.0, -1.0], [2.0, 3.0, 5.0]]
    P1 = [[0.3, 1.0, -2.0], [1.0, 0.5, 4.0], [2.0, -3.0, 1.0]]
    a, b = M.compute_t(P1, P2), M.compute_t(P1, P2, ang_ulps=1)
    d = np.abs(M.hyp_vector(a) - M.hyp_vector(b)).max()
    assert 0 < d < 1e-14


# ---- A -------------------------------------------------------------------------------------------------------------------------------------------------
def test_exact_triples_reach_their_degeneracies():
    sc = T.exact_scene()
    m, ev = evaluated(sc)
    assert m.N == 3 * T.EXACT_CASES + T.EXACT_FILL == 65 and len(ev) == T.EXACT_ITERATIONS
    assert np.array_equal(m.X1c, sc["pairs"][0]["Xw"][:, 0]) and np.array_equal(m.X2c, sc["pairs"][0]["Xw"][:, 1])   # the lattice survives the rig transform
    by = {name: ev[k] for k, (name, _, _) in enumerate(T.EXACT_TRIPLES)}
    for k, (name, _, _) in enumerate(T.EXACT_TRIPLES):
        assert ev[k][0] == [3 * k, 3 * k + 1, 3 * k + 2], name
    nan_cases = ("identity", "scale_2", "scale_half", "collinear_self", "all_coincident", "pr2_zero", "pr1_zero")
    for name, (_, h, inl, _) in by.items():
        v = M.hyp_vector(h)
        if name in nan_cases:
            assert np.isnan(h["R"]).all() and np.isnan(h["s"]) and inl.sum() == 0, name
        else:
            assert np.isfinite(v).all(), name
    # the identity: the quaternion is exactly (1, 0, 0, 0) although the solver rotated (in the lower block): nv = 0, (2 ang) (1 / nv) = 0 * inf
    assert by["identity"][1]["V"][0].tolist() == [1.0, 0.0, 0.0, 0.0] and by["identity"][1]["rotations"] > 0
    assert by["collinear_self"][1]["rotations"] == 0 and by["all_coincident"][1]["rotations"] == 0
    assert by["half_turn"][1]["V"][0][0] == 0.0                                            # w an exact zero: atan2(nv, 0)
    assert np.allclose(by["half_turn"][1]["R"], np.diag([-1.0, -1.0, 1.0]), atol=1e-15)
    assert np.allclose(by["quarter_turn"][1]["R"], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15) and by["quarter_turn"][2].sum() > 15
    W = by["collinear_quarter"][1]["W"]
    assert W[0] == W[1] and W[0] > 0                                                       # a double top eigenvalue, bit for bit
    for name in ("collinear_tie_a", "collinear_tie_b"):
        W = by[name][1]["W"]
        assert W[0] == W[1] and W[0] > 0 and by[name][1]["rotations"] > 0
    h = by["coincident_pair_one_side"][1]
    assert abs(h["W"][0] - h["W"][1]) <= 4e-16 * h["W"][0] and h["rotations"] > 0 and (h["N"] != np.round(h["N"] * 3) / 3).any()   # double, from rounded products
    assert np.allclose(by["reflection"][1]["R"] @ by["reflection"][1]["R"].T, np.eye(3), atol=1e-12)   # a rotation is returned for a reflection
    assert near_of(ev) == 0


# ---- B -------------------------------------------------------------------------------------------------------------------------------------------------
def test_world_scale_reaches_the_absolute_stopping_rule():
    stats = {}
    for f in T.SCALE_FACTORS:
        m, ev = evaluated(T.scale_scene(f))
        assert len(ev) == T.SCALE_ITERATIONS and near_of(ev) == 0
        stats[f] = ([e[1]["rotations"] for e in ev], [T.jacobi_residual(e[1]) for e in ev], [int(e[2].sum()) for e in ev])
    print({f: (min(s[0]), max(s[0]), "%.2e" % max(s[1])) for f, s in stats.items()})
    assert max(stats[1.0][1]) < 1e-12                                                       # converged at metre scale
    assert any(max(s[0]) == 0 for s in stats.values())                                      # some factor stops the solver before its first rotation
    assert any(min(s[0]) > 0 and max(s[1]) > 1e-6 for s in stats.values())                  # some factor stops it half-way: W, V do not diagonalise N
    assert stats[1e-9][2] != stats[1.0][2] and stats[1e4][2] == stats[1.0][2] == stats[1e8][2]   # the unconverged hypotheses decide differently
    assert max(stats[1.0][2]) >= 20
    p1, p4 = T.scale_scene(1.0)["pairs"][0], T.scale_scene(1e4)["pairs"][0]
    assert np.allclose(p4["Xw"], 1e4 * p1["Xw"], rtol=1e-15) and np.allclose(p4["M_t_inv"].reshape(2, 4, 4)[:, :3, 3], 1e4 * p1["M_t_inv"].reshape(2, 4, 4)[:, :3, 3])
    assert np.allclose(np.stack(T.scale_scene(1e4)["M_c"])[:, :3, 3], 1e4 * np.stack(M.rig_poses(3))[:, :3, 3])
    plain = M.make_pair(np.random.default_rng(2202), M.rig_poses(3), 40, inlier_frac=0.7)
    assert all(np.array_equal(plain[k], p1[k]) for k in ("Xw", "cam", "sigma2", "index1", "M_t_inv", "MtMc_inv"))   # factor 1 is make_pair itself


# ---- C -------------------------------------------------------------------------------------------------------------------------------------------------
def test_poisoned_points_are_stated_and_never_inliers():
    sc = T.poison_scene()
    m, ev = evaluated(sc)
    assert m.N == 65 and len(ev) == T.POISON_ITERATIONS
    X = sc["pairs"][0]["Xw"]
    assert np.isnan(X[T.POISONED[0], 0]).sum() == 1 and np.isinf(X[T.POISONED[1], 1]).sum() == 1 and (X[T.POISONED[2], 0] == 1e200).all()
    poisoned = [any(p in T.POISONED for p in e[0]) for e in ev]
    assert sum(poisoned) >= 10 and len(ev) - sum(poisoned) >= 200
    assert not any(e[2][list(T.POISONED)].any() for e in ev)
    assert sum(1 for e, p in zip(ev, poisoned) if p and np.isnan(M.hyp_vector(e[1])).any()) >= 5      # NaN hypotheses ...
    assert sum(1 for e, p in zip(ev, poisoned) if p and np.isfinite(M.hyp_vector(e[1])).all() and abs(e[1]["s"]) > 1e150) >= 1   # the 1e200 pair: finite, huge
    assert all(np.isfinite(M.hyp_vector(e[1])).all() for e, p in zip(ev, poisoned) if not p)
    assert max(int(e[2].sum()) for e in ev) >= 30


# ---- D -------------------------------------------------------------------------------------------------------------------------------------------------
def test_threshold_pairs_sit_where_the_table_says():
    sc = T.threshold_scene()
    m, ev = evaluated(sc)
    _, h, inl, near = ev[0]
    err = m.errors(h)
    e = (m.e1, m.e2)
    inside = [(i, side) for i, side, _, rel in T.THRESHOLD_TARGETS if rel == 0.0]
    outside = [(i, side, rel) for i, side, _, rel in T.THRESHOLD_TARGETS if rel != 0.0]
    assert len(inside) >= 8 and len(outside) >= 8
    assert {side for _, side in inside} == {1, 2} and {side for _, side, _ in outside} == {1, 2}
    assert len({lv for _, _, lv, _ in T.THRESHOLD_TARGETS[:8]}) >= 3 and len({lv for _, _, lv, _ in T.THRESHOLD_TARGETS[8:]}) >= 3
    for i, side in inside:
        assert abs(err[side - 1][i] - e[side - 1][i]) <= T.IN_BAND * e[side - 1][i] and near[i], i
        assert err[2 - side][i] < 0.75 * e[2 - side][i]            # the other side does not decide
    for i, side, rel in outside:
        d = (err[side - 1][i] - e[side - 1][i]) / e[side - 1][i]
        assert abs(d - rel) <= 1e-3 * T.OUT_BAND and not near[i], (i, d)
        assert inl[i] == (rel < 0) and err[2 - side][i] < 0.75 * e[2 - side][i]
    assert near.sum() == len(inside)
    assert all(np.array_equal(x[2], inl) for x in ev)             # the same hypothesis in every iteration


# ---- E -------------------------------------------------------------------------------------------------------------------------------------------------
def test_projection_rigs_cover_the_stretched_cameras():
    rigs = T.projection_rigs()
    used = {n for name in rigs for n in name.split("+")}
    assert set(T.HC.STRETCHED) <= used
    degs = {len(c["invP"]) for cams in rigs.values() for c in cams}
    assert 16 in degs and 1 in degs and 6 in degs


@pytest.mark.parametrize("name", list(T.projection_rigs()))
def test_projection_regimes_are_reached(name):
    sc = T.projection_scene(name)
    m, ev = evaluated(sc)
    assert len(ev) == T.PROJ_ITERATIONS and near_of(ev) == 0
    assert (m.cam1[18:] != m.cam2[18:]).all() and len(set(m.cam1)) == 3
    reached = {r: max(int(T.regimes(m, e[1])[r].sum()) for e in ev if np.isfinite(M.hyp_vector(e[1])).all()) for r in T.REGIMES}
    assert all(v >= 4 for v in reached.values()), reached
    first = T.regimes(m, ev[0][1])
    assert first["on_axis"][3:8].all() and first["behind"][8:13].all() and first["grazing"][13:18].all()
    best = max(int(e[2].sum()) for e in ev)
    assert best >= 0.3 * m.N
    # the projection decides: under the best hypothesis some noisy lattice pairs are inliers and some are not
    k = int(np.argmax([int(e[2].sum()) for e in ev]))
    fill = ev[k][2][18:18 + T.PROJ_FILL]
    assert 0 < fill.sum() < T.PROJ_FILL


# ---- F -------------------------------------------------------------------------------------------------------------------------------------------------
def test_sigma_edges_truncate_to_zero_and_one():
    assert 9.210 * T.SIGMA_DOWN < 1.0 <= 9.210 * T.SIGMA_UP and np.nextafter(T.SIGMA_DOWN, 1.0) == T.SIGMA_UP
    assert [M.max_error(v) for v in T.SIGMA_EDGES] == [0.0, 0.0, 1.0, 9.21e15, 9.0, 118.0]
    sc = T.sigma_scene()
    m, ev = evaluated(sc)
    assert near_of(ev) == 0
    assert set(m.e1) == set(m.e2) == {0.0, 1.0, 9.0, 118.0, 9.21e15} and (m.e1 != m.e2).any()
    zero = (m.e1 == 0) | (m.e2 == 0)
    assert zero.sum() >= 10 and not any(e[2][zero].any() for e in ev)          # a threshold of 0 never holds an inlier ...
    _, h, inl, _ = ev[0]
    e1, e2 = m.errors(h)
    exact = (e1 == 0) & (e2 == 0)
    assert (exact & zero).sum() >= 2 and not inl[exact & zero].any()            # ... also for a correspondence without any error
    one = exact & ~zero & ((m.e1 == 1) | (m.e2 == 1))
    assert one.any() and inl[one].all()                                         # 0 < 1
    assert max(int(e[2].sum()) for e in ev) > 15


# ---- G -------------------------------------------------------------------------------------------------------------------------------------------------
def test_batch_shapes():
    sc = T.word_scene()
    assert [len(p["index1"]) for p in sc["pairs"]] == [3, 63, 64, 65, 127, 128, 129]
    for s in range(len(sc["pairs"])):
        m, ev = evaluated(sc, s)
        assert near_of(ev) == 0 and len(ev) == (1 if m.N == 3 else 40)
    assert sum(1 for s in range(7) if max(int(e[2].sum()) for e in evaluated(sc, s)[1]) > 3) >= 4
    many = T.many_scene()
    ms = T.models_of(many)
    assert len(ms) == T.MANY == 130 and max(m.N for m in ms) <= 20 and ms[T.MANY_EMPTY].N == 0 and 0 < ms[T.MANY_SHORT].N < 6
    assert all(m.mRansacMaxIts <= 12 for m in ms)
    totals, after, near = T.slot_totals(many, T.MANY_CALLS)
    assert near == 0 and any(t % 4 for t in totals) and any(t > 256 for t in totals), totals
    assert sum(1 for m in after if m.mnBestInliers > 6) >= 20 and after[T.MANY_EMPTY].best is None and after[T.MANY_SHORT].best is None
    one, wide = T.one_camera_scene(), T.many_camera_scene()
    assert len(one["cams"]) == 1 and len(wide["cams"]) == 32 and len(wide["M_c"]) == 32
    assert set(np.unique(wide["pairs"][0]["cam"])) == {0, 15, 31}
    for sc in (one, wide):
        m, ev = evaluated(sc)
        assert near_of(ev) == 0 and max(int(e[2].sum()) for e in ev) >= 15


# ---- H -------------------------------------------------------------------------------------------------------------------------------------------------
def test_state_scripts_on_the_model():
    # caller draws: the NaN identity hypothesis is the best one after the first iteration (0 >= 0)
    models, near, _ = T.drive_state(T.exact_scene(), T.STATE_SCRIPT_DRAWS[:1])
    assert near == 0 and models[0].mnBestInliers == 0 and np.isnan(models[0].best["R"]).all()
    models, near, refusals = T.drive_state(T.exact_scene(), T.STATE_SCRIPT_DRAWS)
    assert near == 0 and refusals == 2 and models[0].mnBestInliers > 15
    trace = []
    m = T.models_of(T.exact_scene())[0]
    dr = T.draws_of(T.exact_scene(), 0)
    for what, arg in T.STATE_SCRIPT_DRAWS:
        if what == "iterate":
            trace.append(m.iterate(arg, dr)[:2] + (m.mnIterations, m.mnBestInliers))
        elif what == "params":
            m.SetRansacParameters(*arg)
            trace.append(("params", m.mRansacMaxIts))
    print(trace)
    assert (True, False) in [t[:2] for t in trace] and (False, True) in [t[:2] for t in trace]
    # after the higher minInliers the kept mnBestInliers blocks every update: the iterations run out without a success
    k = next(i for i, t in enumerate(trace) if t[0] == "params")
    assert trace[k + 1][:2] == (False, False) and trace[k + 2][:2] == (False, True) and trace[k + 2][3] == trace[k - 1][3]
    assert ("params", 0) in trace                                                # minInliers > N
    models, near, refusals = T.drive_state(T.state_scene(), T.STATE_SCRIPT_SEED)
    assert near == 0 and refusals == 0 and [m.N for m in models] == [24, 40, 70] and max(m.mnBestInliers for m in models) > 15
