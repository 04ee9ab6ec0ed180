"""CPU: tests/essgraph_model.py itself, the restatement of cOptimizer::OptimizeEssentialGraph the device is held to, and the scenes' conditions.

The numeric Jacobian against the derivative; zero residuals and no step where nothing was corrected; a loop with an injected drift is distributed and the
corrected chain closes; one test per quirk that fails when the model "repairs" it (parallel edges summed, the terminate action's cap at iteration 15, a
kind-1 edge mixing Snc on one side with Scw on the other, points of reference -1 untouched); the blocked solve against numpy's; every scene keeps its margins
and its spread (what tests/test_gpu_essgraph.py derives its tolerance from)."""
import numpy as np
import pytest

import essgraph_model as M
import essgraph_scenes as S


def test_numeric_jacobian_equals_the_derivative_within_what_a_1e_9_step_allows():
    """The derivative is taken by central differences with h = 1e-6 and one Richardson step (truncation of the order h^4, rounding 1e-16 / 1e-6 = 1e-10 per
    unit of the residual's terms).  The step stays below 1e-5: log() changes its formulas where |sigma| or 1 - d crosses 1e-5, and with them — sim3.h:199 —
    its value, so a residual whose sigma is exactly 0 (an edge between two keyframes of scale 1) has no derivative across a step that wide.
    g2o's own step of 1e-9 divides the rounding of a residual (2^-53 per unit of the largest term that enters it, the translations) by 2e-9: 5.5e-8 per
    unit for ONE rounding; a residual is a chain of some tens of them.  Bound: 100 roundings, 5.5e-6 per unit of max(1, |t|).  Measured: 2.3e-6 at |t| <= 3.9."""
    pr = S.build("scale")
    idx, ei, ej, meas = M.measurements(pr)
    est = M.sim3_of(pr.Scw)
    _, A, B = M.jacobians(est, ei, ej, meas)

    def res(du_i, du_j):
        Si = M.sim3_mul(M.sim3_exp(du_i), tuple(c[ei] for c in est))
        Sj = M.sim3_mul(M.sim3_exp(du_j), tuple(c[ej] for c in est))
        return M.edge_error(meas, Si, M.sim3_inverse(Sj))

    def derivative(side):
        cols = []
        for d in range(7):
            def cd(h):
                u = np.zeros((len(ei), 7))
                u[:, d] = h
                z = np.zeros_like(u)
                return (res(u, z) - res(-u, z)) / (2 * h) if side == 0 else (res(z, u) - res(z, -u)) / (2 * h)
            cols.append((4 * cd(0.5e-6) - cd(1e-6)) / 3)
        return np.stack(cols, -1)

    scale = max(1.0, float(np.abs(pr.Scw[:, 4:7]).max()))
    worst = max(float(np.abs(A - derivative(0)).max()), float(np.abs(B - derivative(1)).max()))
    print("numeric Jacobian against the derivative: %.3g (|t| up to %.3g, bound %.3g)" % (worst, scale, 5.5e-6 * scale))
    assert worst <= 5.5e-6 * scale
    assert np.abs(A).max() > 0.5 and np.abs(B).max() > 0.5


def test_numeric_jacobian_equals_the_closed_form_where_there_is_one():
    """An independent reference, not made of the model's residual: for an edge whose measurement is the identity between two vertices at the SAME Sim3 S,
    e(d_i) = log(Sim3(d_i) S S^-1) = d_i and e(d_j) = log(S (Sim3(d_j) S)^-1) = log(Sim3(-d_j)) = -d_j, so A = I and B = -I whatever S is (scale 1: with
    another scale the small-angle branch of log is not the inverse of exp, sim3.h:199).  Bound as above: 100 roundings of 5.5e-8 per unit of max(1, |t|).
    The general case has no closed form short of deriving g2o's analytic edge, which the reference does not use; there the test above stands on central
    differences of the residual with a step a thousand times wider, which share the residual's own formulas: what they cannot see is an error in log() or
    the products themselves, and those are held to recorded g2o results (tests/test_sim3g_cpu.py) and to log(exp(v)) = v (tests/test_sim3g_log_cpu.py)."""
    rng = np.random.default_rng(7)
    n = 40
    q = rng.normal(0, 1, (n, 4))
    S = np.concatenate([q / np.linalg.norm(q, axis=1)[:, None], rng.normal(0, 3, (n, 3)), np.ones((n, 1))], 1)
    S[0] = [0, 0, 0, 1, 0, 0, 0, 1]
    est = M.sim3_of(np.concatenate([S, S]))
    ei, ej = np.arange(n), np.arange(n, 2 * n)
    meas = M.sim3_of(np.tile([0, 0, 0, 1, 0, 0, 0, 1.0], (n, 1)))
    r, A, B = M.jacobians(est, ei, ej, meas)
    scale = np.maximum(1.0, np.abs(S[:, 4:7]).max(1))[:, None, None]
    print("closed form: |A - I| %.3g, |B + I| %.3g per unit of max(1, |t|)" % (np.abs((A - np.eye(7)) / scale).max(), np.abs((B + np.eye(7)) / scale).max()))
    assert np.abs(r[:, 0]).max() <= 1e-14
    assert (np.abs(A - np.eye(7)) <= 5.5e-6 * scale).all() and (np.abs(B + np.eye(7)) <= 5.5e-6 * scale).all()
    assert np.array_equal(A[0], np.eye(7)) or np.abs(A[0] - np.eye(7)).max() <= 5.5e-8        # at the identity itself: one rounding at most


def test_nothing_corrected_nothing_moves():
    m = S.model("identity")
    pr = S.build("identity")
    assert m.status == M.EG_OK and m.chi2 == 0.0 and (m.iters, m.stop, m.trials[:2]) == (1, M.STOP_TRIALS, [1, 0])
    assert np.array_equal(m.Scw_out, pr.Scw) and np.array_equal(m.kf_t, -pr.Scw[:, 4:7])
    assert np.abs(m.pos - pr.pos).max() <= 1e-14          # (X + t) - t: two roundings at |X + t| <= 16
    # the same on a drifting trajectory whose products are not exact: residuals of rounding size, whatever Levenberg-Marquardt makes of them
    pr = S.make(3, 10, {}, [(9, 0)], [0])
    r = M.residuals(M.sim3_of(pr.Scw), *M.measurements(pr)[1:])
    assert np.abs(r).max() <= 1e-13
    m = M.optimize(pr)
    assert m.status == M.EG_OK and m.chi2 <= 1e-24 and np.abs(m.Scw_out - pr.Scw).max() <= 1e-10 and np.abs(m.pos - pr.pos).max() <= 1e-9


def test_an_injected_drift_is_distributed_and_the_chain_closes():
    """12 keyframes on a closed circle; the estimate drifts; the loop correction D moves the last two keyframes.  Before the optimisation the whole
    discrepancy sits on the edges between corrected and uncorrected keyframes; behind it the largest edge residual is a fraction of that and chi2 has
    fallen: one residual r spread evenly over n edges leaves chi2 = r^2 / n.  Asserted: the largest residual at most half, chi2 at most a third
    (the model: 0.66 -> 0.018 and 0.56 -> 0.0033)."""
    pr = S.make(5, 12, S._tail(12, 2, 0.02, 0.3, 1.03), [(11, 0)], [0], covis=1)
    idx, ei, ej, meas = M.measurements(pr)
    r0 = M.residuals(M.sim3_of(pr.Scw), ei, ej, meas)
    m = M.optimize(pr)
    r1 = M.residuals(M.sim3_of(m.Scw_out), ei, ej, meas)
    n0, n1 = np.linalg.norm(r0, axis=1), np.linalg.norm(r1, axis=1)
    print("residual norms before", np.round(n0, 4), "after", np.round(n1, 4), "chi2 %.4g -> %.4g" % ((n0 ** 2).sum(), m.chi2))
    assert m.status == M.EG_OK and (n0 > 1e-3).sum() == 2 and n0[0] <= 1e-12      # the loop edge is satisfied by construction; the tree edges of the two corrected keyframes carry it all
    assert n1.max() <= 0.5 * n0.max() and m.chi2 <= (n0 ** 2).sum() / 3 and (n1 > 1e-3).sum() >= 4
    assert abs(m.chi2 - (n1 ** 2).sum()) <= 1e-9 * m.chi2
    assert np.array_equal(m.Scw_out[0], pr.Scw[0])                                   # the fixed vertex
    moved = np.abs(m.Scw_out - pr.Scw).max(1)
    assert (moved[1:] > 1e-4).all()                                                  # every free vertex took its share


def test_quirk_parallel_edges_are_summed():
    pr = S.build("dup")
    a, b = S.model("dup"), M.optimize(pr, fix=["dedup"])
    assert a.n_edges == b.n_edges + 1 and S.rel(a.Scw_out, b.Scw_out) > 1e-4
    # two edges of one pair weigh as one edge with twice the information: H and b of the pair double
    idx, ei, ej, meas = M.measurements(pr)
    r, A, B = M.jacobians(M.sim3_of(pr.Scw), ei, ej, meas)
    fidx = np.cumsum(pr.fixed == 0) - 1
    fidx[pr.fixed != 0] = -1
    keep = [k for k in range(len(ei)) if not (ei[k] == 5 and ej[k] == 0 and pr.edge_kind[idx[k]] == 1)]
    H2, b2 = M.build_system(A, B, r[:, 0], ei, ej, fidx, 5, False)
    H1, b1 = M.build_system(A[keep], B[keep], r[keep, 0], ei[keep], ej[keep], fidx, 5, False)
    assert np.abs(H2 - H1)[28:, 28:].max() > 0.5 and np.array_equal((H2 - H1)[:28, :28], np.zeros((28, 28)))


def test_quirk_the_cap_fires_at_iteration_15():
    a = S.model("isolated")
    assert (a.iters, a.stop) == (16, M.STOP_CAP) and all(t >= 1 for t in a.trials[:16]) and a.trials[16:] == [0] * 4
    b = M.optimize(S.build("isolated"), fix=["cap"])
    assert b.iters > 16 or b.stop != M.STOP_CAP


def test_quirk_a_kind_1_edge_mixes_snc_and_scw():
    pr = S.build("chain6")
    idx, ei, ej, meas = M.measurements(pr)
    k = [n for n in range(len(ei)) if pr.has_nc[ei[n]] and not pr.has_nc[ej[n]] and pr.edge_kind[idx[n]]]
    assert k                                                                         # the edge from the first corrected keyframe to its uncorrected parent
    want = M.sim3_mul(M.sim3_of(pr.Scw[ej[k]]), M.sim3_inverse(M.sim3_of(pr.Snc[ei[k]])))
    assert np.array_equal(M.sim3_vec(meas)[k], M.sim3_vec(want))
    b = M.optimize(pr, fix=["nc_both"])
    assert S.rel(S.model("chain6").Scw_out, b.Scw_out) > 1e-4


def test_quirk_points_without_a_reference_stay():
    pr = S.build("fixed_mid")
    a, b = S.model("fixed_mid"), M.optimize(pr, fix=["all_points"])
    none = pr.pt_ref < 0
    assert none.sum() >= 3 and np.array_equal(a.pos[none], pr.pos[none]) and not np.array_equal(b.pos[none], pr.pos[none])
    assert np.abs(a.pos[~none] - pr.pos[~none]).max() > 1e-6


def test_statuses():
    pr = S.build("chain6")
    pr.fixed[:] = 1
    assert M.optimize(pr).status == M.EG_NO_FREE_VERTEX
    pr = S.build("chain6")
    pr.edge_i[:] = pr.edge_j
    m = M.optimize(pr)
    assert m.status == M.EG_FAILED and m.n_edges == 0
    pr = S.build("chain6")
    pr.Scw[1, 0] = np.inf
    assert M.optimize(pr).status == M.EG_NONFINITE


@pytest.mark.parametrize("n", [5, 32, 77, 161, 230])
def test_the_blocked_solve(n):
    """both forms of ldlt_solve (the exact column order up to kExactSolve unknowns, one product per panel above) solve the system, agree with each other to
    rounding, and fail on a zero or non-finite pivot"""
    rng = np.random.default_rng(n)
    A = rng.normal(0, 1, (n, n))
    H = A @ A.T + n * np.eye(n)
    b = rng.normal(0, 1, n)
    ok, x = M.ldlt_solve(H, b)
    ok2, x2 = M.ldlt_solve(H, b, reverse=True)
    want = np.linalg.solve(H, b)
    assert ok and ok2 and np.abs(x - want).max() <= 1e-12 * np.abs(want).max() and np.abs(x2 - x).max() <= 1e-12 * np.abs(want).max()
    keep = M.kExactSolve
    try:
        M.kExactSolve = 0 if n <= keep else 10 ** 6
        ok3, x3 = M.ldlt_solve(H, b)
    finally:
        M.kExactSolve = keep
    assert ok3 and np.abs(x3 - x).max() <= 1e-12 * np.abs(want).max()
    H[n // 2, :] = H[:, n // 2] = 0.0
    assert M.ldlt_solve(H, b) == (False, None)
    H[0, 0] = np.nan
    assert M.ldlt_solve(H, b) == (False, None)


@pytest.mark.parametrize("name", [n for n in S.SCENES if n != "identity"])
def test_scene_keeps_its_margins_and_its_spread(name):
    """what the GPU test asserts again: the ten runs of the spread take the same decisions, every decision keeps its margin, and the spread stays within
    MAX_SPREAD, so that twice the largest one — the device's tolerance — stays within 1e-4"""
    spread, margin, same = S.spread(name)
    print("%s: spread %.3g, margin / MARGIN %.3g" % (name, spread, margin))
    assert same and margin >= 1.0 and spread <= S.MAX_SPREAD, (name, spread, margin)
    assert S.model(name).status == M.EG_OK and 2 * spread <= 1e-4


def test_scale_scene_runs_every_branch_of_log():
    assert S.model("scale").branches == {0, 1, 2, 3}
    pr = S.build("scale")
    assert sorted(np.round(pr.Scw[pr.has_nc != 0, 7] / 1.0, 2).tolist())[0] == 0.93 and round(float(pr.Scw[6, 7]), 2) == 1.07
