"""cOptimizer::PoseOptimization (src/cOptimizer.cpp:259-459) restated statement by statement: numpy, FP64, no GPU.  What the device is held to.

Sources restated (reference tree): the problem set-up src/cOptimizer.cpp:259-459; the residual EdgeProjectXYZ2MCS::computeError
(src/g2o_MultiCol_vertices_edges.cpp:26-53) over cayley2hom (include/misc.h:133-160, 212-224), cConverter::invMat (src/cConverter.cpp:31-44) and
cCamModelGeneral_::WorldToImg (src/cam_model_omni.cpp:146-161); the update x + dx of VertexMt_cayley; RobustKernelHuber::robustify
(ThirdParty/g2o/g2o/core/robust_kernel_impl.cpp:78-91); BaseMultiEdge::constructQuadraticForm (core/base_multi_edge.hpp:36-48);
OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-164); SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-419);
SparseOptimizerTerminateAction (core/sparse_optimizer_terminate_action.cpp:21-57); Solver::resize (core/solver.cpp:46-66: x starts from zeros).

The Jacobian is NOT the reference's generated code: it is derived here by the chain rule (jacobian()), and test_poseopt_cpu.py holds it to a central
difference of the residual.

What the sources say about each edge's stored _error.  The terminate action calls computeActiveErrors() itself (:29) before it reads activeRobustChi2(), in
every post-iteration call, and SparseOptimizer::optimize calls postIteration after EVERY iteration, whatever solve() returned (:413).  So after an iteration
the active edges' errors are those of the CURRENT estimate (after a rejected trial: of the restored one), and the gain test and both outlier passes judge
the returned pose.  `fix={"stale_errors"}` is the other reading (the action reads what the last trial left), kept for the test that tells the two apart.

The 6x6 solve is an UNPIVOTED LDL^T (ldlt6), "not positive" = some pivot is not > 0: the project's choice, the same in the kernel.
"""
import math

import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)
POSE_OK, POSE_NONFINITE = 0, 1
# why a round ended: its 10 iterations ran; the terminate action set the stop flag; solve() returned Terminate (10 trials or rho == 0); solve() returned
# Terminate by the nBad >= 3 rule; the round never started (stop flag still set, or the problem was not optimised)
STOP_ITERATIONS, STOP_GAIN, STOP_TRIALS, STOP_NBAD, STOP_NOT_RUN = 0, 1, 2, 3, 4


def cayley2rot(c):   # include/misc.h:133-160
    c1, c2, c3 = float(c[0]), float(c[1]), float(c[2])
    c1s, c2s, c3s = c1 * c1, c2 * c2, c3 * c3
    scale = 1.0 + c1s + c2s + c3s
    R = np.array([[1 + c1s - c2s - c3s, 2 * (c1 * c2 - c3), 2 * (c1 * c3 + c2)],
                  [2 * (c1 * c2 + c3), 1 - c1s + c2s - c3s, 2 * (c2 * c3 - c1)],
                  [2 * (c1 * c3 - c2), 2 * (c2 * c3 + c1), 1 - c1s - c2s + c3s]], np.float64)
    return (1 / scale) * R


def cayley2hom(c6):   # :212-224
    M = np.zeros((4, 4))
    M[:3, :3] = cayley2rot(c6[:3])
    M[:3, 3] = [float(v) for v in c6[3:6]]
    M[3, 3] = 1.0
    return M


def matx_mul(A, B):   # cv::Matx product: s = 0; s += a(i,k) * b(k,j) in increasing k
    n, m, p = A.shape[0], A.shape[1], B.shape[1]
    out = np.zeros((n, p))
    for i in range(n):
        for j in range(p):
            s = 0.0
            for k in range(m):
                s += float(A[i, k]) * float(B[k, j])
            out[i, j] = s
    return out


def inv_mat(M):   # cConverter::invMat
    Rt = M[:3, :3].T.copy()
    t = matx_mul(-Rt, M[:3, 3:4])[:, 0]
    out = np.zeros((4, 4))
    out[:3, :3] = Rt
    out[:3, 3] = t
    out[3, 3] = 1.0
    return out


def rig_from_min(pose, Mc_min):   # cMultiCamSys_::Set_M_t_from_min (src/cam_system_omni.cpp:170-183): MtMc[c], MtMc_inv[c]
    Mt = cayley2hom(pose)
    MtMc = [matx_mul(Mt, cayley2hom(mc)) for mc in Mc_min]
    return np.stack(MtMc), np.stack([inv_mat(M) for M in MtMc])


def _atan(a):   # libm's atan, element by element (numpy's vector arctan is another implementation)
    return np.array([math.atan(v) for v in a], np.float64)


def _horner(coeffs, x):   # include/misc.h:115-122
    res = np.zeros_like(x)
    for c in coeffs[::-1]:
        res = res * x + c
    return res


def world_to_img(cam, x, y, z):   # WorldToImg
    norm = np.sqrt(x * x + y * y)
    norm = np.where(norm == 0.0, 1e-14, norm)
    theta = _atan(-z / norm)
    rho = _horner(cam["invP"], theta)
    uu = x / norm * rho
    vv = y / norm * rho
    return uu * cam["c"] + vv * cam["d"] + cam["u0"], uu * cam["e"] + vv + cam["v0"]


def d_world_to_img(cam, x, y, z):
    """d(u, v) / d(x, y, z) of WorldToImg by the chain rule: [m][2][3].  The norm == 0 -> 1e-14 branch is a constant (its derivative is 0)."""
    n0 = np.sqrt(x * x + y * y)
    const = n0 == 0.0
    n = np.where(const, 1e-14, n0)
    dn = np.stack([np.where(const, 0.0, x / n), np.where(const, 0.0, y / n), np.zeros_like(x)], 1)   # dn/d(x, y, z)
    q = -z / n
    theta = _atan(q)
    dth_dq = 1.0 / (1.0 + q * q)
    dq = (z / (n * n))[:, None] * dn
    dq[:, 2] = -1.0 / n
    dth = dth_dq[:, None] * dq
    inv = np.asarray(cam["invP"], np.float64)
    rho = _horner(inv, theta)
    drho = _horner(inv[1:] * np.arange(1, len(inv)), theta)[:, None] * dth
    fx, fy = x / n, y / n
    dfx = -(x / (n * n))[:, None] * dn
    dfx[:, 0] += 1.0 / n
    dfy = -(y / (n * n))[:, None] * dn
    dfy[:, 1] += 1.0 / n
    duu = dfx * rho[:, None] + fx[:, None] * drho
    dvv = dfy * rho[:, None] + fy[:, None] * drho
    return np.stack([duu * cam["c"] + dvv * cam["d"], duu * cam["e"] + dvv], 1)


def d_cayley2rot(c):
    """dR/dc_i of cayley2rot, i = 0..2: R = N / s, s = 1 + |c|^2, so dR = (dN - 2 c_i R) / s."""
    c1, c2, c3 = float(c[0]), float(c[1]), float(c[2])
    s = 1.0 + c1 * c1 + c2 * c2 + c3 * c3
    R = cayley2rot(c)
    dN = [np.array([[2 * c1, 2 * c2, 2 * c3], [2 * c2, -2 * c1, -2.0], [2 * c3, 2.0, -2 * c1]]),
          np.array([[-2 * c2, 2 * c1, 2.0], [2 * c1, 2 * c2, 2 * c3], [-2.0, 2 * c3, -2 * c2]]),
          np.array([[-2 * c3, -2.0, 2 * c1], [2.0, -2 * c3, 2 * c2], [2 * c1, 2 * c2, 2 * c3]])]
    return [(dN[i] - 2.0 * (c1, c2, c3)[i] * R) / s for i in range(3)]


class Problem:
    """One frame as PoseOptimization reads it.  keys: [n] structured (x, y float32, octave) or an [n][2] float32 array with `octave`; points: ids into pos, -1 = NULL."""

    def __init__(self, xy, octave, cam, points, pos, Mc_min, cams, inv_sigma2, pose0, huber=1.0):
        self.xy = np.asarray(xy, np.float32)
        self.octave = np.asarray(octave, np.int32)
        self.cam = np.asarray(cam, np.int32)
        self.points = np.asarray(points, np.int32)
        self.pos = np.asarray(pos, np.float64).reshape(-1, 3)
        self.Mc_min = np.asarray(Mc_min, np.float64).reshape(-1, 6)
        self.cams = cams
        self.inv_sigma2 = np.asarray(inv_sigma2, np.float64)
        self.pose0 = np.asarray(pose0, np.float64).copy()
        self.huber = float(huber)
        self.n = len(self.points)

    def edges(self, guard=True):
        """feature index of every edge, in feature order (:348-403): `if (pMP)` alone.  guard: the device kind's guards (a feature whose point id, camera or
        octave is out of range contributes no edge)."""
        ok = self.points >= 0
        if guard:
            ok &= (self.points < len(self.pos)) & (self.cam >= 0) & (self.cam < len(self.Mc_min)) & (self.octave >= 0) & (self.octave < len(self.inv_sigma2))
        return np.nonzero(ok)[0]


def project(pr, pose, idx):
    """(u, v) of the edges idx at `pose`: computeError up to WorldToImg."""
    _, inv = rig_from_min(pose, pr.Mc_min)
    X = pr.pos[pr.points[idx]]
    u, v = np.zeros(len(idx)), np.zeros(len(idx))
    for c in range(len(pr.Mc_min)):
        m = pr.cam[idx] == c
        if not m.any():
            continue
        M = inv[c]
        p = [((M[r, 0] * X[m, 0] + M[r, 1] * X[m, 1]) + M[r, 2] * X[m, 2]) + M[r, 3] * 1.0 for r in range(3)]   # Matx44 * Vec4, increasing k
        u[m], v[m] = world_to_img(pr.cams[c], p[0], p[1], p[2])
    return u, v


def residual(pr, pose, idx):
    u, v = project(pr, pose, idx)
    z = pr.xy[idx].astype(np.float64)
    return np.stack([z[:, 0] - u, z[:, 1] - v], 1)


def jacobian(pr, pose, idx):
    """d e / d pose, [m][2][6], by the chain rule.  With Mct = Mt * Mc: p = Rc^T Rt^T (X - t) - Rc^T tc, so dp/dt = -(Rt Rc)^T and
    dp/dc_i = Rc^T (dRt/dc_i)^T (X - t); then e = z - (u, v)."""
    Rt = cayley2rot(pose[:3])
    dRt = d_cayley2rot(pose[:3])
    d = pr.pos[pr.points[idx]] - pose[3:6][None, :]
    J = np.zeros((len(idx), 2, 6))
    _, inv = rig_from_min(pose, pr.Mc_min)
    for c in range(len(pr.Mc_min)):
        m = pr.cam[idx] == c
        if not m.any():
            continue
        Rc = cayley2rot(pr.Mc_min[c][:3])
        M = inv[c]
        X = pr.pos[pr.points[idx]][m]
        p = [((M[r, 0] * X[:, 0] + M[r, 1] * X[:, 1]) + M[r, 2] * X[:, 2]) + M[r, 3] * 1.0 for r in range(3)]
        D = d_world_to_img(pr.cams[c], p[0], p[1], p[2])            # [m][2][3]
        dp = np.zeros((int(m.sum()), 3, 6))
        for i in range(3):
            dp[:, :, i] = d[m] @ (Rc.T @ dRt[i].T).T
        dp[:, :, 3:6] = -(Rt @ Rc).T[None, :, :]
        J[m] = -np.einsum("mij,mjk->mik", D, dp)
    return J


def ldlt6(A, b):
    """Unpivoted LDL^T of the symmetric A, then the solve.  (ok, x): ok is False as soon as a pivot is not > 0 (NaN included), and x is then not computed."""
    n = len(b)
    L = np.eye(n)
    d = np.zeros(n)
    for j in range(n):
        s = float(A[j, j])
        for k in range(j):
            s -= L[j, k] * L[j, k] * d[k]
        if not s > 0.0:
            return False, None
        d[j] = s
        for i in range(j + 1, n):
            t = float(A[i, j])
            for k in range(j):
                t -= L[i, k] * L[j, k] * d[k]
            L[i, j] = t / s
    y = np.zeros(n)
    for i in range(n):
        t = float(b[i])
        for k in range(i):
            t -= L[i, k] * y[k]
        y[i] = t
    y = y / d
    x = np.zeros(n)
    for i in range(n - 1, -1, -1):
        t = float(y[i])
        for k in range(i + 1, n):
            t -= L[k, i] * x[k]
        x[i] = t
    return True, x


class Result:
    pass


def sum_margin(a, b):
    """relative distance of two chi2 sums, scaled by 1e3 (DECISION MARGINS).  An infinite sum is infinitely far from a finite one; a NaN sum decides by being
    NaN, which nothing here can vouch for: distance 0."""
    if math.isnan(a) or math.isnan(b):
        return 0.0
    if math.isinf(a) or math.isinf(b):
        return 0.0 if a == b else math.inf
    return abs(a - b) / max(abs(a), abs(b), 1e-300) * 1e3


def threshold_margin(c2, t):
    """smallest distance of the values c2 from the threshold t >= 0 they are compared with, relative to t.  Against an infinite threshold a finite value is
    infinitely far from its edge; against t == 0 there is nothing to be relative to and the distance is the value itself."""
    c2 = np.asarray(c2, np.float64)
    if math.isinf(t):
        return float(np.min(np.where(c2 == t, 0.0, math.inf)))
    if t == 0.0:
        return float(np.min(np.abs(c2)))
    return float(np.min(np.abs(c2 - t) / t))


def optimize(pr, reverse=False, fix=(), guard=True):
    with np.errstate(all="ignore"):
        return _optimize(pr, reverse, fix, guard)


def _optimize(pr, reverse, fix, guard):
    """PoseOptimization on one problem.  reverse: every sum over the edges runs in reversed index order (the spread measurement of the GPU tests).
    fix: the set of quirks "repaired" (for the tests that show each one matters): stale_errors, clear_stop, skip_bad (needs pr.bad), second_all_levels,
    reset_nbad, second_clears, share_is_inliers."""
    fix = set(fix)
    res = Result()
    idx_all = pr.edges(guard)
    if "skip_bad" in fix:
        keep = np.ones(len(idx_all), bool)
        seen = set()
        for k, i in enumerate(idx_all):
            pid = int(pr.points[i])
            if pr.bad[pid] or pid in seen:
                keep[k] = False
            seen.add(pid)
        idx_all = idx_all[keep]
    nInitial = len(idx_all)
    res.status, res.pose = POSE_OK, pr.pose0.copy()
    res.outlier = np.zeros(pr.n, np.uint8)
    res.iters, res.stop, res.trials = [0, 0], [STOP_NOT_RUN, STOP_NOT_RUN], np.zeros((2, 10), np.int32)
    res.lam, res.chi2, res.n_inliers, res.share, res.margin = 0.0, 0.0, 0, 0.0, math.inf
    res.nInitial = nInitial
    # what the tests of the hostile scenes ask about a run: failed 6x6 solves, active edges at the start of each round, the [build, trial] passes behind the
    # first evaluation that held a non-finite sum
    res.failed_solves, res.n_active, res.late_nonfinite, res.flag_margin = 0, [nInitial, 0], [0, 0], math.inf   # flag_margin: of the two outlier passes alone
    res.accepted_failed = 0
    if nInitial == 0:   # quirk 6: nothing is optimised
        res.MtMc, res.MtMc_inv = rig_from_min(res.pose, pr.Mc_min)
        return res
    delta = 1.345 * pr.huber
    dsqr = delta * delta
    th2 = delta * delta          # thHuber2 (:409): the same product
    omega = pr.inv_sigma2[pr.octave[idx_all]]
    level = np.zeros(nInitial, np.int32)
    margins = []

    def not_optimised():   # the project's choice: pose unchanged, no flag, every edge counted
        res.status = POSE_NONFINITE
        res.n_inliers, res.share = nInitial, 0.0
        res.MtMc, res.MtMc_inv = rig_from_min(res.pose, pr.Mc_min)
        return res

    def ssum(a):   # one ordered chain over the edges
        a = a[::-1] if reverse else a
        return np.cumsum(a, axis=0)[-1]

    def chi2_of(e, w):   # _error.dot(information() * _error), information = I * invSigma2
        return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])

    def robust(c2, track=True):   # robustify: rho[0], rho[1]
        inl = c2 <= dsqr
        if track and len(c2):
            margins.append(threshold_margin(c2, dsqr))
        sq = np.sqrt(np.where(inl, 1.0, c2))
        return np.where(inl, c2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)

    pose = pr.pose0.copy()
    state = {"err": residual(pr, pose, idx_all)}   # every edge's stored _error (only read by the stale_errors reading before the first evaluation)

    def active_errors(act):   # computeActiveErrors
        state["err"] = state["err"].copy()
        state["err"][act] = residual(pr, pose, idx_all[act])

    def active_robust_chi2(act):
        if not act.any():
            return 0.0
        return float(ssum(robust(chi2_of(state["err"][act], omega[act]))[0]))

    stop_flag = False
    last_chi = 0.0
    nBad = 0
    x = np.zeros(6)
    lam, ni = -1.0, 2.0
    for rnd in range(2):
        act = level == 0
        if rnd == 1 and "second_all_levels" in fix:
            act = np.ones(nInitial, bool)
        if rnd == 1 and "clear_stop" in fix:
            stop_flag = False
        res.n_active[rnd] = int(act.sum())
        x = np.zeros(6)           # buildStructure -> Solver::resize: zeros
        result_ok = True
        it = 0
        stop = STOP_NOT_RUN if stop_flag or not act.any() else STOP_ITERATIONS   # no active edge: optimize() returns before its loop (:356-359)
        lm_bad = 0
        while it < 10 and not stop_flag and result_ok and act.any():
            # ---- OptimizationAlgorithmLevenberg::solve(it)
            active_errors(act)
            first = rnd == 0 and it == 0
            # the screen of the first evaluation: every edge's residual, Jacobian and weight, the Huber pair (delta, delta^2) ...
            if first and not (np.isfinite(state["err"]).all() and np.isfinite(jacobian(pr, pose, idx_all)).all() and np.isfinite(omega).all()
                              and math.isfinite(delta) and math.isfinite(dsqr)):
                return not_optimised()
            currentChi = active_robust_chi2(act)
            iniChi = currentChi
            e = state["err"][act]
            w = omega[act]
            J = jacobian(pr, pose, idx_all[act])
            rho1 = robust(chi2_of(e, w), track=False)[1]
            rw = rho1 * w                                           # robustInformation = rho[1] * information
            H = np.zeros((6, 6))
            for a in range(6):
                for c in range(a, 6):
                    H[a, c] = H[c, a] = ssum(rw * (J[:, 0, a] * J[:, 0, c] + J[:, 1, a] * J[:, 1, c]))
            b = np.array([ssum(-rw * (J[:, 0, a] * e[:, 0] + J[:, 1, a] * e[:, 1])) for a in range(6)])
            if first and not (np.isfinite(H).all() and np.isfinite(b).all() and math.isfinite(currentChi)):   # ... and the sums it reduces to
                return not_optimised()
            res.late_nonfinite[0] += not (np.isfinite(H).all() and np.isfinite(b).all() and math.isfinite(currentChi))
            if it == 0:
                lam, ni, lm_bad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
            rho, qmax = 0.0, 0
            while True:
                backup = pose.copy()                                # push
                ok2, sol = ldlt6(H + lam * np.eye(6), b)
                if ok2:
                    x = sol
                else:
                    res.failed_solves += 1
                pose = pose + x                                     # oplus, with the stale x after a failed solve
                active_errors(act)
                tempChi = active_robust_chi2(act)
                res.late_nonfinite[1] += not math.isfinite(tempChi)
                if not ok2:
                    tempChi = DBL_MAX
                rho = currentChi - tempChi
                scale = 0.0
                for j in range(6):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                if not ok2 and not math.isnan(scale):   # the stale x against the new b: scale has either sign, and with tempChi = DBL_MAX it alone decides the trial (DECISION MARGINS)
                    margins.append(abs(scale) / max(sum(abs(x[j] * (lam * x[j] + b[j])) for j in range(6)) + 1e-3, 1e-300))
                rho = float(np.float64(rho) / np.float64(scale))                 # IEEE division: inf or NaN where C++ gives them
                margins.append(sum_margin(currentChi, tempChi))   # sign of rho: see DECISION MARGINS
                if rho > 0 and math.isfinite(tempChi):
                    res.accepted_failed += not ok2                  # DBL_MAX is finite: a failed solve whose scale is negative is accepted
                    try:
                        alpha = 1.0 - (2 * rho - 1) ** 3
                    except OverflowError:                           # pow() gives the infinity where Python's ** raises
                        alpha = -math.inf
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    currentChi = tempChi
                else:
                    lam *= ni
                    ni *= 2
                    pose = backup                                   # pop
                qmax += 1
                if not (rho < 0 and qmax < 10 and not stop_flag):
                    break
            res.trials[rnd, it] = qmax
            if qmax == 10 or rho == 0:
                result_ok, stop = False, STOP_TRIALS
            else:
                margins.append(abs((iniChi - currentChi) * 1e3 - iniChi) / max(abs(iniChi), 1e-300))
                lm_bad = lm_bad + 1 if (iniChi - currentChi) * 1e3 < iniChi else 0
                if lm_bad >= 3:
                    result_ok, stop = False, STOP_NBAD
            # ---- postIteration(it): the terminate action
            if "stale_errors" not in fix:
                active_errors(act)
            if it == 0:
                last_chi = active_robust_chi2(act)
            else:
                cur = active_robust_chi2(act)
                gain = float(np.float64(last_chi - cur) / np.float64(cur))
                margins.append(abs(last_chi - cur) / max(abs(cur), 1e-300) * 1e3)         # gain >= 0
                margins.append(abs(gain - 1e-6) / 1e-6)                                   # gain < threshold
                last_chi = cur
                if gain >= 0 and gain < 1e-6:
                    stop_flag = True
                    if result_ok:
                        stop = STOP_GAIN
            it += 1
        res.iters[rnd], res.stop[rnd] = it, stop
        # ---- the outlier pass behind this round (:412-427, :433-447)
        c2 = chi2_of(state["err"], omega)
        if rnd == 0:
            margins.append(threshold_margin(c2, th2))
            res.flag_margin = min(res.flag_margin, margins[-1])
            level[c2 > th2] = 1
            nBad = int((c2 > th2).sum())
        else:
            if "reset_nbad" in fix:
                nBad = 0
            live = level == 0
            if "second_clears" in fix:                  # every edge judged again at the returned pose
                c2 = chi2_of(residual(pr, pose, idx_all), omega)
                live = np.ones(nInitial, bool)
                level[:] = 0
                nBad = 0
            if live.any():
                margins.append(threshold_margin(c2[live], th2))
                res.flag_margin = min(res.flag_margin, margins[-1])
            second = live & (c2 > th2)
            nBad += int(second.sum())
            level[second] = 1
    res.pose = pose
    res.outlier[idx_all[level == 1]] = 1
    res.lam, res.chi2 = lam, last_chi
    res.n_inliers = nInitial - nBad
    res.share = (nInitial - nBad) / nInitial if "share_is_inliers" in fix else nBad / nInitial
    res.MtMc, res.MtMc_inv = rig_from_min(pose, pr.Mc_min)
    res.margin = (0.0 if any(math.isnan(v) for v in margins) else min(margins)) if margins else math.inf   # a NaN distance vouches for nothing
    return res


# DECISION MARGINS.  Result.margin is the smallest distance of any decision from its edge, each relative to its threshold: every edge's chi2 against
# dsqr (the Huber switch, every evaluation) and against thHuber^2 (both outlier passes), the gain against 1e-6, the nBad rule's (iniChi - currentChi) * 1e3
# against iniChi.  A SIGN test (rho > 0, rho < 0, gain >= 0) has no threshold to be relative to: it compares two chi2 sums, and by construction it is taken
# when they differ by less than 1e-6 of themselves (that is when the gain test fires).  Its margin is the relative difference of the two sums, scaled by 1e3,
# so that margin >= 1e-6 means they differ by >= 1e-9 of themselves: three orders above the 1e-12 the summation order moves them.
# After a FAILED solve tempChi is DBL_MAX and the sign of rho is the sign of `scale`, the stale x against the new b, which cancels like any sum: its margin is
# |scale| relative to the sum of its terms' magnitudes.  (A scale of NaN, lambda = inf against x = 0, decides nothing: rho is NaN on either side.)
# threshold_margin() is the distance from a chi2 threshold: infinite against an infinite threshold, absolute against a threshold of 0.
MARGIN = 1e-6


def lafida_like_scene(seed, n_edges, cams, Mc_min, nlevels=8, noise=0.5, n_outliers=0, start=0.02, n_null=0):
    """A synthetic frame: points in front of the rig's cameras, projected at a true pose, keys = projection + noise (float32), start pose = true + offset."""
    rng = np.random.default_rng(seed)
    nr = len(Mc_min)
    true = np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)])
    n = n_edges + n_null
    cam = rng.integers(0, nr, n).astype(np.int32)
    octave = rng.integers(0, nlevels, n).astype(np.int32)
    MtMc, _ = rig_from_min(true, Mc_min)
    pos = np.zeros((n, 3))
    for i in range(n):   # a point 1-6 m along a ray of its camera, 20-70 degrees off its axis (+z)
        th, ph, r = rng.uniform(0.35, 1.2), rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 6.0)
        pc = np.array([r * np.sin(th) * np.cos(ph), r * np.sin(th) * np.sin(ph), r * np.cos(th), 1.0])
        pos[i] = (MtMc[cam[i]] @ pc)[:3]
    points = np.arange(n, dtype=np.int32)
    inv_sigma2 = 1.0 / (1.2 ** np.arange(nlevels)) ** 2
    pr = Problem(np.zeros((n, 2), np.float32), octave, cam, points, pos, Mc_min, cams, inv_sigma2, true, 1.0)
    u, v = project(pr, true, np.arange(n))
    xy = np.stack([u, v], 1) + rng.normal(0, noise, (n, 2))
    if n_outliers:
        bad = rng.choice(n_edges, n_outliers, replace=False)
        xy[bad] += rng.normal(0, 25.0, (n_outliers, 2))
    pr.xy = xy.astype(np.float32)
    if n_null:
        pr.points[rng.choice(n, n_null, replace=False)] = -1
    pr.pose0 = true + np.concatenate([rng.normal(0, start * 0.3, 3), rng.normal(0, start, 3)])
    return pr
