"""cOptimizer::LocalBundleAdjustment (src/cOptimizer.cpp:461-874) restated statement by statement: numpy, FP64, no GPU.  What mcs_local_bundle_adjustment is
held to.  The list-building and the fixing rules (:473-529, :555-595) are build_problem() below, over duck-typed keyframes and points; the rest takes arrays.

Sources restated (reference tree): the set-up and both passes, src/cOptimizer.cpp:531-873; cMapPoint::EraseObservation / TotalNrObservations
(src/cMapPoint.cpp:118-176); BlockSolver::buildSystem / solve / setLambda (ThirdParty/g2o/g2o/core/block_solver.hpp:354-486, 502-589); Eigen's closed-form 3x3
inverse (Eigen/src/LU/Inverse.h:117-158); OptimizationAlgorithmLevenberg::solve, computeLambdaInit, computeScale (core/optimization_algorithm_levenberg.cpp:
61-189); SparseOptimizer::optimize (core/sparse_optimizer.cpp:354-419); SparseOptimizerTerminateAction (core/sparse_optimizer_terminate_action.cpp:21-72).
The edge, the Cayley pieces and the derivative of WorldToImg come from tests/poseopt_model.py; the point Jacobian is derived here by the chain rule:
p = (Rt Rc)^T (X - t) - Rc^T tc, so dp/dX = (Rt Rc)^T = -dp/dt, and (Rt Rc)^T is the rotation block of invMat(Mt Mc).

What the sources say, where a reader might expect otherwise (DESIGN 7 lists them with their tests):
  * optimize() returns -1 (== OptimizationAlgorithm::Fail) only when no non-fixed vertex holds an active edge (:356-359) or init() fails; the `return 0` of
    :415-417 is NOT Fail.  So "Optimization failed" (:750, :788) means: no active edge.  Status LBA_FAILED.
  * EraseObservation counts every observation, those of bad keyframes included (:139-141); TotalNrObservations (:164-176) skips bad keyframes.  The problem
    carries both numbers per point: total_obs (all) and bad_obs (those at bad keyframes).
  * the terminate action's setMaxIterations(15) never fires: optimize(15) numbers its iterations 0..14.

Choices (the same in the library): the reduced system is solved by an unpivoted dense LDL^T in the call's keyframe order (fails on a pivot that is zero or
not finite); a free keyframe or a point without an active edge stays in the system with zero blocks (its step is 0, its pivot lambda) instead of leaving the
index mapping; the stop flag of a caller is read once per Levenberg trial, before the trial."""
import math

import numpy as np

import poseopt_model as PM
from poseopt_model import STOP_GAIN, STOP_ITERATIONS, STOP_NBAD, STOP_NOT_RUN, STOP_TRIALS, MARGIN, sum_margin, threshold_margin  # noqa: F401

DBL_MAX = PM.DBL_MAX
LBA_OK, LBA_NONFINITE, LBA_STOPPED, LBA_NO_FREE_POSE, LBA_FAILED, LBA_TOO_FEW = 0, 1, 2, 3, 4, 5
PT_WRITTEN, PT_KEPT, PT_BAD = 0, 1, 2
ROUND_ITERS = (10, 15)
MAX_FREE = 64


class Problem:
    def __init__(self, kf_pose, kf_fixed, n_local, pos, pt_first, edge_kf, edge_cam, xy, octave, Mc_min, cams, inv_sigma2, std_recon=2.0, total_obs=None,
                 bad_obs=None):
        self.kf_pose = np.asarray(kf_pose, np.float64).reshape(-1, 6).copy()
        self.kf_fixed = np.asarray(kf_fixed, np.uint8).copy()
        self.n_local = int(n_local)
        self.pos = np.asarray(pos, np.float64).reshape(-1, 3).copy()
        self.pt_first = np.asarray(pt_first, np.int32).copy()
        self.edge_kf = np.asarray(edge_kf, np.int32).copy()
        self.edge_cam = np.asarray(edge_cam, np.int32).copy()
        self.xy = np.asarray(xy, np.float32).reshape(-1, 2).copy()
        self.octave = np.asarray(octave, np.int32).copy()
        self.Mc_min = np.asarray(Mc_min, np.float64).reshape(-1, 6)
        self.cams = cams
        self.inv_sigma2 = np.asarray(inv_sigma2, np.float64)
        self.std_recon = float(std_recon)
        self.total_obs = None if total_obs is None else np.asarray(total_obs, np.int32).copy()
        self.bad_obs = None if bad_obs is None else np.asarray(bad_obs, np.int32).copy()

    @property
    def n_kfs(self):
        return len(self.kf_pose)

    @property
    def n_points(self):
        return len(self.pos)

    @property
    def n_edges(self):
        return len(self.edge_kf)

    def edge_point(self):
        """point of every edge (-1: the edge lies in no point's range) and the device kind's guards: an edge whose keyframe, camera or octave is out of range,
        or that lies in a range that is not inside [0, n_edges), contributes nothing"""
        ept = np.full(self.n_edges, -1, np.int32)
        for p in range(self.n_points):
            a, b = int(self.pt_first[p]), int(self.pt_first[p + 1])
            if 0 <= a <= b <= self.n_edges:
                ept[a:b] = p
        ok = (ept >= 0) & (self.edge_kf >= 0) & (self.edge_kf < self.n_kfs) & (self.edge_cam >= 0) & (self.edge_cam < len(self.Mc_min))
        ok &= (self.octave >= 0) & (self.octave < len(self.inv_sigma2))
        return ept, ok


def evaluate(pr, poses, pos, idx, ept, jac=True):
    """residual [m][2] of the edges idx at (poses, pos); jac: also d e / d pose [m][2][6] and d e / d point [m][2][3]"""
    m = len(idx)
    e, Jp, Jl = np.zeros((m, 2)), np.zeros((m, 2, 6)), np.zeros((m, 2, 3))
    kf, cam = pr.edge_kf[idx], pr.edge_cam[idx]
    key = kf.astype(np.int64) * len(pr.Mc_min) + cam
    order = np.argsort(key, kind="stable")
    cuts = np.nonzero(np.diff(key[order]))[0] + 1
    rig = {}
    for grp in np.split(order, cuts):
        if not len(grp):
            continue
        k, c = int(kf[grp[0]]), int(cam[grp[0]])
        pose = poses[k]
        if k not in rig:
            rig[k] = PM.rig_from_min(pose, pr.Mc_min)[1]
        M = rig[k][c]
        X = pos[ept[idx[grp]]]
        p = [((M[r, 0] * X[:, 0] + M[r, 1] * X[:, 1]) + M[r, 2] * X[:, 2]) + M[r, 3] * 1.0 for r in range(3)]
        u, v = PM.world_to_img(pr.cams[c], p[0], p[1], p[2])
        z = pr.xy[idx[grp]].astype(np.float64)
        e[grp, 0], e[grp, 1] = z[:, 0] - u, z[:, 1] - v
        if not jac:
            continue
        D = PM.d_world_to_img(pr.cams[c], p[0], p[1], p[2])
        dRt = PM.d_cayley2rot(pose[:3])
        Rc = PM.cayley2rot(pr.Mc_min[c][:3])
        d = X - pose[3:6][None, :]
        dp = np.zeros((len(grp), 3, 6))
        for i in range(3):
            dp[:, :, i] = d @ (Rc.T @ dRt[i].T).T
        dp[:, :, 3:6] = -M[:3, :3][None, :, :]
        Jp[grp] = -np.einsum("mij,mjk->mik", D, dp)
        Jl[grp] = -np.einsum("mij,jk->mik", D, M[:3, :3])
    return (e, Jp, Jl) if jac else e


def eigen_inv3(D):
    """Eigen's closed-form inverse of [n][3][3] (Inverse.h:117-158): cofactors, det = the column-0 cofactors dotted with column 0, result = cofactor * (1 / det)"""
    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return D[:, i1, j1] * D[:, i2, j2] - D[:, i1, j2] * D[:, i2, j1]
    c0 = [cof(0, 0), cof(1, 0), cof(2, 0)]
    det = (c0[0] * D[:, 0, 0] + c0[1] * D[:, 1, 0]) + c0[2] * D[:, 2, 0]
    inv = 1.0 / det
    out = np.zeros_like(D)
    for j in range(3):
        for i in range(3):
            out[:, j, i] = (c0[i] if j == 0 else cof(i, j)) * inv
    return out


def ldlt(A, b):
    """unpivoted LDL^T of the symmetric A (its lower triangle is read) and the solve -> (ok, x); ok is False at the first pivot that is zero or not finite"""
    A = np.array(A, np.float64)
    n = len(b)
    d = np.zeros(n)
    for j in range(n):
        dj = A[j, j]
        if dj == 0.0 or not math.isfinite(dj):
            return False, None
        d[j] = dj
        col = A[j + 1:, j] / dj
        A[j + 1:, j + 1:] -= np.outer(col, col) * dj
        A[j + 1:, j] = col
    y = np.array(b, np.float64)
    for k in range(n):
        y[k + 1:] -= A[k + 1:, k] * y[k]
    y /= d
    for k in range(n - 1, -1, -1):
        y[:k] -= A[k, :k] * y[k]
    return True, y


class System:
    """what buildSystem leaves: Hpp [F][6][6], bp [F][6], Hll [P][3][3], bl [P][3], and per active edge at a free keyframe its W block"""


def build_system(pr, fidx, ept, idx, e, Jp, Jl, rw, reverse=False):
    F, P = int((fidx >= 0).sum()), pr.n_points
    s = System()
    s.Hpp, s.bp, s.Hll, s.bl = np.zeros((F, 6, 6)), np.zeros((F, 6)), np.zeros((P, 3, 3)), np.zeros((P, 3))
    o = np.arange(len(idx))[::-1] if reverse else np.arange(len(idx))
    f = fidx[pr.edge_kf[idx]]
    p = ept[idx]
    HP = rw[:, None, None] * (Jp[:, 0, :, None] * Jp[:, 0, None, :] + Jp[:, 1, :, None] * Jp[:, 1, None, :])
    BP = -rw[:, None] * (Jp[:, 0, :] * e[:, 0:1] + Jp[:, 1, :] * e[:, 1:2])
    HL = rw[:, None, None] * (Jl[:, 0, :, None] * Jl[:, 0, None, :] + Jl[:, 1, :, None] * Jl[:, 1, None, :])
    BL = -rw[:, None] * (Jl[:, 0, :] * e[:, 0:1] + Jl[:, 1, :] * e[:, 1:2])
    of = o[f[o] >= 0]
    np.add.at(s.Hpp, f[of], HP[of])      # unbuffered: one ordered chain per block
    np.add.at(s.bp, f[of], BP[of])
    np.add.at(s.Hll, p[o], HL[o])
    np.add.at(s.bl, p[o], BL[o])
    s.W = rw[:, None, None] * (Jp[:, 0, :, None] * Jl[:, 0, None, :] + Jp[:, 1, :, None] * Jl[:, 1, None, :])   # [m][6][3]
    s.f, s.p, s.act_pt = f, p, np.zeros(P, bool)
    s.act_pt[p] = True
    return s


def schur_solve(s, lam, reverse=False):
    """BlockSolver::solve with the Schur complement -> (ok, xp [F][6], xl [P][3]); xl only of the points that hold an active edge"""
    F, P = len(s.Hpp), len(s.Hll)
    D = s.Hll + lam * np.eye(3)[None]
    Dinv = np.zeros_like(D)
    Dinv[s.act_pt] = eigen_inv3(D[s.act_pt])
    db = np.einsum("pij,pj->pi", Dinv, s.bl)
    S = np.zeros((6 * F, 6 * F))
    bs = s.bp.reshape(-1).copy()
    for f in range(F):
        S[6 * f:6 * f + 6, 6 * f:6 * f + 6] = s.Hpp[f] + lam * np.eye(6)
    at = np.nonzero(s.f >= 0)[0]
    at = at[np.argsort(s.p[at], kind="stable")]
    groups = np.split(at, np.nonzero(np.diff(s.p[at]))[0] + 1) if len(at) else []
    for grp in (groups[::-1] if reverse else groups):
        p = int(s.p[grp[0]])
        Wk = {}
        for k in grp:                    # two edges of one point at one keyframe add into one block
            Wk[int(s.f[k])] = Wk.get(int(s.f[k]), 0.0) + s.W[k]
        for i, Wi in Wk.items():
            T = Wi @ Dinv[p]
            bs[6 * i:6 * i + 6] -= Wi @ db[p]
            for j, Wj in Wk.items():
                if j >= i:
                    S[6 * i:6 * i + 6, 6 * j:6 * j + 6] -= T @ Wj.T
    iu = np.triu_indices(6 * F, 1)
    S.T[iu] = S[iu]                      # the lower triangle mirrors the upper
    ok, xp = ldlt(S, bs)
    if not ok:
        return False, None, None
    xp = xp.reshape(F, 6)
    cl = s.bl.copy()
    o = at[::-1] if reverse else at
    np.subtract.at(cl, s.p[o], np.einsum("mij,mi->mj", s.W[o], xp[s.f[o]]))
    xl = np.einsum("pij,pj->pi", Dinv, cl)
    return True, xp, xl


def full_system(s, lam):
    """the (6F + 3P) system the Schur complement reduces, dense: for the identity test"""
    F, P = len(s.Hpp), len(s.Hll)
    n = 6 * F + 3 * P
    H, b = np.zeros((n, n)), np.concatenate([s.bp.reshape(-1), s.bl.reshape(-1)])
    for f in range(F):
        H[6 * f:6 * f + 6, 6 * f:6 * f + 6] = s.Hpp[f] + lam * np.eye(6)
    for p in range(P):
        q = 6 * F + 3 * p
        H[q:q + 3, q:q + 3] = s.Hll[p] + lam * np.eye(3)
    for k in np.nonzero(s.f >= 0)[0]:
        i, q = 6 * int(s.f[k]), 6 * F + 3 * int(s.p[k])
        H[i:i + 6, q:q + 3] += s.W[k]
        H[q:q + 3, i:i + 6] += s.W[k].T
    return H, b


class Result:
    pass


def optimize(pr, stop_flag=None, reverse=False, fix=()):
    with np.errstate(all="ignore"):
        return _optimize(pr, stop_flag, reverse, set(fix))


def _optimize(pr, stop_flag, reverse, fix):
    """stop_flag: None (pbStopFlag == NULL) or a one-element list holding the caller's flag, read and written in place.  reverse: every sum over edges and
    points runs in reversed order.  fix: quirks "repaired", for the tests that show each one matters: own_flag (the action never writes the caller's flag),
    no_shield (an erasure never shields the edges behind it), write_all (every point is written back), fail_goes_on (a round without active edge is skipped)."""
    res = Result()
    E, P = pr.n_edges, pr.n_points
    res.status = LBA_OK
    res.kf_pose, res.pos = pr.kf_pose.copy(), pr.pos.copy()
    res.edge_state, res.pt_state = np.zeros(E, np.uint8), np.full(P, PT_KEPT, np.uint8)
    res.iters, res.stop, res.trials = [0, 0], [STOP_NOT_RUN, STOP_NOT_RUN], np.zeros((2, 15), np.int32)
    res.lam, res.chi2, res.margin = 0.0, 0.0, math.inf
    res.n_free, res.n_edges1, res.n_erased = 0, 0, [0, 0]
    res.failed_solves = 0
    margins = []

    def done(status):
        res.status = status
        res.margin = (0.0 if any(math.isnan(v) for v in margins) else min(margins)) if margins else math.inf
        res.kf_t = res.kf_pose[:pr.n_local, 3:6].copy()
        return res

    if pr.n_local < 2:                                   # :489
        return done(LBA_TOO_FEW)
    user = stop_flag is not None and "own_flag" not in fix
    aux = [False]
    flag = stop_flag if user else None                   # optimizer._forceStopFlag: the caller's, or null until the action attaches its own

    def terminate():
        return bool(flag[0]) if flag is not None else False

    if user and stop_flag[0]:                            # :739-741
        return done(LBA_STOPPED)
    fidx = np.full(pr.n_kfs, -1, np.int32)
    free = np.nonzero(pr.kf_fixed == 0)[0]
    fidx[free] = np.arange(len(free))
    res.n_free = len(free)
    if len(free) == 0:
        return done(LBA_NO_FREE_POSE)
    ept, valid = pr.edge_point()
    res.n_edges1 = int(valid.sum())
    delta = 1.345 * pr.std_recon
    dsqr = delta * delta
    th2 = delta * delta
    omega_all = np.where(valid, pr.inv_sigma2[np.clip(pr.octave, 0, len(pr.inv_sigma2) - 1)], 0.0)
    level = np.where(valid, 0, 1).astype(np.int32)
    poses, pos = pr.kf_pose.copy(), pr.pos.copy()
    deg = np.zeros(P, np.int64)
    np.add.at(deg, ept[valid], 1)
    total = deg.copy() if pr.total_obs is None else pr.total_obs.astype(np.int64).copy()
    bad_obs = np.zeros(P, np.int64) if pr.bad_obs is None else pr.bad_obs.astype(np.int64)
    bad = np.zeros(P, bool)

    def ssum(a):
        a = a[::-1] if reverse else a
        return float(np.cumsum(a)[-1]) if len(a) else 0.0

    def chi2_of(e, w):
        return e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])

    def robust(c2, track=True):
        inl = c2 <= dsqr
        if track and len(c2):
            margins.append(threshold_margin(c2, dsqr))
        sq = np.sqrt(np.where(inl, 1.0, c2))
        return np.where(inl, c2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)

    def robust_chi2(idx, at_poses, at_pos):
        e = evaluate(pr, at_poses, at_pos, idx, ept, jac=False)
        return ssum(robust(chi2_of(e, omega_all[idx]))[0])

    last_chi, lam, ni = 0.0, -1.0, 2.0
    for rnd in range(2):
        idx = np.nonzero(level == 0)[0]
        if len(idx) == 0:                                # optimize() returns -1 == Fail (:750-754, :788-792)
            if "fail_goes_on" not in fix:
                res.pt_state[bad] = PT_BAD                 # round two: the erasures and bad flags of pass one are already applied
                return done(LBA_FAILED)
        F = len(free)
        xp, xl = np.zeros((F, 6)), np.zeros((P, 3))     # buildStructure -> Solver::resize: zeros
        w = omega_all[idx]
        it, stop, result_ok, lm_bad = 0, STOP_ITERATIONS, True, 0
        if terminate() or len(idx) == 0:
            stop = STOP_NOT_RUN
        while it < ROUND_ITERS[rnd] and not terminate() and result_ok and len(idx):
            e, Jp, Jl = evaluate(pr, poses, pos, idx, ept)
            first = rnd == 0 and it == 0
            if first and not (np.isfinite(e).all() and np.isfinite(Jp).all() and np.isfinite(Jl).all() and np.isfinite(w).all() and math.isfinite(dsqr)):
                return done(LBA_NONFINITE)
            rho0, rho1 = robust(chi2_of(e, w))
            currentChi = iniChi = ssum(rho0)
            s = build_system(pr, fidx, ept, idx, e, Jp, Jl, rho1 * w, reverse)
            if first and not (np.isfinite(s.Hpp).all() and np.isfinite(s.bp).all() and np.isfinite(s.Hll).all() and np.isfinite(s.bl).all()
                              and math.isfinite(currentChi)):
                return done(LBA_NONFINITE)
            if it == 0:                                  # computeLambdaInit: poses AND points
                md = max(float(np.abs(np.einsum("fii->fi", s.Hpp)).max()), float(np.abs(np.einsum("pii->pi", s.Hll)).max()))
                lam, ni, lm_bad = 1e-5 * md, 2.0, 0
            post_chi = currentChi
            rho, qmax = 0.0, 0
            while True:
                stop_seen = terminate()                  # the caller's flag as the trial's enqueue reads it
                ok2, sxp, sxl = schur_solve(s, lam, reverse)
                if ok2:
                    xp = sxp
                    xl = np.where(s.act_pt[:, None], sxl, xl)
                else:
                    res.failed_solves += 1
                t_poses, t_pos = poses.copy(), pos.copy()
                t_poses[free] += xp                      # oplus, with the stale x after a failed solve
                t_pos[s.act_pt] += xl[s.act_pt]
                raw = robust_chi2(idx, t_poses, t_pos)
                tempChi = raw if ok2 else DBL_MAX
                rho = currentChi - tempChi
                sc_p = xp * (lam * xp + s.bp)
                sc_l = (xl * (lam * xl + s.bl))[s.act_pt]
                scale = ssum(sc_p.reshape(-1)) + ssum(sc_l.sum(1))
                scale += 1e-3
                rho = float(np.float64(rho) / np.float64(scale))
                margins.append(sum_margin(currentChi, tempChi))
                if rho > 0 and math.isfinite(tempChi):
                    try:
                        alpha = 1.0 - (2 * rho - 1) ** 3
                    except OverflowError:
                        alpha = -math.inf
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    currentChi = tempChi
                    post_chi = raw
                    poses, pos = t_poses, t_pos          # discardTop
                else:
                    lam *= ni
                    ni *= 2
                qmax += 1
                if not (rho < 0 and qmax < 10 and not stop_seen):
                    break
            res.trials[rnd, it] = qmax
            if qmax == 10 or rho == 0:
                result_ok, stop = False, STOP_TRIALS
            else:
                margins.append(abs((iniChi - currentChi) * 1e3 - iniChi) / max(abs(iniChi), 1e-300))
                lm_bad = lm_bad + 1 if (iniChi - currentChi) * 1e3 < iniChi else 0
                if lm_bad >= 3:
                    result_ok, stop = False, STOP_NBAD
            # ---- postIteration(it): the terminate action, on the errors of the current estimate
            if it == 0:
                last_chi = post_chi
            else:
                gain = float(np.float64(last_chi - post_chi) / np.float64(post_chi))
                margins.append(abs(last_chi - post_chi) / max(abs(post_chi), 1e-300) * 1e3)
                margins.append(abs(gain - 1e-6) / 1e-6)
                last_chi = post_chi
                if gain >= 0 and gain < 1e-6:            # setOptimizerStopFlag(true): through the caller's pointer if there is one (:64-72)
                    if flag is None:
                        flag = aux
                    flag[0] = True
                    if result_ok:
                        stop = STOP_GAIN
            it += 1
        res.iters[rnd], res.stop[rnd] = it, stop
        res.lam, res.chi2 = lam, last_chi
        if rnd == 0 and user and stop_flag[0]:           # :756-762: bDoMore = false, nothing at all is written back
            return done(LBA_STOPPED)
        # ---- the pass behind this round (:764-783, :795-816): sequential inside a point, the point's bad flag shields what lies behind an erasure
        c2 = chi2_of(evaluate(pr, poses, pos, idx, ept, jac=False), w) if len(idx) else np.zeros(0)
        tested = []
        for k, ed in enumerate(idx):
            p = int(ept[ed])
            if bad[p] and "no_shield" not in fix:
                continue
            tested.append(k)
            if c2[k] > th2:
                res.edge_state[ed] = rnd + 1
                level[ed] = 1
                res.n_erased[rnd] += 1
                total[p] -= 1
                if total[p] < 2:                         # EraseObservation: nrObs < 2 -> SetBadFlag
                    bad[p] = True
        if tested:
            margins.append(threshold_margin(c2[tested], th2))
    # ---- write-back (:825-869)
    res.kf_pose[:pr.n_local] = poses[:pr.n_local]
    for p in range(P):
        if bad[p]:
            res.pt_state[p] = PT_BAD
        elif "write_all" in fix or (total[p] - bad_obs[p] > 1 and deg[p] >= 2):
            res.pt_state[p] = PT_WRITTEN
            res.pos[p] = pos[p]
    return done(LBA_OK)


# ---------------------------------------------------------------------------------------------- the lists and the fixing rules (:473-529, :555-595)
def build_problem(pKF, Mc_min, cams, inv_sigma2, std_recon=2.0):
    """The three lists and the arrays of the call from duck-typed objects.  A keyframe: mnId, isBad(), GetVectorCovisibleKeyFrames(), GetMapPointMatches(),
    pose_min (Get_M_t_min()), keypoint_to_cam, GetKeyPoint(i) -> dict(x, y, octave).  A point: mnId, isBad(), GetObservations() -> {keyframe: [feature, ...]},
    GetWorldPos().  std::map<cMultiKeyFrame*, ...> iterates in ascending mnId (the project's convention).
    -> (Problem, lLocalKeyFrames, lFixedCameras, lLocalMapPoints, edge_feature [n_edges])"""
    local = [pKF] + [k for k in pKF.GetVectorCovisibleKeyFrames() if not k.isBad()]
    in_local = {id(k) for k in [pKF] + list(pKF.GetVectorCovisibleKeyFrames())}     # mnBALocalForKF is set on bad neighbours too (:484)
    points, seen = [], set()
    for k in local:
        for mp in k.GetMapPointMatches():
            if mp is not None and not mp.isBad() and id(mp) not in seen:
                seen.add(id(mp))
                points.append(mp)
    fixed, marked = [], set()
    for mp in points:
        for k in sorted(mp.GetObservations(), key=lambda q: q.mnId):
            if id(k) not in in_local and id(k) not in marked:
                marked.add(id(k))                        # mnBAFixedForKF is set before the isBad test (:524-526)
                if not k.isBad():
                    fixed.append(k)
    kfs = local + fixed
    is_fixed = np.ones(len(kfs), np.uint8)
    one_fixed = False
    for i, k in enumerate(local):                        # :556-571: oneFixed is overwritten per keyframe
        one_fixed = k.mnId == 0
        is_fixed[i] = one_fixed
    if not one_fixed and not fixed:                      # :575-581
        is_fixed[0] = 1
    slot = {id(k): i for i, k in enumerate(kfs)}
    first, ekf, ecam, xy, octv, feat, total, badobs = [0], [], [], [], [], [], [], []
    for mp in points:
        obs = mp.GetObservations()
        t = b = 0
        for k in sorted(obs, key=lambda q: q.mnId):
            t += len(obs[k])
            if k.isBad():
                b += len(obs[k])
                continue
            for i in obs[k]:
                kp = k.GetKeyPoint(i)
                ekf.append(slot[id(k)])
                ecam.append(int(k.keypoint_to_cam[i]))
                xy.append([kp["x"], kp["y"]])
                octv.append(int(kp["octave"]))
                feat.append(int(i))
        first.append(len(ekf))
        total.append(t)
        badobs.append(b)
    pr = Problem([k.pose_min for k in kfs], is_fixed, len(local), [np.asarray(mp.GetWorldPos(), np.float64).reshape(-1)[:3] for mp in points] or np.zeros((0, 3)),
                 first, ekf, ecam, np.asarray(xy, np.float32).reshape(-1, 2), octv, Mc_min, cams, inv_sigma2, std_recon, total, badobs)
    return pr, local, fixed, points, np.asarray(feat, np.int32)
