"""cOptimizer::OptimizeSim3 (src/cOptimizerLoopStuff.cpp:58-264) restated statement by statement: Python floats and numpy, FP64, no GPU.  What the device
(mcs_sim3_optimize, csrc/mcs_sim3opt.hip) is held to.

Sources restated (reference tree): the set-up, both rounds and both tests src/cOptimizerLoopStuff.cpp:58-264; the vertex, cam_map1 / cam_map2 and the two
edges include/g2o_MultiCol_sim3_expmap.h:113-250; g2o::Sim3 ThirdParty/g2o/g2o/types/sim3.h:41-292 with skew (types/se3_ops.hpp:27-38); the NUMERIC Jacobian
and the quadratic form of a binary edge ThirdParty/g2o/g2o/core/base_binary_edge.hpp:55-120, 130-205; the quaternion of Eigen 3.2.10
ThirdParty/Eigen/Eigen/src/Geometry/Quaternion.h:419-474, 523-557, 655-660, 720-759, MatrixBase::cross Geometry/OrthoMethods.h:26-44 and the halving scalar
redux Core/Redux.h:77-90 (trace and norm of three numbers are a0 + (a1 + a2)).  Levenberg-Marquardt, the Huber kernel, the terminate action and
SparseOptimizer::optimize are those poseopt_model.py cites; its camera, matrix and LDL^T pieces are imported, not copied.

Every transcendental is libm's scalar function (math.atan / sin / cos / exp) through `Libm`, which can perturb each result by a seeded +-k ulp: one of the two
switches that measure how far a different but equally valid arithmetic moves the result.  The other reverses the order of every sum over the edges.

The active edges are in the order the optimiser keeps them (by internal id: e12 of correspondence 0, e21 of 0, e12 of 1, ...), so each of the 36 sums is ONE
chain over the interleaved edges.

Which camera an edge projects with.  e12's point vertex is vPoint2, whose ptID is i2 (:149, :167), and cam_map1 looks ptID up in keypoint_to_cam1; e21's point
vertex is vPoint1 with ptID i (:140, :185), looked up in keypoint_to_cam2.  The reference therefore projects e12 with KF1's camera of feature i2 and e21 with
KF2's camera of feature i — the indices are crossed.  The model takes cam[i][2] as given; keyframe_problem() below builds it crossed, as the reference does.
"""
import math

import numpy as np

import poseopt_model as PM
from poseopt_model import (STOP_GAIN, STOP_ITERATIONS, STOP_NBAD, STOP_NOT_RUN, STOP_TRIALS, inv_mat, ldlt6, sum_margin, threshold_margin,  # noqa: F401
                           world_to_img)

DBL_MAX = PM.DBL_MAX
SIM3_OK, SIM3_NONFINITE = 0, 1
EPS = 0.00001
# ULP bounds of the device's double-precision functions.  No published figure for ocml's was at hand, so these are the OpenCL full-profile bounds
# (OpenCL C specification, "Relative error as ULPs", double precision): atan <= 5, sin <= 4, cos <= 4, exp <= 3.
ULP = dict(atan=5, sin=4, cos=4, exp=3)


class Libm:
    """libm's scalar functions; seed is not None: every result moved by a uniformly drawn integer in [-k, k] ulp (k per function, ULP)"""

    def __init__(self, seed=None, k=None):
        self.rng = None if seed is None else np.random.default_rng(seed)
        self.k = dict(ULP if k is None else k)

    def _p(self, name, r):
        if self.rng is None or not math.isfinite(r):
            return r
        return r + float(self.rng.integers(-self.k[name], self.k[name] + 1)) * float(np.spacing(abs(r)))

    def sin(self, x):
        return self._p("sin", math.sin(x))

    def cos(self, x):
        return self._p("cos", math.cos(x))

    def exp(self, x):
        try:
            return self._p("exp", math.exp(x))
        except OverflowError:
            return math.inf

    def atan(self, a):
        r = np.array([math.atan(v) for v in a], np.float64)
        if self.rng is not None and len(r):
            k = self.k["atan"]
            with np.errstate(invalid="ignore"):
                r = np.where(np.isfinite(r), r + self.rng.integers(-k, k + 1, len(r)) * np.spacing(np.abs(r)), r)
        return r


EXACT = Libm()


# ---------------------------------------------------------------------------------------------- Eigen's quaternion; q = [x, y, z, w] (coeffs() order)
def quat_from_mat(R, margins=None):   # Quaternion.h:720-759
    R = [[float(R[i][j]) for j in range(3)] for i in range(3)]
    t = R[0][0] + (R[1][1] + R[2][2])
    if margins is not None:
        margins.append(abs(t))
    q = [0.0] * 4
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2][1] - R[1][2]) * t
        q[1] = (R[0][2] - R[2][0]) * t
        q[2] = (R[1][0] - R[0][1]) * t
    else:
        i = 0
        if R[1][1] > R[0][0]:
            i = 1
        if R[2][2] > R[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        v = R[i][i] - R[j][j] - R[k][k] + 1.0
        t = math.sqrt(v) if v >= 0 else math.nan
        q[i] = 0.5 * t
        t = float(np.float64(0.5) / np.float64(t))
        q[3] = (R[k][j] - R[j][k]) * t
        q[j] = (R[j][i] + R[i][j]) * t
        q[k] = (R[k][i] + R[i][k]) * t
    return q


def quat_mul(a, b):   # :419-430, the generic scalar form
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def cross3(a, b):   # OrthoMethods.h:26-44; a: three scalars, b: three scalars or three arrays
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rotate(q, v):   # _transformVector, :462-474; v: three scalars or three arrays
    uv = cross3(q, v)
    uv = [c + c for c in uv]
    c = cross3(q, uv)
    return [v[k] + q[3] * uv[k] + c[k] for k in range(3)]


def quat_conj(q):   # :655-660
    return [-q[0], -q[1], -q[2], q[3]]


def quat_to_mat(q):   # :523-557
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


# ---------------------------------------------------------------------------------------------- g2o::Sim3 as (q, t, s)
def sim3_from_rts(R, t, s, margins=None):   # sim3.h:64-67
    return (quat_from_mat(np.asarray(R, np.float64).reshape(3, 3), margins), [float(v) for v in t], float(s))


def sim3_exp(u, lm=EXACT, margins=None, normalize=False, info=None):
    """Sim3(const Vector7d&), sim3.h:70-142.  info (a list): gets the branch, 2 * (|sigma| >= eps) + (theta >= eps)."""
    w = [float(u[0]), float(u[1]), float(u[2])]
    ups = [float(u[3]), float(u[4]), float(u[5])]
    sigma = float(u[6])
    theta = math.sqrt(w[0] * w[0] + (w[1] * w[1] + w[2] * w[2]))
    Om = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    s = lm.exp(sigma)
    Om2 = [[(Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j]) + Om[i][2] * Om[2][j] for j in range(3)] for i in range(3)]
    eye = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    if margins is not None:
        margins.append(abs(abs(sigma) - EPS) / EPS)
        margins.append(abs(theta - EPS) / EPS)
    if info is not None:
        info.append((0 if abs(sigma) < EPS else 2) + (0 if theta < EPS else 1))
    with np.errstate(all="ignore"):
        f = np.float64
        if abs(sigma) < EPS:
            C = 1.0
            if theta < EPS:
                A, B, series = 1. / 2., 1. / 6., True
            else:
                theta2 = theta * theta
                A = float((1 - f(lm.cos(theta))) / f(theta2))
                B = float((theta - f(lm.sin(theta))) / f(theta2 * theta))
                series = False
        else:
            C = float(f(s - 1) / f(sigma))
            if theta < EPS:
                sigma2 = sigma * sigma
                A = float(f((sigma - 1) * s + 1) / f(sigma2))
                B = float(f((0.5 * sigma2 - sigma + 1) * s) / f(sigma2 * sigma))
                series = True
            else:
                series = False
                a = s * lm.sin(theta)
                b = s * lm.cos(theta)
                theta2 = theta * theta
                sigma2 = sigma * sigma
                c = theta2 + sigma2
                A = float(f(a * sigma + (1 - b) * theta) / f(theta * c))
                B = float(f((C - float(f((b - 1) * sigma + a * theta) / f(c))) * 1.) / f(theta2))
        if series:
            R = [[(eye[i][j] + Om[i][j]) + Om2[i][j] for j in range(3)] for i in range(3)]
        else:
            ca = float(f(lm.sin(theta)) / f(theta))
            cb = float(f(1 - lm.cos(theta)) / f(theta * theta))
            R = [[(eye[i][j] + ca * Om[i][j]) + cb * Om2[i][j] for j in range(3)] for i in range(3)]
        q = quat_from_mat(R, margins)
        if normalize:
            nq = math.sqrt(sum(c * c for c in q))
            q = [c / nq for c in q]
        W = [[(A * Om[i][j] + B * Om2[i][j]) + C * eye[i][j] for j in range(3)] for i in range(3)]
        t = [(W[i][0] * ups[0] + W[i][1] * ups[1]) + W[i][2] * ups[2] for i in range(3)]
    return (q, t, s)


def sim3_map(S, x):   # :144-146; x: three scalars or three arrays
    q, t, s = S
    v = quat_rotate(q, x)
    return [s * v[k] + t[k] for k in range(3)]


def sim3_inverse(S):   # :233-236
    q, t, s = S
    with np.errstate(all="ignore"):
        f = float(np.float64(-1.) / np.float64(s))
        qi = quat_conj(q)
        return (qi, quat_rotate(qi, [f * t[0], f * t[1], f * t[2]]), float(np.float64(1.) / np.float64(s)))


def sim3_mul(a, b):   # :266-272
    v = quat_rotate(a[0], b[1])
    return (quat_mul(a[0], b[0]), [a[2] * v[k] + a[1][k] for k in range(3)], a[2] * b[2])


def sim3_vec(S):   # operator[] order: qx qy qz qw tx ty tz s
    return np.array(list(S[0]) + list(S[1]) + [S[2]], np.float64)


# ---------------------------------------------------------------------------------------------- the problem
class Problem:
    """One candidate as OptimizeSim3 reads it, in the order its loop keeps the correspondences.  Xw [n][2][3], cam [n][2], obs [n][2][2] (float32 values), w [n][2]
    (the two information factors AS GIVEN: the GetSigma2 quirk lives in whoever builds them), Mc [nr][4][4], cams (dicts), Mt_inv [2][4][4]."""

    def __init__(self, Xw, cam, obs, w, Mc, cams, Mt_inv, R12, t12, s12, std_sim=4.0):
        self.Xw = np.asarray(Xw, np.float64).reshape(-1, 2, 3)
        self.cam = np.asarray(cam, np.int32).reshape(-1, 2)
        self.obs = np.asarray(obs, np.float64).reshape(-1, 2, 2)
        self.w = np.asarray(w, np.float64).reshape(-1, 2)
        self.Mc = np.asarray(Mc, np.float64).reshape(-1, 4, 4)
        self.cams = cams
        self.Mt_inv = np.asarray(Mt_inv, np.float64).reshape(2, 4, 4)
        self.R12, self.t12, self.s12 = np.asarray(R12, np.float64).reshape(3, 3).copy(), np.asarray(t12, np.float64).copy(), float(s12)
        self.std_sim = float(std_sim)
        self.n = len(self.Xw)

    def pairs(self):
        """index of every correspondence that gives an edge pair: both cameras inside the rig (the device kind's guard; the host kind refuses the call)"""
        nr = len(self.Mc)
        return np.nonzero(((self.cam >= 0) & (self.cam < nr)).all(1))[0]


def _hom_rows(M, X):   # rows 0..2 of Matx44d * Vec4d(X, 1.0): s = 0; s += M(i,k) * p(k) in increasing k
    return [(((0.0 + M[r, 0] * X[0]) + M[r, 1] * X[1]) + M[r, 2] * X[2]) + M[r, 3] * 1.0 for r in range(3)]


def rig_points(pr, idx):
    """invMat(M_t) * (Xw, 1) of both points of the correspondences idx (:113-146): P1 in rig 1, P2 in rig 2, each three arrays"""
    X1, X2 = pr.Xw[idx, 0], pr.Xw[idx, 1]
    return _hom_rows(pr.Mt_inv[0], [X1[:, 0], X1[:, 1], X1[:, 2]]), _hom_rows(pr.Mt_inv[1], [X2[:, 0], X2[:, 1], X2[:, 2]])


def cam_map(pr, inv_Mc, cam, v, lm):
    """cam_map1 / cam_map2 (g2o_MultiCol_sim3_expmap.h:141-161): invMat(M_c[cam]) * (v, 1), then WorldToImg.  -> u, v arrays"""
    u, vv = np.zeros(len(cam)), np.zeros(len(cam))
    for c in np.unique(cam):
        m = cam == c
        p = _hom_rows(inv_Mc[c], [v[0][m], v[1][m], v[2][m]])
        u[m], vv[m] = _world_to_img(pr.cams[c], p[0], p[1], p[2], lm)
    return u, vv


def _world_to_img(cam, x, y, z, lm):   # poseopt_model.world_to_img with the atan of `lm`
    if lm is EXACT:
        return world_to_img(cam, x, y, z)
    norm = np.sqrt(x * x + y * y)
    norm = np.where(norm == 0.0, 1e-14, norm)
    theta = lm.atan(-z / norm)
    rho = PM._horner(cam["invP"], theta)
    uu = x / norm * rho
    vv = y / norm * rho
    return uu * cam["c"] + vv * cam["d"] + cam["u0"], uu * cam["e"] + vv + cam["v0"]


def errors(pr, S, Sinv, idx, P1, P2, inv_Mc, lm=EXACT):
    """[m][2 edges][2]: e12 = obs1 - cam_map1(S.map(P2)), e21 = obs2 - cam_map2(S.inverse().map(P1)) (computeError of both edge classes)"""
    e = np.zeros((len(idx), 2, 2))
    u, v = cam_map(pr, inv_Mc, pr.cam[idx, 0], sim3_map(S, P2), lm)
    e[:, 0, 0], e[:, 0, 1] = pr.obs[idx, 0, 0] - u, pr.obs[idx, 0, 1] - v
    u, v = cam_map(pr, inv_Mc, pr.cam[idx, 1], sim3_map(Sinv, P1), lm)
    e[:, 1, 0], e[:, 1, 1] = pr.obs[idx, 1, 0] - u, pr.obs[idx, 1, 1] - v
    return e


DELTA = 1e-9   # base_binary_edge.hpp:147


def numeric_jacobian(pr, S, idx, P1, P2, inv_Mc, lm=EXACT, margins=None, normalize=False):
    """linearizeOplus (base_binary_edge.hpp:130-205) of both edges: column d = (1 / (2 delta)) * (e(Sim3(+delta e_d) * S) - e(Sim3(-delta e_d) * S)).  [m][2][2][7]"""
    scalar = 1.0 / (2 * DELTA)
    J = np.zeros((len(idx), 2, 2, 7))
    for d in range(7):
        add = [0.0] * 7
        add[d] = DELTA
        Sp = sim3_mul(sim3_exp(add, lm, margins, normalize), S)
        bak = errors(pr, Sp, sim3_inverse(Sp), idx, P1, P2, inv_Mc, lm)
        add[d] = -DELTA
        Sm = sim3_mul(sim3_exp(add, lm, margins, normalize), S)
        bak = bak - errors(pr, Sm, sim3_inverse(Sm), idx, P1, P2, inv_Mc, lm)
        J[:, :, :, d] = scalar * bak
    return J


class Result:
    pass


def optimize(pr, reverse=False, fix=(), lm=EXACT):
    with np.errstate(all="ignore"):
        return _optimize(pr, reverse, set(fix), lm)


def _optimize(pr, reverse, fix, lm):
    """OptimizeSim3 on one problem.  reverse: every sum over the edges runs in reversed order.  lm: the transcendental functions.
    fix: quirks "repaired", for the tests that show each one matters: both_edges (a correspondence is bad only if BOTH edges exceed the bound), always_5 (the
    second round runs 5 iterations whatever nBad), write_back (the return-0 path stores the estimate), clear_stop (the stop flag is cleared before round two),
    normalize (the quaternion of every exponential is normalised), inverse_w2 (w[:, 1] is inverted: GetInvSigma2 for the second edge)."""
    res = Result()
    idx = pr.pairs()
    nC = len(idx)
    margins = []
    S = sim3_from_rts(pr.R12, pr.t12, pr.s12, margins)
    S_in = S
    res.status, res.keep = SIM3_OK, np.ones(pr.n, np.uint8)
    res.iters, res.stop, res.trials = [0, 0], [STOP_NOT_RUN, STOP_NOT_RUN], np.zeros((2, 10), np.int32)
    res.lam, res.chi2, res.n_inliers, res.n_corr, res.n_bad1 = 0.0, 0.0, 0, nC, 0
    res.trace, res.branches = [], []
    w_all = pr.w[idx].copy()
    if "inverse_w2" in fix:
        w_all[:, 1] = 1.0 / w_all[:, 1]
    delta = 1.345 * pr.std_sim
    dsqr = delta * delta   # deltaHuber2 (:110) is the same product
    inv_Mc = [inv_mat(M) for M in pr.Mc]
    P1, P2 = rig_points(pr, idx)
    normalize = "normalize" in fix

    def finish(S_out, n_in):
        res.S12, res.R12 = sim3_vec(S_out), quat_to_mat(S_out[0])
        res.n_inliers = n_in
        res.margin = (0.0 if any(math.isnan(v) for v in margins) else min(margins)) if margins else math.inf
        return res

    if nC == 0:   # optimize() returns -1 before its loop (no vertex to optimise); 0 - 0 < 3
        return finish(S_in, 0)

    def sub(P, m):
        return [P[0][m], P[1][m], P[2][m]]

    def ssum(a):
        a = a[::-1] if reverse else a
        return np.cumsum(a, axis=0)[-1]

    def chi2_of(e, w):   # _error.dot(information() * _error), information = I2x2 * w
        return e[..., 0] * (w * e[..., 0]) + e[..., 1] * (w * e[..., 1])

    def robust(c2, track=True):
        inl = c2 <= dsqr
        if track and c2.size:
            margins.append(threshold_margin(c2, dsqr))
        sq = np.sqrt(np.where(inl, 1.0, c2))
        return np.where(inl, c2, 2 * sq * delta - dsqr), np.where(inl, 1.0, delta / sq)

    alive = np.ones(nC, bool)   # the correspondences whose edges are still in the graph
    state = {"S": S}

    def err_at(Sx, act):
        return errors(pr, Sx, sim3_inverse(Sx), idx[act], sub(P1, act), sub(P2, act), inv_Mc, lm)

    def robust_chi2(e, w):
        return float(ssum(robust(chi2_of(e, w).reshape(-1))[0]))

    stop_flag = False
    last_chi = 0.0
    lam, ni = -1.0, 2.0
    e_cur = None
    for rnd in range(2):
        if rnd == 1:
            res.n_bad1 = int((~alive).sum())
            if nC - res.n_bad1 < 3:   # :234-235: return 0, g2oS12 NOT written back, the matches stay nulled
                res.keep[idx[~alive]] = 0
                res.lam, res.chi2 = lam, last_chi
                return finish(state["S"] if "write_back" in fix else S_in, 0)
            if "clear_stop" in fix:
                stop_flag = False
        max_it = 5 if rnd == 0 or res.n_bad1 == 0 or "always_5" in fix else 10
        act = alive.copy()
        w = w_all[act]
        x = np.zeros(7)
        result_ok = True
        it = 0
        stop = STOP_NOT_RUN if stop_flag else STOP_ITERATIONS
        lm_bad = 0
        while it < max_it and not stop_flag and result_ok:
            # ---- OptimizationAlgorithmLevenberg::solve(it)
            Sc = state["S"]
            e = err_at(Sc, act)
            J = numeric_jacobian(pr, Sc, idx[act], sub(P1, act), sub(P2, act), inv_Mc, lm, margins, normalize)
            first = rnd == 0 and it == 0
            c2 = chi2_of(e, w)
            rho0, rho1 = robust(c2.reshape(-1))
            currentChi = float(ssum(rho0))
            iniChi = currentChi
            # constructQuadraticForm, robust branch (base_binary_edge.hpp:91-113): omega_r = -(omega * e); omega_r *= rho[1]; b += B^T omega_r;
            # A += (B^T * weightedOmega) * B with weightedOmega = rho[1] * omega
            m = e.shape[0] * 2
            ef, Jf, wf = e.reshape(m, 2), J.reshape(m, 2, 7), w.reshape(m)
            rw = rho1 * wf
            or0, or1 = (-(wf * ef[:, 0])) * rho1, (-(wf * ef[:, 1])) * rho1
            H = np.zeros((7, 7))
            for a in range(7):
                for c in range(a, 7):
                    H[a, c] = H[c, a] = ssum((Jf[:, 0, a] * rw) * Jf[:, 0, c] + (Jf[:, 1, a] * rw) * Jf[:, 1, c])
            b = np.array([ssum(Jf[:, 0, a] * or0 + Jf[:, 1, a] * or1) for a in range(7)])
            if first and not (np.isfinite(ef).all() and np.isfinite(Jf).all() and np.isfinite(wf).all() and math.isfinite(delta) and math.isfinite(dsqr)
                              and np.isfinite(H).all() and np.isfinite(b).all() and math.isfinite(currentChi)):
                res.status = SIM3_NONFINITE   # the project's choice: a status, nothing changed, every correspondence counted
                res.margin = math.inf
                res.S12, res.R12, res.n_inliers = sim3_vec(S_in), quat_to_mat(S_in[0]), nC
                return res
            if it == 0:
                lam, ni, lm_bad = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0, 0
            rho, qmax = 0.0, 0
            tr = dict(round=rnd, it=it, trials=[], lam=[], rho=[])
            while True:
                backup = state["S"]                                  # push
                ok2, sol = ldlt6(H + lam * np.eye(7), b)
                if ok2:
                    x = sol
                info = []
                upd = sim3_exp(x, lm, margins, normalize, info)      # oplusImpl: Sim3(update) * estimate, with the stale x after a failed solve
                res.branches.append(info[0])
                state["S"] = sim3_mul(upd, state["S"])
                e_try = err_at(state["S"], act)
                tempChi = robust_chi2(e_try, w)
                if not ok2:
                    tempChi = DBL_MAX
                rho = currentChi - tempChi
                scale = 0.0
                for j in range(7):
                    scale += x[j] * (lam * x[j] + b[j])
                scale += 1e-3
                if not ok2 and not math.isnan(scale):
                    margins.append(abs(scale) / max(sum(abs(x[j] * (lam * x[j] + b[j])) for j in range(7)) + 1e-3, 1e-300))
                rho = float(np.float64(rho) / np.float64(scale))
                margins.append(sum_margin(currentChi, tempChi))
                tr["rho"].append(rho)
                if rho > 0 and math.isfinite(tempChi):
                    try:
                        alpha = 1.0 - (2 * rho - 1) ** 3
                    except OverflowError:
                        alpha = -math.inf
                    alpha = min(alpha, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    currentChi = tempChi
                else:
                    lam *= ni
                    ni *= 2
                    state["S"] = backup                              # pop
                tr["lam"].append(lam)
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
            # ---- postIteration(it): the terminate action recomputes the active errors at the current estimate, then reads the robust chi2
            e_cur = err_at(state["S"], act)
            cur = robust_chi2(e_cur, w)
            gain = math.nan
            if it == 0:
                last_chi = cur
            else:
                gain = float(np.float64(last_chi - cur) / np.float64(cur))
                margins.append(abs(last_chi - cur) / max(abs(cur), 1e-300) * 1e3)
                margins.append(abs(gain - 1e-6) / 1e-6)
                last_chi = cur
                if gain >= 0 and gain < 1e-6:
                    stop_flag = True
                    if result_ok:
                        stop = STOP_GAIN
            tr["trials"], tr["gain"] = qmax, gain
            res.trace.append(tr)
            it += 1
        res.iters[rnd], res.stop[rnd] = it, stop
        # ---- the test behind this round (:206-226, :241-257): every edge's stored error is that of the current estimate (see poseopt_model's docstring);
        # a round that did not run leaves the errors of the round before
        e_cur = err_at(state["S"], act)
        c2 = chi2_of(e_cur, w)                                       # [m][2]
        if c2.size:
            margins.append(threshold_margin(c2.reshape(-1), dsqr))
        bad = (c2[:, 0] > dsqr) & (c2[:, 1] > dsqr) if "both_edges" in fix else (c2[:, 0] > dsqr) | (c2[:, 1] > dsqr)
        where = np.nonzero(act)[0]
        alive[where[bad]] = False
    res.keep[idx[~alive]] = 0
    res.lam, res.chi2 = lam, last_chi
    return finish(state["S"], int(alive.sum()))


def rel_spread(a, b):
    """largest relative difference of two S12 vectors: per component against max(|component|, 1) — a quaternion or translation entry near zero is held
    absolutely, at the scale of the unit quaternion"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1.0)))


# ---------------------------------------------------------------------------------------------- from keyframes (what frontend.OptimizeSim3 and the facade do)
def keyframe_problem(pKF1, pKF2, vpMatches1, R12, t12, s12, Mc, cams, std_sim=4.0, fix=()):
    """The pointer filtering of :117-199 -> (Problem, the feature index of each correspondence).  fix: inverse_w2 passes GetInvSigma2 for the second edge;
    straight_cams looks each edge's camera up by its own keyframe's feature (the reference crosses them, see the module docstring)."""
    vp1 = pKF1.GetMapPointMatches()
    Xw, cam, obs, w, at = [], [], [], [], []
    for i, mp2 in enumerate(vpMatches1):
        if mp2 is None:
            continue
        mp1 = vp1[i]
        idx2 = mp2.GetIndexInKeyFrame(pKF2)
        if mp1 is None or not idx2 or mp1.isBad() or mp2.isBad() or idx2[0] < 0:   # a match pKF2 does not observe: skipped like i2 < 0
            continue
        i2 = idx2[0]
        k1, k2 = pKF1.GetKeyPoint(i), pKF2.GetKeyPoint(i2)
        Xw.append([np.asarray(mp1.GetWorldPos(), np.float64)[:3], np.asarray(mp2.GetWorldPos(), np.float64)[:3]])
        if "straight_cams" in fix:
            cam.append([int(pKF1.keypoint_to_cam[i]), int(pKF2.keypoint_to_cam[i2])])
        else:
            cam.append([int(pKF1.keypoint_to_cam[i2]), int(pKF2.keypoint_to_cam[i])])
        obs.append([[float(k1["x"]), float(k1["y"])], [float(k2["x"]), float(k2["y"])]])
        w.append([pKF1.GetInvSigma2(int(k1["octave"])), pKF2.GetInvSigma2(int(k2["octave"])) if "inverse_w2" in fix else pKF2.GetSigma2(int(k2["octave"]))])
        at.append(i)
    Mt_inv = [inv_mat(np.asarray(pKF1.camSystem.Get_M_t(), np.float64)), inv_mat(np.asarray(pKF2.camSystem.Get_M_t(), np.float64))]
    return Problem(np.zeros((0, 2, 3)) if not Xw else Xw, np.zeros((0, 2), np.int32) if not cam else cam, np.zeros((0, 2, 2)) if not obs else obs,
                   np.zeros((0, 2)) if not w else w, Mc, cams, Mt_inv, R12, t12, s12, std_sim), at
