"""cOptimizer::OptimizeEssentialGraph (src/cOptimizerLoopStuff.cpp:267-513) restated statement by statement in numpy: FP64, no GPU, vectorised over the edges
(a Sim3 is the triple (q [..., 4], t [..., 3], s [...]) in operator[] order qx qy qz qw tx ty tz s).  What the device (mcs_optimize_essential_graph,
csrc/mcs_essgraph.hip) and the header (csrc/mcs_sim3g.h: sim3_log, lu3_solve, sim3_edge_error) are held to.

Sources restated (reference tree): the vertices, the measurements, the run and the write-back src/cOptimizerLoopStuff.cpp:267-513; the vertex and the edge
include/g2o_MultiCol_sim3_expmap.h:47-111 (simpleVertexSim3Expmap's constructor, src/g2o_MultiCol_sim3_expmap.cpp, leaves _fix_scale = false, so the scale
is a free seventh coordinate); g2o::Sim3 ThirdParty/g2o/g2o/types/sim3.h:41-292 with deltaR and skew (types/se3_ops.hpp:27-49); the NUMERIC Jacobian and the
quadratic form of a binary edge core/base_binary_edge.hpp:55-120, 130-205; Levenberg-Marquardt core/optimization_algorithm_levenberg.cpp:60-189 with
setUserLambdaInit(1e-6); the terminate action core/sparse_optimizer_terminate_action.cpp:24-57; Eigen 3.2.10's quaternion (Geometry/Quaternion.h) and its
3x3 PartialPivLU (LU/PartialPivLU.h:245-287, Core/SolveTriangular.h).

The iteration count.  optimize(20) numbers its iterations 0..19 and calls the action behind each.  The action stores chi2 at iteration 0, tests the gain at
1..14 and, at the first iteration with `iteration >= 15`, sets the stop flag without a test.  Iteration 15 has run by then: a run that neither the gain
test nor Levenberg-Marquardt ends has SIXTEEN iterations (0..15), stop reason STOP_CAP.

What replaces the reference's linear solver is DESIGN.md 7's: a dense, unpivoted LDL^T of H + lambda I in the order of the vertices, failing on a pivot that
is zero or not finite.  Column by column it is the arithmetic of the device's blocked factorisation (the panel solve and the trailing update subtract
(l_rj * l_kj) * d_j in increasing j from each entry); above `kExactSolve` unknowns this model gathers the trailing updates that reach a panel into ONE matrix
product, whose inner order numpy does not promise: that difference is of the size the `reverse` switch measures.

Every transcendental is libm's scalar function through `Libm`, which can move each result by a seeded +-k ulp; `reverse` reverses every sum over the edges
(the blocks of H, b, chi2) and the inner sums of the solve.  The two switches measure how far an equally valid arithmetic moves the result.
The blocks of H and b are summed in edge order on the device as here.  chi2 and the terms of computeScale are NOT: the device sums them thread-strided and
then in a fixed tree (k_eg_reduce), a third order next to this model's two; that difference is part of what the derived tolerance allows.
"""
import math

import numpy as np

from poseopt_model import inv_mat, sum_margin  # noqa: F401

DBL_MAX = float(np.finfo(np.float64).max)
EG_OK, EG_NONFINITE, EG_NO_FREE_VERTEX, EG_FAILED = 0, 1, 2, 3
STOP_ITERATIONS, STOP_GAIN, STOP_TRIALS, STOP_NBAD, STOP_NOT_RUN, STOP_CAP = 0, 1, 2, 3, 4, 5
EPS = 0.00001
DELTA = 1e-9
PANEL = 32
kExactSolve = 160
# ULP bounds of the device's double-precision functions.  No published figure for ocml's was at hand, so these are the OpenCL full-profile bounds (OpenCL C
# specification, "Relative error as ULPs", double precision): acos <= 4, sin <= 4, cos <= 4, exp <= 3, log <= 3.
ULP = dict(acos=4, sin=4, cos=4, exp=3, log=3)


class Libm:
    """libm's scalar functions over arrays, element by element (numpy's vector functions are other implementations); seed is not None: every result moved by
    a uniformly drawn integer in [-k, k] ulp (k per function, ULP)"""

    def __init__(self, seed=None):
        self.rng = None if seed is None else np.random.default_rng(seed)

    def _f(self, name, fn, x):
        x = np.asarray(x, np.float64)
        r = np.array([fn(float(v)) for v in x.ravel()], np.float64).reshape(x.shape)
        if self.rng is not None and r.size:
            k = ULP[name]
            with np.errstate(invalid="ignore"):
                r = np.where(np.isfinite(r), r + self.rng.integers(-k, k + 1, r.shape) * np.spacing(np.abs(r)), r)
        return r

    @staticmethod
    def _safe(fn):
        def g(v):
            try:
                return fn(v)
            except (ValueError, OverflowError):
                return math.nan if not (fn is math.exp and v > 0) else math.inf
        return g

    def sin(self, x):
        return self._f("sin", self._safe(math.sin), x)

    def cos(self, x):
        return self._f("cos", self._safe(math.cos), x)

    def exp(self, x):
        return self._f("exp", self._safe(math.exp), x)

    def acos(self, x):
        return self._f("acos", self._safe(math.acos), x)

    def log(self, x):
        def lg(v):
            if v == 0.0:
                return -math.inf
            return math.log(v) if v > 0 else math.nan
        return self._f("log", lg, x)


EXACT = Libm()


class Margins:
    """the smallest distance of every kind of decision from its edge over a run (relative where the edge is not 0)"""

    def __init__(self):
        self.m = dict(rho=math.inf, gain=math.inf, branch=math.inf, quat=math.inf, pivot=math.inf)

    def add(self, kind, values):
        v = np.asarray(values, np.float64)
        if v.size:
            self.m[kind] = min(self.m[kind], float(np.min(np.where(np.isnan(v), 0.0, v))))

    def least(self):
        return min(self.m.values())


# ---------------------------------------------------------------------------------------------- Eigen's quaternion, vectorised; q = [..., (x, y, z, w)]
def _v(a, k):
    return a[..., k]


def quat_from_mat(R, mg=None):   # Quaternion.h:720-759; R [..., 9] row-major
    R = np.asarray(R, np.float64)
    m = lambda i, j: R[..., 3 * i + j]   # noqa: E731
    tr = m(0, 0) + (m(1, 1) + m(2, 2))
    pos = tr > 0.0
    with np.errstate(all="ignore"):
        t = np.sqrt(tr + 1.0)
        qa = np.stack([(m(2, 1) - m(1, 2)) * (0.5 / t), (m(0, 2) - m(2, 0)) * (0.5 / t), (m(1, 0) - m(0, 1)) * (0.5 / t), 0.5 * t], -1)
        out = qa.copy()
        i1 = m(1, 1) > m(0, 0)
        dmax = np.where(i1, m(1, 1), m(0, 0))
        i2 = m(2, 2) > dmax
        idx = np.where(i2, 2, np.where(i1, 1, 0))
        if mg is not None:
            mg.add("quat", np.abs(tr))
            if (~pos).any():
                mg.add("quat", np.where(pos, np.inf, np.minimum(np.abs(m(1, 1) - m(0, 0)), np.abs(m(2, 2) - dmax))))
        for i in range(3):
            sel = (~pos) & (idx == i)
            if not sel.any():
                continue
            j, k = (i + 1) % 3, (i + 2) % 3
            v = m(i, i) - m(j, j) - m(k, k) + 1.0
            t = np.sqrt(v)
            f = 0.5 / t
            qb = np.zeros(R.shape[:-1] + (4,))
            qb[..., i] = 0.5 * t
            qb[..., 3] = (m(k, j) - m(j, k)) * f
            qb[..., j] = (m(j, i) + m(i, j)) * f
            qb[..., k] = (m(k, i) + m(i, k)) * f
            out = np.where(sel[..., None], qb, out)
    return out


def quat_mul(a, b):   # :419-430, the generic scalar form
    ax, ay, az, aw = (_v(a, k) for k in range(4))
    bx, by, bz, bw = (_v(b, k) for k in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], -1)


def cross3(a, b):   # OrthoMethods.h:26-44
    return np.stack([_v(a, 1) * _v(b, 2) - _v(a, 2) * _v(b, 1), _v(a, 2) * _v(b, 0) - _v(a, 0) * _v(b, 2), _v(a, 0) * _v(b, 1) - _v(a, 1) * _v(b, 0)], -1)


def quat_rotate(q, v):   # _transformVector, :462-474
    uv = cross3(q, v)
    uv = uv + uv
    c = cross3(q, uv)
    return v + q[..., 3:4] * uv + c


def quat_conj(q):   # :655-660
    return q * np.array([-1.0, -1.0, -1.0, 1.0])


def quat_to_mat(q):   # :523-557 -> [..., 9] row-major
    x, y, z, w = (_v(q, k) for k in range(4))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)], -1)


# ---------------------------------------------------------------------------------------------- g2o::Sim3
def sim3_of(v):
    v = np.asarray(v, np.float64)
    return (v[..., :4].copy(), v[..., 4:7].copy(), v[..., 7].copy())


def sim3_vec(S):
    return np.concatenate([S[0], S[1], S[2][..., None]], -1)


def sim3_from_rts(R, t, s, mg=None):   # sim3.h:64-67
    return (quat_from_mat(np.asarray(R, np.float64).reshape(np.shape(R)[:-1] + (9,)) if np.shape(R)[-1] == 9 else np.asarray(R, np.float64).reshape(
        np.shape(R)[:-2] + (9,)), mg), np.asarray(t, np.float64).copy(), np.asarray(s, np.float64).copy())


def sim3_mul(a, b):   # :266-272
    return (quat_mul(a[0], b[0]), a[2][..., None] * quat_rotate(a[0], b[1]) + a[1], a[2] * b[2])


def sim3_inverse(S):   # :233-236
    qc = quat_conj(S[0])
    return (qc, quat_rotate(qc, (-1. / S[2])[..., None] * S[1]), 1. / S[2])


def sim3_map(S, x):   # :144-146
    return S[2][..., None] * quat_rotate(S[0], x) + S[1]


def _skew_parts(w):
    z = np.zeros_like(w[..., 0])
    Om = np.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1)
    return Om


def _mat3_mul(A, B):   # [..., 9] x [..., 9], sums in increasing k
    out = []
    for i in range(3):
        for j in range(3):
            a = A[..., 3 * i] * B[..., j]
            a = a + A[..., 3 * i + 1] * B[..., 3 + j]
            a = a + A[..., 3 * i + 2] * B[..., 6 + j]
            out.append(a)
    return np.stack(out, -1)


_I9 = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])


def sim3_exp(u, lm=EXACT, mg=None, info=None):   # Sim3(const Vector7d&), :70-142; u [..., 7]
    u = np.asarray(u, np.float64)
    w, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    with np.errstate(all="ignore"):
        theta = np.sqrt(w[..., 0] * w[..., 0] + (w[..., 1] * w[..., 1] + w[..., 2] * w[..., 2]))
        Om = _skew_parts(w)
        Om2 = _mat3_mul(Om, Om)
        s = lm.exp(sigma)
        small_s, small_t = np.abs(sigma) < EPS, theta < EPS
        if mg is not None:
            mg.add("branch", np.abs(np.abs(sigma) - EPS) / EPS)
            mg.add("branch", np.abs(theta - EPS) / EPS)
        if info is not None:
            info.append(np.where(small_s, 0, 2) + np.where(small_t, 0, 1))
        sn, cs = lm.sin(theta), lm.cos(theta)
        theta2, sigma2 = theta * theta, sigma * sigma
        A00, B00 = 0.5, 1. / 6.
        A01, B01 = (1 - cs) / theta2, (theta - sn) / (theta2 * theta)
        C1 = (s - 1) / sigma
        A10, B10 = ((sigma - 1) * s + 1) / sigma2, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C1 - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        A = np.where(small_s, np.where(small_t, A00, A01), np.where(small_t, A10, A11))
        B = np.where(small_s, np.where(small_t, B00, B01), np.where(small_t, B10, B11))
        C = np.where(small_s, 1.0, C1)
        Rs = (_I9 + Om) + Om2
        ca, cb = sn / theta, (1 - cs) / (theta * theta)
        Rr = (_I9 + ca[..., None] * Om) + cb[..., None] * Om2
        R = np.where(small_t[..., None], Rs, Rr)
        q = quat_from_mat(R, mg)
        W = (A[..., None] * Om + B[..., None] * Om2) + C[..., None] * _I9
        t = []
        for i in range(3):
            acc = W[..., 3 * i] * ups[..., 0]
            acc = acc + W[..., 3 * i + 1] * ups[..., 1]
            acc = acc + W[..., 3 * i + 2] * ups[..., 2]
            t.append(acc)
    return (q, np.stack(t, -1), s)


def lu3_solve(W, b, mg=None, info=None):   # PartialPivLU of a 3x3 and its solve, as csrc/mcs_sim3g.h states it; W [..., 9], b [..., 3]
    W = [[W[..., 3 * i + j].copy() for j in range(3)] for i in range(3)]
    y = [b[..., k].copy() for k in range(3)]
    piv_info = []
    with np.errstate(all="ignore"):
        for k in range(3):
            piv = np.full(W[0][0].shape, k)
            big = np.abs(W[k][k])
            for r in range(k + 1, 3):
                g = np.abs(W[r][k]) > big
                big = np.where(g, np.abs(W[r][k]), big)
                piv = np.where(g, r, piv)
            if k < 2:
                piv_info.append(piv)
                if mg is not None:   # how far the chosen pivot is from each other candidate, relative to the pivot
                    others = [np.abs(big - np.abs(W[r][k])) / np.where(big > 0, big, 1.0) for r in range(k, 3)]
                    cand = np.stack([np.where(piv == r, np.inf, others[r - k]) for r in range(k, 3)], -1)
                    mg.add("pivot", np.min(cand, -1))
            for r in range(k + 1, 3):
                sw = piv == r
                for c in range(3):
                    a, bb = W[k][c], W[r][c]
                    W[k][c], W[r][c] = np.where(sw, bb, a), np.where(sw, a, bb)
                a, bb = y[k], y[r]
                y[k], y[r] = np.where(sw, bb, a), np.where(sw, a, bb)
            nz = big != 0.0
            for r in range(k + 1, 3):
                W[r][k] = np.where(nz, W[r][k] / W[k][k], W[r][k])
            for r in range(k + 1, 3):
                for c in range(k + 1, 3):
                    W[r][c] = W[r][c] - W[r][k] * W[k][c]
        y[1] = y[1] - W[1][0] * y[0]
        y[2] = y[2] - (W[2][0] * y[0] + W[2][1] * y[1])
        x2 = y[2] / W[2][2]
        x1 = (y[1] - W[1][2] * x2) / W[1][1]
        x0 = (y[0] - (W[0][1] * x1 + W[0][2] * x2)) / W[0][0]
    if info is not None:
        info.append(np.stack(piv_info, -1))
    return np.stack([x0, x1, x2], -1)


def sim3_log(S, lm=EXACT, mg=None, info=None):   # Sim3::log, :148-230 -> [..., 7]
    q, t, s = S
    with np.errstate(all="ignore"):
        sigma = lm.log(s)
        R = quat_to_mat(q)
        d = 0.5 * (R[..., 0] + R[..., 4] + R[..., 8] - 1)
        dR = np.stack([R[..., 7] - R[..., 5], R[..., 2] - R[..., 6], R[..., 3] - R[..., 1]], -1)
        small_s, small_t = np.abs(sigma) < EPS, d > 1 - EPS
        if mg is not None:
            mg.add("branch", np.abs(np.abs(sigma) - EPS) / EPS)
            mg.add("branch", np.abs(d - (1 - EPS)) / EPS)
        if info is not None:
            info.append(np.where(small_s, 0, 2) + np.where(small_t, 0, 1))
        theta = lm.acos(d)
        sn, cs = lm.sin(theta), lm.cos(theta)
        theta2, sigma2 = theta * theta, sigma * sigma
        f = np.where(small_t, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        A01, B01 = (1 - cs) / theta2, (theta - sn) / (theta2 * theta)
        C1 = (s - 1) / sigma
        A10, B10 = ((sigma - 1) * s + 1) / sigma2, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b, c = s * sn, s * cs, theta2 + sigma * sigma
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C1 - ((b - 1) * sigma + a * theta) / c) * 1. / theta2
        A = np.where(small_s, np.where(small_t, 0.5, A01), np.where(small_t, A10, A11))
        B = np.where(small_s, np.where(small_t, 1. / 6., B01), np.where(small_t, B10, B11))
        C = np.where(small_s, 1.0, C1)
        w = f[..., None] * dR
        Om = _skew_parts(w)
        P = _mat3_mul(B[..., None] * Om, Om)
        W = (A[..., None] * Om + P) + C[..., None] * _I9
        ups = lu3_solve(W, t, mg, info)
    return np.concatenate([w, ups, sigma[..., None]], -1)


def edge_error(C, Si, Sjinv, lm=EXACT, mg=None, info=None):   # edgeSim3::computeError, g2o_MultiCol_sim3_expmap.h:86-94
    return sim3_log(sim3_mul(sim3_mul(C, Si), Sjinv), lm, mg, info)


# ---------------------------------------------------------------------------------------------- the linear system
def ldlt_solve(H, b, reverse=False):
    """Unpivoted LDL^T of the symmetric H (its lower triangle), right-looking in panels of PANEL columns, then the two substitutions.  (ok, x): ok is False at
    the first pivot that is zero or not finite, and x is then None.  Inside a panel and in the panel solve every entry loses (l_rj * l_kj) * d_j in increasing
    j; the trailing update does the same up to kExactSolve unknowns; above, a panel's columns
    receive what the earlier panels take from them as one matrix product just before the panel is factored.  reverse: decreasing j / the product's columns flipped."""
    n = len(b)
    S = np.array(H, np.float64, order="F")   # a column is contiguous
    d = np.zeros(n)
    exact = n <= kExactSolve
    with np.errstate(all="ignore"):
        for c0 in range(0, n, PANEL):
            c1 = min(n, c0 + PANEL)
            if not exact and c0:   # left-looking: what the earlier panels' trailing updates took from these columns, as one product
                Lq, dq = (S[c0:, c0 - 1::-1], d[c0 - 1::-1]) if reverse else (S[c0:, :c0], d[:c0])
                S[c0:, c0:c1] -= (Lq * dq) @ Lq[:c1 - c0].T
            for j in range(c0, c1):   # the diagonal block and the panel below it, column by column
                dj = S[j, j]
                if dj == 0.0 or not np.isfinite(dj):
                    return False, None
                d[j] = dj
                l = S[j + 1:, j] / dj
                S[j + 1:, j] = l
                if j + 1 < c1:
                    S[j + 1:, j + 1:c1] -= ((l[:c1 - j - 1, None] * l[None, :]) * dj).T
            if c1 == n:
                break
            if exact:
                Lp = S[c1:, c0:c1]
                for j in (range(c1 - c0 - 1, -1, -1) if reverse else range(c1 - c0)):
                    S[c1:, c1:] -= (Lp[:, j, None] * Lp[None, :, j]) * d[c0 + j]
        y = np.array(b, np.float64)
        for k in range(n):
            y[k + 1:] -= S[k + 1:, k] * y[k]
        y = y / d
        S = np.ascontiguousarray(S)                # a row is contiguous
        for k in range(n - 1, -1, -1):
            y[:k] -= S[k, :k] * y[k]
    return True, y


class Problem:
    def __init__(self, Scw, Snc, has_nc, fixed, edge_i, edge_j, edge_kind, pos, pt_ref):
        self.Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8)
        self.Snc = np.ascontiguousarray(Snc, np.float64).reshape(-1, 8)
        self.has_nc = np.ascontiguousarray(has_nc, np.uint8)
        self.fixed = np.ascontiguousarray(fixed, np.uint8)
        self.edge_i = np.ascontiguousarray(edge_i, np.int32)
        self.edge_j = np.ascontiguousarray(edge_j, np.int32)
        self.edge_kind = np.ascontiguousarray(edge_kind, np.uint8)
        self.pos = np.ascontiguousarray(pos, np.float64).reshape(-1, 3)
        self.pt_ref = np.ascontiguousarray(pt_ref, np.int32)

    def arrays(self):
        return (self.Scw, self.Snc, self.has_nc, self.fixed, self.edge_i, self.edge_j, self.edge_kind, self.pos, self.pt_ref)


class Result:
    status = EG_OK
    iters = 0
    stop = STOP_NOT_RUN
    n_free = 0
    n_edges = 0
    lam = 0.0
    chi2 = 0.0

    def __init__(self):
        self.trials = [0] * 20
        self.Scw_out = self.pose = self.kf_t = self.pos = None
        self.margins = Margins()
        self.branches = set()
        self.pivots = set()


def measurements(pr):
    """Sjw * Swi per edge that passes the guards (:355-371, :384-459) and the indices of those edges"""
    K = len(pr.Scw)
    ok = (pr.edge_i >= 0) & (pr.edge_i < K) & (pr.edge_j >= 0) & (pr.edge_j < K) & (pr.edge_i != pr.edge_j)
    idx = np.nonzero(ok)[0]
    ei, ej, kind = pr.edge_i[idx], pr.edge_j[idx], pr.edge_kind[idx]
    src = lambda v: np.where(((kind != 0) & (pr.has_nc[v] != 0))[:, None], pr.Snc[v], pr.Scw[v])   # noqa: E731
    Swi = sim3_inverse(sim3_of(src(ei)))
    return idx, ei, ej, sim3_mul(sim3_of(src(ej)), Swi)


def _steps():
    u = np.zeros((15, 7))
    for dd in range(7):
        u[1 + 2 * dd, dd] = DELTA
        u[2 + 2 * dd, dd] = -DELTA
    return u


def jacobians(est, ei, ej, meas, lm=EXACT, mg=None, res=None):
    """the 29 residuals of every edge: r [E, 29, 7] (0: the estimate; 1 + 2d / 2 + 2d: vertex i moved by +-1e-9 e_d; 15 + 2d / 16 + 2d: vertex j), and both
    numeric Jacobians [E, 7(row), 7(column d)] (base_binary_edge.hpp:130-205)"""
    K = len(est[0])
    step = sim3_exp(_steps()[1:], lm, mg)
    V = tuple(np.concatenate([c[:, None], m], 1) for c, m in zip(est, sim3_mul(tuple(x[None] for x in step), tuple(x[:, None] for x in est))))   # [K, 15]
    Vinv = sim3_inverse(V)
    E = len(ei)
    ki = np.concatenate([np.arange(15), np.zeros(14, int)])
    kj = np.concatenate([np.zeros(15, int), np.arange(1, 15)])
    Si = tuple(x[ei[:, None], ki[None]] for x in V)
    Sj = tuple(x[ej[:, None], kj[None]] for x in Vinv)
    C = tuple(x[:, None] for x in meas)
    info = []
    r = edge_error(C, Si, Sj, lm, mg, info)
    if res is not None and E:
        res.branches |= set(int(b) for b in np.unique(info[0]))
        res.pivots |= set(tuple(int(c) for c in p) for p in np.unique(info[1].reshape(-1, 2), axis=0))
    scalar = 1.0 / (2 * DELTA)
    A = np.stack([scalar * (r[:, 1 + 2 * dd] - r[:, 2 + 2 * dd]) for dd in range(7)], -1)
    B = np.stack([scalar * (r[:, 15 + 2 * dd] - r[:, 16 + 2 * dd]) for dd in range(7)], -1)
    return r, A, B


def residuals(est, ei, ej, meas, lm=EXACT, mg=None):
    return edge_error(meas, tuple(x[ei] for x in est), tuple(x[ej] for x in sim3_inverse(est)), lm, mg)


def _chi(r, reverse):   # e.dot(information * e) with the identity: the seven squares left to right; the edges in order
    c = r[:, 0] * r[:, 0]
    for k in range(1, 7):
        c = c + r[:, k] * r[:, k]
    tot = 0.0
    for v in (c[::-1] if reverse else c):
        tot += float(v)
    return c, tot


def build_system(A, B, r0, ei, ej, fidx, nfree, reverse):
    """H (dense, symmetric, both triangles filled) and b over the free vertices (base_binary_edge.hpp:55-90): block (i, i) += A^T A, (j, j) += B^T B,
    (i, j) += A^T B, b_i += -A^T e, b_j += -B^T e; every block's entries sum over the seven rows in increasing k and over the edges in ascending order"""
    N = 7 * nfree
    H = np.zeros((N, N))
    b = np.zeros(N)

    def ata(X, Y):
        out = X[:, 0, :, None] * Y[:, 0, None, :]
        for k in range(1, 7):
            out = out + X[:, k, :, None] * Y[:, k, None, :]
        return out

    def atv(X, e):
        out = X[:, 0, :] * -e[:, 0, None]
        for k in range(1, 7):
            out = out + X[:, k, :] * -e[:, k, None]
        return out

    AA, BB, AB, Ae, Be = ata(A, A), ata(B, B), ata(A, B), atv(A, r0), atv(B, r0)
    order = range(len(ei) - 1, -1, -1) if reverse else range(len(ei))
    for e in order:
        fi, fj = fidx[ei[e]], fidx[ej[e]]
        if fi >= 0:
            H[7 * fi:7 * fi + 7, 7 * fi:7 * fi + 7] += AA[e]
            b[7 * fi:7 * fi + 7] += Ae[e]
        if fj >= 0:
            H[7 * fj:7 * fj + 7, 7 * fj:7 * fj + 7] += BB[e]
            b[7 * fj:7 * fj + 7] += Be[e]
        if fi >= 0 and fj >= 0:
            H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += AB[e]
            H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += AB[e].T
    return H, b


def pose_of(S):
    """invMat(toCvSE3(R, t / s)) of :481-484 -> [K, 16] row-major, and Hom2T of it [K, 3]"""
    R = quat_to_mat(S[0])
    t = S[1] / S[2][:, None]
    K = len(R)
    out = np.zeros((K, 16))
    for i in range(3):
        s = np.zeros(K)
        for k in range(3):
            out[:, 4 * i + k] = R[:, 3 * k + i]
            s = s + (-R[:, 3 * k + i]) * t[:, k]
        out[:, 4 * i + 3] = s
    out[:, 15] = 1.0
    return out, out[:, [3, 7, 11]].copy()


def optimize(pr, lm=EXACT, reverse=False, fix=(), max_iterations=20):
    with np.errstate(all="ignore"):
        return _optimize(pr, lm, reverse, set(fix), max_iterations)


def _optimize(pr, lm, reverse, fix, max_iterations):
    """fix: the quirks "repaired", for the tests that show each one matters: dedup (a pair gets one edge), cap (the action's cap ignored), nc_both (a kind-1
    edge takes Scw on both sides unless both have an Snc), all_points (a point of reference -1 is mapped through vertex 0)"""
    res = Result()
    mg = res.margins
    K = len(pr.Scw)
    fidx = np.full(K, -1)
    free = np.nonzero(pr.fixed == 0)[0]
    fidx[free] = np.arange(len(free))
    res.n_free = nfree = len(free)
    if "nc_both" in fix:
        pr = Problem(*pr.arrays())
        both = (pr.has_nc[np.clip(pr.edge_i, 0, K - 1)] != 0) & (pr.has_nc[np.clip(pr.edge_j, 0, K - 1)] != 0)
        pr.edge_kind = np.where(both, pr.edge_kind, 0).astype(np.uint8)
    idx, ei, ej, meas = measurements(pr)
    if "dedup" in fix:
        seen, keep = set(), []
        for n, (a, b) in enumerate(zip(ei, ej)):
            key = (min(a, b), max(a, b))
            if key not in seen:
                seen.add(key)
                keep.append(n)
        keep = np.array(keep, int)
        idx, ei, ej, meas = idx[keep], ei[keep], ej[keep], tuple(x[keep] for x in meas)
    res.n_edges = len(idx)
    if nfree == 0:
        res.status = EG_NO_FREE_VERTEX
        return res
    if len(idx) == 0:
        res.status = EG_FAILED
        return res
    est = sim3_of(pr.Scw)
    N = 7 * nfree
    lam, ni, nbad, last_chi = 0.0, 2.0, 0, 0.0
    it, why, ok = 0, STOP_ITERATIONS, True
    stop = False
    while it < max_iterations and not stop and ok:
        r, A, B = jacobians(est, ei, ej, meas, lm, mg, res)
        _, current = _chi(r[:, 0], reverse)
        ini = post = current
        if it == 0:
            if not (np.isfinite(r[:, 0]).all() and np.isfinite(A[fidx[ei] >= 0]).all() and np.isfinite(B[fidx[ej] >= 0]).all() and math.isfinite(current)):
                res.status = EG_NONFINITE
                return res
            lam, ni, nbad = 1e-6, 2.0, 0
        H, b = build_system(A, B, r[:, 0], ei, ej, fidx, nfree, reverse)
        qmax, x = 0, np.zeros(N) if it == 0 else x   # noqa: F821 — a failed solve leaves the previous x
        while True:
            solved, xs = ldlt_solve(H + lam * np.eye(N), b, reverse)
            if solved:
                x = xs
            upd = sim3_exp(x.reshape(nfree, 7), lm, mg)
            trial = tuple(c.copy() for c in est)
            moved = sim3_mul(upd, tuple(c[free] for c in est))
            for c, m in zip(trial, moved):
                c[free] = m
            rt = residuals(trial, ei, ej, meas, lm, mg)
            _, raw = _chi(rt, reverse)
            temp = raw if solved else DBL_MAX
            rho = current - temp
            scale = 0.0
            for k in (range(N - 1, -1, -1) if reverse else range(N)):
                scale += float(x[k]) * (lam * float(x[k]) + float(b[k]))
            scale += 1e-3
            rho /= scale
            post = raw
            mg.add("rho", [sum_margin(current, temp)])
            if rho > 0 and math.isfinite(temp):
                alpha = 1. - pow(2 * rho - 1, 3)
                alpha = min(alpha, 2. / 3.)
                lam *= max(1. / 3., alpha)
                ni = 2.0
                current = temp
                est = trial
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        res.trials[it] = qmax
        if qmax == 10 or rho == 0:
            ok, why = False, STOP_TRIALS
        else:
            nbad = nbad + 1 if (ini - current) * 1e3 < ini else 0
            if nbad >= 3:
                ok, why = False, STOP_NBAD
        # postIteration(it): the terminate action, on the errors the edges hold (those of the last trial)
        if it == 0:
            last_chi = post
        elif it < 15 or "cap" in fix:
            gain = (last_chi - post) / post
            last_chi = post
            mg.add("gain", [abs(gain - 1e-6) / 1e-6, abs(gain) / 1e-6])
            if gain >= 0 and gain < 1e-6:
                stop = True
                if ok:
                    why = STOP_GAIN
        else:
            stop = True
            if ok:
                why = STOP_CAP
        res.lam, res.chi2 = lam, current
        it += 1
    res.iters, res.stop = it, why
    res.Scw_out = sim3_vec(est)
    res.pose, res.kf_t = pose_of(est)
    res.pos = pr.pos.copy()
    ref = pr.pt_ref.copy()
    if "all_points" in fix:
        ref[ref < 0] = 0
    sel = np.nonzero((ref >= 0) & (ref < K))[0]
    if len(sel):
        Srw = sim3_of(pr.Scw[ref[sel]])
        Swr = sim3_inverse(tuple(c[ref[sel]] for c in est))
        res.pos[sel] = sim3_map(Swr, sim3_map(Srw, pr.pos[sel]))
    return res
