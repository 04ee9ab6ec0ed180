"""cSim3Solver (src/cSim3Solver.cpp, include/cSim3Solver.h) stated line by line, with the OpenCV pieces it calls restated once:
cv::Matx products (s = 0; s += a(i,k) * b(k,j) in increasing k), Matx::dot (row-major), Vec operator/= (a multiplication by 1. / alpha), cv::eigen of the
symmetric 4x4 (JacobiImpl_, cyclic pivot on the largest off-diagonal element, OpenCV's hypot, selection sort), cv::norm, the one MatExpr scale factor of
`2 * ang * vec / norm(vec)`, cv::Rodrigues, cv::pow(P3, 2).  The draws are an input.  The projection is the oracle's WorldToCamHom_fast
(oracle_lib.world_to_cam: glibc atan, pinned against src/cam_model_omni.cpp).  Python floats are IEEE doubles and numpy element-wise operations do
not contract, so every step below rounds as the reference's does.  Divisions, square roots, cos and sin go through _div / _sqrt / _cos / _sin, which return
what IEEE arithmetic and C's libm return (an infinity or a NaN) where Python would raise: non-finite and degenerate inputs (tests/hostile_sim3.py) are stated,
not refused.  Comparisons with a NaN are false in Python as in C++."""
import math

import numpy as np

import oracle_lib as O

DBL_EPSILON = 2.220446049250313e-16
INT_MIN = -2147483648
_M64 = (1 << 64) - 1
FLAG_BAND = 1e-9   # pairs whose error lies within FLAG_BAND * threshold of the threshold may differ from the device (ocml vs glibc in the last place)


# ---------------------------------------------------------------------------------------------- the draws (the one deviation)
def draw(seed, solver, k, j, n):
    """output number ctr + 1 of the splitmix64 stream at seed, ctr = (solver << 32) | (3k + j), mapped to [0, n) by (hi32 * n) >> 32"""
    ctr = ((solver & 0xFFFFFFFF) << 32) | ((3 * k + j) & 0xFFFFFFFF)
    z = (seed + 0x9E3779B97F4A7C15 * (ctr + 1)) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    z ^= z >> 31
    return ((z >> 32) * n) >> 32


def generated_draws(seed, solver, n):
    return lambda k, j: draw(seed, solver, k, j, n)


def table_draws(table):
    """caller draws: table[k][j] = randi of iteration k, pick j"""
    t = np.asarray(table, np.int64).reshape(-1, 3)
    return lambda k, j: int(t[k, j])


# ---------------------------------------------------------------------------------------------- SetRansacParameters (:139-165)
def _cvt_int(d):
    """double -> int as x86-64 converts it (cvttsd2si): INT_MIN when out of range or NaN"""
    return int(d) if (d >= -2147483648.0 and d < 2147483648.0) else INT_MIN


def ransac_max_its(probability, minInliers, maxIterations, N):
    with np.errstate(all="ignore"):
        epsilon = np.float64(minInliers) / np.float64(N)
        if minInliers == N:
            nIterations = 1
        else:
            d = np.ceil(np.log(np.float64(1) - np.float64(probability)) / np.log(np.float64(1) - np.float64(math.pow(float(epsilon), 3))))
            nIterations = _cvt_int(float(d))
    return max(1, min(nIterations, maxIterations))


def max_error(sigma2):
    """mvnMaxError1/2 are std::vector<size_t>: 9.210 * sigma^2 truncated.  A product that is NaN, negative or >= 2^64 has no defined conversion (in the
    reference either): mcs_sim3_create refuses it, and so does the model"""
    e = 9.210 * float(sigma2)
    if not (e >= 0.0 and e < 18446744073709551616.0):   # false for NaN
        raise ValueError("9.210 * sigma2 = %r cannot be converted to size_t" % e)
    return float(int(e))


# ---------------------------------------------------------------------------------------------- cv::Matx / cConverter
def matmul(A, B):
    n, m, p = len(A), len(B), len(B[0])
    out = [[0.0] * p for _ in range(n)]
    for i in range(n):
        for j in range(p):
            s = 0.0
            for k in range(m):
                s += A[i][k] * B[k][j]
            out[i][j] = s
    return out


def inv_mat(M):
    """cConverter::invMat (src/cConverter.cpp:31-44)"""
    M = [[float(x) for x in row] for row in np.asarray(M, np.float64).reshape(4, 4)]
    R = [[M[j][i] for j in range(3)] for i in range(3)]
    t = [0.0, 0.0, 0.0]
    for i in range(3):
        s = 0.0
        for k in range(3):
            s += -R[i][k] * M[k][3]
        t[i] = s
    return np.array([R[0] + [t[0]], R[1] + [t[1]], R[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]])


# ---------------------------------------------------------------------------------------------- cv::eigen (JacobiImpl_)
def _div(a, b):
    """a / b as IEEE divides: x / 0 is an infinity or NaN, never an exception"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    """sqrt as IEEE: NaN of a NaN or a negative number"""
    return math.sqrt(x) if x >= 0.0 else float("nan")


def _cos(x):
    return math.cos(x) if math.isfinite(x) else float("nan")   # glibc's cos for every finite argument; NaN of an infinity as in C


def _sin(x):
    return math.sin(x) if math.isfinite(x) else float("nan")


def cv_hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = _div(b, a)
        return a * _sqrt(1 + b * b)
    if b > 0:
        a = _div(a, b)
        return b * _sqrt(1 + a * a)
    return 0.0


def jacobi_eigen(A, info=None):
    """symmetric n x n (list of lists, consumed) -> (W descending, V rows = eigenvectors).  Comparisons with a NaN are false as in C++: the pivot search
    keeps its first candidate, `fabs(p) <= eps` does not break (the n * n * 30 cap ends the loop) and the selection sort does not swap.  info (a dict)
    receives the number of rotations made"""
    n = len(A)
    rotations = 0
    A = [float(x) for row in A for x in row]
    V = [1.0 if i % (n + 1) == 0 else 0.0 for i in range(n * n)]
    W = [0.0] * n
    indR, indC = [0] * n, [0] * n
    for k in range(n):
        W[k] = A[(n + 1) * k]
        if k < n - 1:
            m, mv = k + 1, abs(A[n * k + k + 1])
            for i in range(k + 2, n):
                val = abs(A[n * k + i])
                if mv < val:
                    mv, m = val, i
            indR[k] = m
        if k > 0:
            m, mv = 0, abs(A[k])
            for i in range(1, k):
                val = abs(A[n * i + k])
                if mv < val:
                    mv, m = val, i
            indC[k] = m
    if n > 1:
        for _ in range(n * n * 30):
            k, mv = 0, abs(A[indR[0]])
            for i in range(1, n - 1):
                val = abs(A[n * i + indR[i]])
                if mv < val:
                    mv, k = val, i
            l = indR[k]
            for i in range(1, n):
                val = abs(A[n * indC[i] + i])
                if mv < val:
                    mv, k, l = val, indC[i], i
            p = A[n * k + l]
            if abs(p) <= DBL_EPSILON:
                break
            y = (W[l] - W[k]) * 0.5
            t = abs(y) + cv_hypot(p, y)
            s = cv_hypot(p, t)
            c = _div(t, s)
            s = _div(p, s)
            t = _div(p, t) * p
            rotations += 1
            if y < 0:
                s, t = -s, -t
            A[n * k + l] = 0.0
            W[k] -= t
            W[l] += t

            def rot(i0, i1, X):
                a0, b0 = X[i0], X[i1]
                X[i0] = a0 * c - b0 * s
                X[i1] = a0 * s + b0 * c
            for i in range(0, k):
                rot(n * i + k, n * i + l, A)
            for i in range(k + 1, l):
                rot(n * k + i, n * i + l, A)
            for i in range(l + 1, n):
                rot(n * k + i, n * l + i, A)
            for i in range(n):
                rot(n * k + i, n * l + i, V)
            for idx in (k, l):
                if idx < n - 1:
                    m, mv = idx + 1, abs(A[n * idx + idx + 1])
                    for i in range(idx + 2, n):
                        val = abs(A[n * idx + i])
                        if mv < val:
                            mv, m = val, i
                    indR[idx] = m
                if idx > 0:
                    m, mv = 0, abs(A[idx])
                    for i in range(1, idx):
                        val = abs(A[n * i + idx])
                        if mv < val:
                            mv, m = val, i
                    indC[idx] = m
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            for i in range(n):
                V[n * m + i], V[n * k + i] = V[n * k + i], V[n * m + i]
    if info is not None:
        info["rotations"] = rotations
    return W, [V[n * i:n * i + n] for i in range(n)]


# ---------------------------------------------------------------------------------------------- computeT (:286-371)
def rodrigues(r):
    rx, ry, rz = r
    theta = _sqrt(rx * rx + ry * ry + rz * rz)
    if theta < DBL_EPSILON:
        return [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    c, s = _cos(theta), _sin(theta)
    c1 = 1.0 - c
    itheta = _div(1.0, theta) if theta else 0.0
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    R = [c * I[k] + c1 * rrt[k] + s * r_x[k] for k in range(9)]
    return [R[0:3], R[3:6], R[6:9]]


def centroid(P):
    C = [0.0, 0.0, 0.0]
    for i in range(3):
        for r in range(3):
            C[r] += P[r][i]
    ia = 1.0 / 3.0   # OpenCV Vec operator/=(double): multiply by 1./alpha
    C = [C[r] * ia for r in range(3)]
    Pr = [[P[r][i] - C[r] for i in range(3)] for r in range(3)]
    return Pr, C


def compute_t(P1, P2, ang_ulps=0):
    """P1, P2: 3x3, one point per column -> dict(R, t, s, T12, T21) as arrays, and what the Jacobi solver did: N (the 4x4 it was given), W, V, rotations.
    ang_ulps moves the quaternion's angle by that many units in the last place (the model's own sensitivity to the libm behind atan2)"""
    Pr1, O1 = centroid(P1)
    Pr2, O2 = centroid(P2)
    M = matmul(Pr2, [[Pr1[j][i] for j in range(3)] for i in range(3)])
    N11 = M[0][0] + M[1][1] + M[2][2]
    N12 = M[1][2] - M[2][1]
    N13 = M[2][0] - M[0][2]
    N14 = M[0][1] - M[1][0]
    N22 = M[0][0] - M[1][1] - M[2][2]
    N23 = M[0][1] + M[1][0]
    N24 = M[2][0] + M[0][2]
    N33 = -M[0][0] + M[1][1] - M[2][2]
    N34 = M[1][2] + M[2][1]
    N44 = -M[0][0] - M[1][1] + M[2][2]
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    info = {}
    W, V = jacobi_eigen([row[:] for row in N], info)
    vec = V[0][1:4]
    nv = _sqrt(((0.0 + vec[0] * vec[0]) + vec[1] * vec[1]) + vec[2] * vec[2])
    ang = math.atan2(nv, V[0][0])
    for _ in range(abs(ang_ulps)):
        ang = math.nextafter(ang, math.inf if ang_ulps > 0 else -math.inf)
    f = (2 * ang) * _div(1.0, nv)
    vec = [v * f for v in vec]
    R = rodrigues(vec)
    P3 = matmul(R, Pr2)
    nom = 0.0
    for i in range(3):
        for j in range(3):
            nom += Pr1[i][j] * P3[i][j]
    den = 0.0
    for i in range(3):
        for j in range(3):
            den += P3[i][j] * P3[i][j]
    s = _div(nom, den)
    sR = [[R[i][j] * s for j in range(3)] for i in range(3)]
    t = [O1[i] - matmul(sR, [[O2[0]], [O2[1]], [O2[2]]])[i][0] for i in range(3)]
    is_ = _div(1.0, s)
    sRinv = [[R[j][i] * is_ for j in range(3)] for i in range(3)]
    tinv = [matmul([[-x for x in row] for row in sRinv], [[t[0]], [t[1]], [t[2]]])[i][0] for i in range(3)]
    T12 = [sR[0] + [t[0]], sR[1] + [t[1]], sR[2] + [t[2]], [0.0, 0.0, 0.0, 1.0]]
    T21 = [sRinv[0] + [tinv[0]], sRinv[1] + [tinv[1]], sRinv[2] + [tinv[2]], [0.0, 0.0, 0.0, 1.0]]
    return dict(R=np.array(R), t=np.array(t), s=s, T12=np.array(T12), T21=np.array(T21), N=np.array(N), W=np.array(W), V=np.array(V),
                rotations=info["rotations"])


def hyp_vector(h):
    """the 45 doubles of mcs_sim3_hypotheses"""
    return np.concatenate([h["T12"].reshape(16), h["T21"].reshape(16), h["R"].reshape(9), h["t"], [h["s"]]])


# ---------------------------------------------------------------------------------------------- the solver
def _affine(M, X):
    """rows 0..2 of a 3x4 / 4x4 (x, 1) product per point, numpy element-wise in the reference's order; M [n,4,4] or [4,4], X [n,3]"""
    M = np.asarray(M, np.float64)
    if M.ndim == 2:
        M = np.broadcast_to(M, (len(X), 4, 4))
    out = np.zeros((len(X), 3))
    for i in range(3):
        s = 0.0 + M[:, i, 0] * X[:, 0]
        s = s + M[:, i, 1] * X[:, 1]
        s = s + M[:, i, 2] * X[:, 2]
        out[:, i] = s + M[:, i, 3]
    return out


class Sim3Model:
    """one cSim3Solver.  cams: calibration dicts of the local rig, M_c its poses; M_t_inv (KF1, KF2), MtMc_inv (KF1, KF2) per camera; per kept pair
    Xw [n,2,3], cam [n,2], sigma2 [n,2], index1 [n]; mN1 = vpMatched12.size()"""

    def __init__(self, cams, M_c, M_t_inv, MtMc_inv, Xw, cam, sigma2, index1, mN1):
        self.cams = cams
        self.McInv = [inv_mat(m) for m in M_c]
        Xw = np.asarray(Xw, np.float64).reshape(-1, 2, 3)
        cam = np.asarray(cam, np.int64).reshape(-1, 2)
        sigma2 = np.asarray(sigma2, np.float64).reshape(-1, 2)
        self.N = len(Xw)
        self.mN1 = int(mN1)
        self.index1 = np.asarray(index1, np.int64)
        self.cam1, self.cam2 = cam[:, 0].copy(), cam[:, 1].copy()
        self.X1c = self._rig(M_t_inv[0], Xw[:, 0])
        self.X2c = self._rig(M_t_inv[1], Xw[:, 1])
        self.P1 = self._project(MtMc_inv[0], Xw[:, 0], self.cam1)
        self.P2 = self._project(MtMc_inv[1], Xw[:, 1], self.cam2)
        self.e1 = np.array([max_error(v) for v in sigma2[:, 0]])
        self.e2 = np.array([max_error(v) for v in sigma2[:, 1]])
        self.mnIterations, self.mnBestInliers = 0, 0
        self.best = None
        self.SetRansacParameters()

    @staticmethod
    def _rig(Mt_inv, X):
        """Hom2R(hom) * X + Hom2T(hom)"""
        H = np.asarray(Mt_inv, np.float64).reshape(4, 4)
        out = np.zeros((len(X), 3))
        for i in range(3):
            s = 0.0 + H[i, 0] * X[:, 0]
            s = s + H[i, 1] * X[:, 1]
            s = s + H[i, 2] * X[:, 2]
            out[:, i] = s + H[i, 3]
        return out

    def _project(self, M, X, cam):
        if len(X) == 0:
            return np.zeros((0, 2))
        uv, _ = O.world_to_cam(np.asarray(M, np.float64).reshape(-1, 16), self.cams, None, X, cam.astype(np.int32))
        return uv

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        self.mRansacProb, self.mRansacMinInliers = probability, minInliers
        self.mRansacMaxIts = ransac_max_its(probability, minInliers, maxIterations, self.N) if self.N >= minInliers else 0
        self.mnIterations = 0

    def hypothesis(self, k, draws):
        """iteration k -> (picks, computeT dict)"""
        avail = list(range(self.N))   # a fixed array of N entries: pop_back leaves the stale value in place
        size = self.N
        picks = []
        for j in range(3):
            randi = draws(k, j)
            idx = avail[randi]
            picks.append(idx)
            avail[idx] = avail[size - 1]
            size -= 1
        P1 = [[float(self.X1c[p, r]) for p in picks] for r in range(3)]
        P2 = [[float(self.X2c[p, r]) for p in picks] for r in range(3)]
        return picks, compute_t(P1, P2)

    def errors(self, h):
        """the two squared reprojection errors of CheckInliers (:374-415) per pair -> (err1 [N], err2 [N])"""
        if self.N == 0:
            return np.zeros(0), np.zeros(0)
        with np.errstate(all="ignore"):
            p21 = _affine(h["T12"], self.X2c)   # row 3 of T12 (X, 1) is exactly 1, so (p21, 1) is the 4-vector the reference multiplies on
            p12 = _affine(h["T21"], self.X1c)
            M = np.stack(self.McInv).reshape(-1, 16)
            uv1, _ = O.world_to_cam(M, self.cams, None, p21, self.cam1.astype(np.int32))
            uv2, _ = O.world_to_cam(M, self.cams, None, p12, self.cam2.astype(np.int32))
            d1 = self.P1 - uv1
            d2 = uv2 - self.P2
            err1 = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]
            err2 = d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]
        return err1, err2

    def check_inliers(self, h):
        """CheckInliers (:374-415) -> (inlier flags [N], near-threshold flags [N]).  A threshold of 0 has no band: err < 0 is false whatever err is"""
        err1, err2 = self.errors(h)
        with np.errstate(all="ignore"):
            inl = (err1 < self.e1) & (err2 < self.e2)
            near = ((self.e1 > 0) & (np.abs(err1 - self.e1) <= FLAG_BAND * self.e1)) | ((self.e2 > 0) & (np.abs(err2 - self.e2) <= FLAG_BAND * self.e2))
        return inl, near

    def evaluate(self, k, draws):
        picks, h = self.hypothesis(k, draws)
        inl, near = self.check_inliers(h)
        return picks, h, inl, near

    def iterate(self, nIterations, draws):
        """-> (success, bNoMore, vbInliers [mN1], nInliers, T12 or None, near-threshold pairs seen)"""
        vb = np.zeros(self.mN1, bool)
        near_total = 0
        if self.N < self.mRansacMinInliers:
            return False, True, vb, 0, None, 0
        nCurrentIterations = 0
        while self.mnIterations < self.mRansacMaxIts and nCurrentIterations < nIterations:
            nCurrentIterations += 1
            k = self.mnIterations
            self.mnIterations += 1
            _, h, inl, near = self.evaluate(k, draws)
            near_total += int(near.sum())
            n = int(inl.sum())
            if n >= self.mnBestInliers:
                self.mnBestInliers = n
                self.best = h
                if n > self.mRansacMinInliers:
                    vb[self.index1[inl]] = True
                    return True, False, vb, n, h["T12"], near_total
        return False, self.mnIterations >= self.mRansacMaxIts, vb, 0, None, near_total


# ---------------------------------------------------------------------------------------------- synthetic loop-candidate pairs for the tests
def level_sigma2(nlevels=8, scale=1.2):
    """cMultiFrame's mvLevelSigma2: the scale factor is the double of the float constructor argument"""
    f = float(np.float32(scale))
    sf, out = [1.0], [1.0]
    for i in range(1, nlevels):
        sf.append(sf[i - 1] * f)
        out.append(sf[i] * sf[i])
    return out


def rig_poses(nr):
    """camera c looks along +z rotated by 2 pi c / nr about the rig's y axis, 5 cm off the rig centre"""
    out = []
    for c in range(nr):
        a = 2 * math.pi * c / nr
        R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
        M = np.eye(4)
        M[:3, :3] = R
        M[:3, 3] = R @ np.array([0.0, 0.0, 0.05])
        out.append(M)
    return out


def random_pose(rng, trans=2.0):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = rng.normal(0, trans, 3)
    return M


def make_pair(rng, M_c, n, inlier_frac=0.7, noise=0.002, extra=10, scale=None):
    """one loop-candidate pair: KF2's map points are KF1's moved by a similarity (s, R, t) of the rig frames, X1c = s R X2c + t, plus noise and
    outliers -> dict of the mcs_sim3_create inputs of one solver + the truth"""
    nr = len(M_c)
    Mt1, Mt2 = random_pose(rng), random_pose(rng)
    s = float(rng.uniform(0.5, 2.0)) if scale is None else scale
    S = random_pose(rng, 0.5)
    R, t = S[:3, :3], S[:3, 3]
    cam1 = rng.integers(0, nr, n)
    d = rng.normal(size=(n, 3))
    d[:, 2] = np.abs(d[:, 2]) + 0.6
    d /= np.linalg.norm(d, axis=1)[:, None]
    Xcam = d * rng.uniform(2.0, 8.0, (n, 1))
    X1c = np.stack([(M_c[c][:3, :3] @ Xcam[i]) + M_c[c][:3, 3] for i, c in enumerate(cam1)])
    X1w = (Mt1[:3, :3] @ X1c.T).T + Mt1[:3, 3]
    X2c = ((X1c - t) @ R) / s   # R^T (X1c - t) / s
    McI = [np.linalg.inv(m) for m in M_c]
    zc = np.stack([(McI[c][:3, :3] @ X2c.T).T[:, 2] + McI[c][2, 3] for c in range(nr)], axis=1)
    cam2 = np.argmax(zc, axis=1)
    X2w = (Mt2[:3, :3] @ X2c.T).T + Mt2[:3, 3] + rng.normal(0, noise, (n, 3))
    out = rng.random(n) >= inlier_frac
    X2w[out] = (Mt2[:3, :3] @ (rng.normal(0, 4.0, (int(out.sum()), 3))).T).T + Mt2[:3, 3]
    sig = level_sigma2()
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    mN1 = n + extra
    index1 = np.sort(rng.choice(mN1, n, replace=False)).astype(np.int32)
    Mt_inv = np.stack([inv_mat(Mt1).reshape(16), inv_mat(Mt2).reshape(16)])
    MtMc_inv = np.stack([np.stack([inv_mat(np.array(matmul(M.tolist(), m.tolist()))).reshape(16) for m in M_c]) for M in (Mt1, Mt2)])
    return dict(Xw=np.stack([X1w, X2w], axis=1), cam=np.stack([cam1, cam2], axis=1).astype(np.int32),
                sigma2=np.stack([[sig[o] for o in oct1], [sig[o] for o in oct2]], axis=1), index1=index1, mN1=mN1, M_t_inv=Mt_inv, MtMc_inv=MtMc_inv,
                outlier=out, s=s, R=R, t=t, Mt=(Mt1, Mt2))


def model_of(pair, cams, M_c):
    return Sim3Model(cams, M_c, pair["M_t_inv"].reshape(2, 4, 4), pair["MtMc_inv"].reshape(2, -1, 4, 4), pair["Xw"], pair["cam"], pair["sigma2"],
                     pair["index1"], pair["mN1"])
