"""Hostile loop candidates for the Sim3 RANSAC (csrc/mcs_sim3.hip): the table of scenes that tests/test_sim3_hostile_cpu.py (the model
states every one of them, and the floors that keep a group from passing vacuously) and tests/test_gpu_hostile_sim3.py (device == model under the rule of
DESIGN.md section 7) both walk.  Plain module: numpy, the model and the CPU oracle only, nothing of the device; the comparisons at the end take what the
device returned as plain arrays.

A scene is dict(cams, M_c, pairs, params, seed, draws): the arguments of one mcs_sim3_create.  pairs are dicts with the keys of sim3_model.make_pair,
params one (probability, minInliers, maxIterations) per solver, draws None (generated from seed) or one [maxIterations, 3] table per solver.

  A  exact triples      lattice-valued correspondences under identity keyframe poses, caller draws: the exact-arithmetic degeneracies of computeT
  B  world scale        one scene with every length multiplied by 1e-9 .. 1e8: the absolute stopping rule of the Jacobi solver
  C  non-finite points  a NaN, an infinity and a 1e200 among 65 correspondences
  D  threshold pairs    correspondences bisected onto their inlier threshold (inside FLAG_BAND) and to 1e-7 relative on either side of it (outside)
  E  hostile projection rigs of the stretched cameras of hostile_cameras, transferred points on an axis, behind a camera and at grazing incidence
  F  sigma^2 edges      thresholds 0 and 1, 9.21e15, mixed per side
  G  batch shape        N around the 64-bit mask words, 130 solvers, 1 and 32 cameras
  H  state              scripts of iterate / SetRansacParameters calls, the best-so-far state compared after every call"""
import importlib
import math

import numpy as np

import hostile_cameras as HC
import sim3_model as M

synth = importlib.import_module("multicol-slam_amd.synth")

SIG = M.level_sigma2()
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lafida():
    return synth.lafida_cameras()


def scene(cams, M_c, pairs, params, seed=0, draws=None):
    return dict(cams=cams, M_c=M_c, pairs=pairs, params=params, seed=seed, draws=draws)


def draws_of(sc, s):
    if sc["draws"] is not None:
        return M.table_draws(sc["draws"][s])
    return M.generated_draws(sc["seed"], s, len(sc["pairs"][s]["index1"]))


def models_of(sc):
    out = []
    for p, q in zip(sc["pairs"], sc["params"]):
        m = M.model_of(p, sc["cams"], sc["M_c"])
        m.SetRansacParameters(*q)
        out.append(m)
    return out


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------------------
def pose_arrays(Mt1, Mt2, M_c):
    """-> M_t_inv [2, 16], MtMc_inv [2, nr, 16] as make_pair forms them"""
    Mt_inv = np.stack([M.inv_mat(Mt1).reshape(16), M.inv_mat(Mt2).reshape(16)])
    MtMc_inv = np.stack([np.stack([M.inv_mat(np.array(M.matmul(np.asarray(Mt).tolist(), np.asarray(m).tolist()))).reshape(16) for m in M_c])
                         for Mt in (Mt1, Mt2)])
    return Mt_inv, MtMc_inv


def rig_pair(M_c, X1c, X2c, cam, sigma2, extra=3):
    """a pair under identity keyframe poses: the world points ARE the rig-frame points (1 * x + 0 * y + 0 * z + 0 is exact), so lattice values stay lattice
    values in both rig frames"""
    n = len(X1c)
    Mt_inv, MtMc_inv = pose_arrays(np.eye(4), np.eye(4), M_c)
    return dict(Xw=np.stack([np.asarray(X1c, np.float64), np.asarray(X2c, np.float64)], axis=1), cam=np.asarray(cam, np.int32).reshape(n, 2),
                sigma2=np.asarray(sigma2, np.float64).reshape(n, 2), index1=(np.arange(n) + np.minimum(np.arange(n) // 8, extra)).astype(np.int32),
                mN1=n + extra, M_t_inv=Mt_inv, MtMc_inv=MtMc_inv)


def _scaled_pose(P, f):
    P = np.array(P, np.float64)
    P[:3, 3] = P[:3, 3] * f
    return P


def scaled_pair(rng, M_c, n, factor, **kw):
    """make_pair with every length multiplied by factor: the points, the M_t translations and the M_c translations -> (pair, the scaled M_c).
    (factor 1.0 multiplies by one: the pair of make_pair itself)"""
    p = M.make_pair(rng, M_c, n, **kw)
    Mc = [_scaled_pose(m, factor) for m in M_c]
    Mt = tuple(_scaled_pose(m, factor) for m in p["Mt"])
    Mt_inv, MtMc_inv = pose_arrays(Mt[0], Mt[1], Mc)
    return dict(p, Xw=p["Xw"] * factor, t=p["t"] * factor, Mt=Mt, M_t_inv=Mt_inv, MtMc_inv=MtMc_inv), Mc


def rz90(X):
    """the exact quarter turn about z: (x, y, z) -> (-y, x, z)"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    return np.stack([-X[:, 1], X[:, 0], X[:, 2]], axis=1)


# ---- A: exact triples --------------------------------------------------------------------------------------------------------------------------------
GENERIC = [(1, 2, 3), (-2, 0, 1), (0, 1, -1)]
LINE = [(1, 0, 0), (2, 0, 0), (4, 0, 0)]
POINT = [(2, -1, 3)] * 3
PLANAR = [(1, 0, 0), (0, 2, 0), (-3, 1, 0)]          # z = 0: N's first row vanishes under a half turn about z, the quaternion's w is an exact 0
QUARTER = [(1, 0, 2), (-1, 1, 3), (0, -1, 5)]        # centroid on the z axis
# name -> (X1 of the three correspondences, X2 of the three correspondences), lattice values in both rig frames
EXACT_TRIPLES = [
    ("identity", np.eye(3).tolist(), np.eye(3).tolist()),                                   # Pr1 == Pr2: M is symmetric, no rotation touches row 0, nv = 0, 0 * inf
    ("half_turn", [(-x, -y, z) for x, y, z in PLANAR], PLANAR),                              # w == 0: atan2(nv, 0)
    ("quarter_turn", rz90(QUARTER).tolist(), QUARTER),
    ("scale_2", [(2 * x, 2 * y, 2 * z) for x, y, z in GENERIC], GENERIC),                    # M symmetric again: NaN like the identity
    ("scale_half", [(x / 2, y / 2, z / 2) for x, y, z in GENERIC], GENERIC),
    ("reflection", [(x, y, -z) for x, y, z in GENERIC], GENERIC),
    ("collinear_self", LINE, LINE),
    ("collinear_quarter", rz90(LINE).tolist(), LINE),                                        # a double top eigenvalue: the axis depends on every pivot tie
    ("two_coincident", rz90([GENERIC[0], GENERIC[0], GENERIC[1]]).tolist(), [GENERIC[0], GENERIC[0], GENERIC[1]]),
    ("all_coincident", POINT, POINT),
    ("pr2_zero", GENERIC, POINT),
    ("pr1_zero", POINT, GENERIC),
    # collinear onto another line: a double top eigenvalue AND equal off-diagonal magnitudes, so the returned axis changes outright with the order in which
    # the pivot search takes its ties (`mv < val` against `mv <= val`)
    ("collinear_tie_a", [(0, -1, 2), (0, 0, 3), (0, 1, 4)], [(1, 2, 3), (0, 2, 3), (-1, 2, 3)]),
    ("collinear_tie_b", [(0, -1, 2), (-1, -1, 2), (-2, -1, 2)], [(1, 2, 3), (1, 1, 2), (1, 0, 1)]),
    # two coincident points on one side only: Pr2 is collinear (a double top eigenvalue again) while the centroids are thirds, so the products round: a
    # contracted multiply-add changes N in the last place and, through the double eigenvalue, the returned axis outright (with every product exact, as
    # in the collinear cases above, a contraction changes nothing)
    ("coincident_pair_one_side", [(2, -1, 3), (0, -1, 2), (0, 1, 0)], [(1, 2, 3), (1, 2, 3), (0, 1, 0)]),
]
EXACT_CASES = len(EXACT_TRIPLES)
EXACT_ITERATIONS = 60
EXACT_FILL = 20


def exact_scene():
    """N = 65: the fifteen triples above (correspondences 3k .. 3k + 2, camera 0, which rig_poses makes the exact identity rotation), then 20 lattice
    correspondences under the exact quarter turn (so the quarter-turn hypothesis is a success).  Draw k < 15 picks triple k; the others are random."""
    def make():
        rng = np.random.default_rng(2201)
        X1 = np.concatenate([np.asarray(t[1], np.float64) for t in EXACT_TRIPLES])
        X2 = np.concatenate([np.asarray(t[2], np.float64) for t in EXACT_TRIPLES])
        F2 = np.stack([rng.integers(-4, 5, EXACT_FILL), rng.integers(-4, 5, EXACT_FILL), rng.integers(2, 9, EXACT_FILL)], axis=1).astype(np.float64)
        X1, X2 = np.concatenate([X1, rz90(F2)]), np.concatenate([X2, F2])
        n = len(X1)
        cam = np.zeros((n, 2), np.int32)
        cam[3 * EXACT_CASES:, 0], cam[3 * EXACT_CASES:, 1] = np.arange(EXACT_FILL) % 3, (np.arange(EXACT_FILL) + 1) % 3
        sig = np.array([[SIG[i % 8], SIG[(3 * i + 1) % 8]] for i in range(n)])
        M_c = M.rig_poses(3)
        d = rng.integers(0, n, (EXACT_ITERATIONS, 3))
        d[:EXACT_CASES] = [[3 * k, 3 * k + 1, 3 * k + 2] for k in range(EXACT_CASES)]
        return scene(lafida(), M_c, [rig_pair(M_c, X1, X2, cam, sig)], [(0.98, 15, EXACT_ITERATIONS)], draws=[d])
    return _once("A", make)


# ---- B: world scale ----------------------------------------------------------------------------------------------------------------------------------
SCALE_FACTORS = (1e-9, 1e-7, 1e-6, 1e-4, 1.0, 1e4, 1e8)
SCALE_ITERATIONS = 40


def scale_scene(factor):
    def make():
        pair, Mc = scaled_pair(np.random.default_rng(2202), M.rig_poses(3), 40, factor, inlier_frac=0.7)
        return scene(lafida(), Mc, [pair], [(0.98, 6, SCALE_ITERATIONS)], seed=2202)
    return _once(("B", factor), make)


def jacobi_residual(h):
    """how far the returned W, V are from diagonalising N: max |V N V^T - diag(W)| / max |W|"""
    with np.errstate(all="ignore"):
        V, N, W = h["V"], h["N"], h["W"]
        return float(np.abs(V @ N @ V.T - np.diag(W)).max() / np.abs(W).max())


# ---- C: non-finite and extreme points ------------------------------------------------------------------------------------------------------------------
POISON_SEED = 2203
POISONED = (7, 23, 50)     # a NaN coordinate on side 1, a +Inf coordinate on side 2, a point at 1e200 (its squares overflow in the projection)
POISON_ITERATIONS = 300


def poison_scene():
    def make():
        M_c = M.rig_poses(3)
        pair = M.make_pair(np.random.default_rng(POISON_SEED), M_c, 65, inlier_frac=0.8)
        pair["Xw"][POISONED[0], 0, 0] = np.nan
        pair["Xw"][POISONED[1], 1, 1] = np.inf
        pair["Xw"][POISONED[2], 0, :] = 1e200
        # the tightest thresholds (9) on the poisoned pairs: a hypothesis drawn from the 1e200 pair has s ~ 1e199 and sends every point to one pixel,
        # which a wide threshold on the other side can contain
        pair["sigma2"][list(POISONED)] = SIG[0]
        return scene(lafida(), M_c, [pair], [(0.98, 6, POISON_ITERATIONS)], seed=POISON_SEED)
    return _once("C", make)


# ---- D: threshold pairs ------------------------------------------------------------------------------------------------------------------------------
IN_BAND = 1e-10      # |err - e| <= IN_BAND * e: inside FLAG_BAND, the device may fall on either side
OUT_BAND = 1e-7      # |err - e| ~ OUT_BAND * e: one hundred times FLAG_BAND, the device must agree
# (correspondence, side whose error is bisected, pyramid level of that side's sigma^2, signed relative distance from the threshold)
THRESHOLD_TARGETS = ([(3 + i, 1 + i % 2, (0, 2, 4)[i % 3], 0.0) for i in range(8)] +
                     [(11 + i, 1 + i % 2, (0, 2, 4)[i % 3], OUT_BAND if i % 4 < 2 else -OUT_BAND) for i in range(8)])


def _sideways(pair, i):
    """a unit vector at right angles to the line from KF2's rig centre to X2w[i]"""
    ray = pair["Xw"][i, 1] - pair["Mt"][1][:3, 3]
    v = np.cross(ray, [0.3, -0.5, 0.8])
    return v / np.linalg.norm(v)


def threshold_scene():
    """a noise-free pair at scale 1 and one hypothesis (draws 0, 1, 2 in every iteration); X2w of the targets is moved sideways by a bisected length until the
    model's error of the chosen side sits where THRESHOLD_TARGETS says.  The other side's threshold is level 7's (118), far above its error."""
    def make():
        cams, M_c = lafida(), M.rig_poses(3)
        pair = M.make_pair(np.random.default_rng(2204), M_c, 40, inlier_frac=1.0, noise=0.0, scale=1.0)
        h = M.model_of(pair, cams, M_c).hypothesis(0, M.table_draws([[0, 1, 2]]))[1]
        for i, side, level, rel in THRESHOLD_TARGETS:
            pair["sigma2"][i] = (SIG[level], SIG[7]) if side == 1 else (SIG[7], SIG[level])
            e = M.max_error(SIG[level])
            want = e * (1.0 + rel)
            base, v = pair["Xw"][i, 1].copy(), _sideways(pair, i)

            def err(delta):
                one = dict(pair, Xw=np.stack([pair["Xw"][i, 0], base + delta * v])[None], cam=pair["cam"][i:i + 1], sigma2=pair["sigma2"][i:i + 1],
                           index1=np.zeros(1, np.int32), mN1=1)
                return float(M.model_of(one, cams, M_c).errors(h)[side - 1][0])
            lo, hi = 0.0, 1e-3
            while err(hi) < want:
                lo, hi = hi, 2 * hi
            best = hi
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                f = err(mid)
                if abs(f - want) < abs(err(best) - want):
                    best = mid
                if abs(f - want) <= 1e-3 * IN_BAND * e:
                    break
                lo, hi = (mid, hi) if f < want else (lo, mid)
            pair["Xw"][i, 1] = base + best * v
        return scene(cams, M_c, [pair], [(0.98, 6, 4)], draws=[np.tile([0, 1, 2], (4, 1))])
    return _once("D", make)


# ---- E: hostile projection -----------------------------------------------------------------------------------------------------------------------------
PROJ_W, PROJ_H = 400, 300
PROJ_ITERATIONS = 40
TRIPLE = QUARTER                                                                    # the hypothesis of draw 0: the exact quarter turn, t = 0 exactly
ON_AXIS = [(0, 0, z) for z in (1, 2, 3, 5, 8)]                                      # T12 X2c = (0, 0, z): norm == 0 in camera 0, the 1e-14 branch
BEHIND = [(1, 2, -3), (-2, 1, -1), (3, -1, -4), (0, 2, -2), (-1, -1, -6)]            # z < 0 in camera 0
GRAZING = [(3, 4, 0.05), (-2, 5, 0.05), (1e6, 0, 0.55), (0, -7, 0.05), (2.5e6, 1e6, 1.05)]   # camera 0 sits at z = 0.05: |z| / norm < 1e-6
PROJ_FILL, PROJ_OUTLIERS = 30, 8


def _max_poly(cam):
    """invP_deg = MCS_MAX_POLY (16): four more coefficients on top of the calibration's twelve"""
    inv = list(cam["invP"]) + [0.5, -0.25, 0.125, -0.0625]
    return dict(cam, invP=inv[:16] + [0.03125] * (16 - len(inv)))


def _one_coefficient(cam):
    """invP_deg = 1: rho is a constant, every point lands on one circle"""
    return dict(cam, invP=[0.3 * PROJ_W])


def projection_rigs():
    """name -> three cameras: every stretched camera of hostile_cameras (mixed per rig camera), and the two polynomial lengths"""
    names = list(HC.STRETCHED)
    groups = [(names[i:i + 3] + names[:3])[:3] for i in range(0, len(names), 3)]      # the last group is filled up from the front
    rigs = {"+".join(g): [HC.camera(n, PROJ_W, PROJ_H) for n in g] for g in groups}
    base = [HC.camera(n, PROJ_W, PROJ_H) for n in HC.CONTROLS]
    rigs["poly16+poly1+lafida2"] = [_max_poly(base[0]), _one_coefficient(base[1]), base[2]]
    return rigs


def lattice_pair(rng, M_c, noise, sigma2):
    """N = 56 correspondences under the exact quarter turn X1c = Rz90 X2c with identity keyframe poses: the triple, the three regimes (cameras 0 / 0),
    30 lattice points seen by different cameras on the two sides (X1c carries `noise`), 8 outliers.  sigma2(i) -> (side 1, side 2)"""
    F2 = np.stack([rng.integers(-5, 6, PROJ_FILL), rng.integers(-5, 6, PROJ_FILL), rng.integers(1, 9, PROJ_FILL)], axis=1).astype(np.float64)
    O2 = np.stack([rng.integers(-5, 6, PROJ_OUTLIERS), rng.integers(-5, 6, PROJ_OUTLIERS), rng.integers(1, 9, PROJ_OUTLIERS)], axis=1).astype(np.float64)
    X2 = np.concatenate([np.asarray(TRIPLE + ON_AXIS + BEHIND + GRAZING, np.float64), F2, O2])
    X1 = rz90(X2)
    k = len(TRIPLE + ON_AXIS + BEHIND + GRAZING)
    X1[k:k + PROJ_FILL] += rng.normal(0, noise, (PROJ_FILL, 3)) if noise else 0.0
    X1[k + PROJ_FILL:] = rng.normal(0, 4.0, (PROJ_OUTLIERS, 3))
    n = len(X2)
    cam = np.zeros((n, 2), np.int32)
    cam[k:, 0], cam[k:, 1] = np.arange(n - k) % 3, (np.arange(n - k) + 1) % 3
    return rig_pair(M_c, X1, X2, cam, [sigma2(i) for i in range(n)])


def lattice_draws(rng, n, iterations):
    d = rng.integers(0, n, (iterations, 3))
    d[0] = [0, 1, 2]
    return d


def projection_scene(name):
    def make():
        rng = np.random.default_rng(2205)
        M_c = M.rig_poses(3)
        pair = lattice_pair(rng, M_c, 0.05, lambda i: (SIG[i % 8], SIG[(5 * i + 2) % 8]))
        return scene(projection_rigs()[name], M_c, [pair], [(0.98, 15, PROJ_ITERATIONS)], draws=[lattice_draws(rng, len(pair["index1"]), PROJ_ITERATIONS)])
    return _once(("E", name), make)


REGIMES = ("on_axis", "behind", "grazing")


def regimes(m, h):
    """the transferred points of CheckInliers in their cameras' frames, both directions -> {regime: bool [N]}"""
    with np.errstate(all="ignore"):
        McInv = np.stack(m.McInv)
        out = {r: np.zeros(m.N, bool) for r in REGIMES}
        for T, X, cam in ((h["T12"], m.X2c, m.cam1), (h["T21"], m.X1c, m.cam2)):
            r = M._affine(McInv[cam], M._affine(T, X))
            norm = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
            out["on_axis"] |= norm == 0.0
            out["behind"] |= r[:, 2] < 0.0
            out["grazing"] |= (norm > 0.0) & (np.abs(r[:, 2]) / norm < 1e-6)
    return out


# ---- F: sigma^2 edges --------------------------------------------------------------------------------------------------------------------------------
def _around_one():
    """the two neighbouring doubles at 1 / 9.210 whose products with 9.210 fall below 1 and reach 1"""
    x = 1.0 / 9.210
    while 9.210 * x >= 1.0:
        x = math.nextafter(x, 0.0)
    return x, math.nextafter(x, 1.0)


SIGMA_DOWN, SIGMA_UP = _around_one()
SIGMA_EDGES = (0.1, SIGMA_DOWN, SIGMA_UP, 1e15, 1.0, SIG[7])   # thresholds 0, 0, 1, 9.21e15, 9, 118
SIGMA_ITERATIONS = 40


def sigma_scene():
    """the lattice pair without noise on the Lafida rig: the on-axis correspondences (3 .. 7) have err1 = err2 = 0 exactly under the quarter-turn hypothesis
    and take side-1 thresholds 0, 0, 1, 9.21e15, 9; the sides are mixed"""
    def make():
        rng = np.random.default_rng(2206)
        M_c = M.rig_poses(3)
        pair = lattice_pair(rng, M_c, 0.0, lambda i: (SIGMA_EDGES[(i - 3) % 6], SIGMA_EDGES[(5 * i + 1) % 6]))
        return scene(lafida(), M_c, [pair], [(0.98, 15, SIGMA_ITERATIONS)], draws=[lattice_draws(rng, len(pair["index1"]), SIGMA_ITERATIONS)])
    return _once("F", make)


REFUSED_SIGMA2 = (float("nan"), -1e-300, -1.0, -float("inf"), float("inf"), 2.0 ** 64 / 9.210 * (1 + 2.0 ** -50), 1e300)
LARGEST_SIGMA2 = 2.0 ** 64 / 9.210 * (1 - 2.0 ** -50)     # 9.210 * sigma2 just below 2^64: accepted


# ---- G: batch shape ------------------------------------------------------------------------------------------------------------------------------------
WORD_SIZES = (3, 63, 64, 65, 127, 128, 129)
MANY = 130
MANY_EMPTY, MANY_SHORT = 40, 77
MANY_CALLS = (1, 3, 5)


def word_scene():
    def make():
        rng = np.random.default_rng(2207)
        M_c = M.rig_poses(3)
        return scene(lafida(), M_c, [M.make_pair(rng, M_c, n, inlier_frac=0.6) for n in WORD_SIZES], [(0.98, 3, 40)] * len(WORD_SIZES), seed=2207)
    return _once("G/words", make)


def many_scene():
    """130 solvers with N in 3 .. 20 at (0.98, 6, 12); solver 40 has no correspondence at all, solver 77 has 4 (< minInliers)"""
    def make():
        rng = np.random.default_rng(2208)
        M_c = M.rig_poses(3)
        sizes = rng.integers(3, 21, MANY)
        sizes[MANY_SHORT] = 4
        pairs = [M.make_pair(rng, M_c, int(n), inlier_frac=0.9) for n in sizes]
        p = pairs[MANY_EMPTY]
        pairs[MANY_EMPTY] = dict(p, Xw=p["Xw"][:0], cam=p["cam"][:0], sigma2=p["sigma2"][:0], index1=p["index1"][:0], mN1=2)
        return scene(lafida(), M_c, pairs, [(0.98, 6, 12)] * MANY, seed=2208)
    return _once("G/many", make)


def slot_totals(sc, calls):
    """the hypotheses each iterate() call of run_rounds evaluates on the device: per call, the sum over the solvers that are not done of
    min(n, mRansacMaxIts - mnIterations).  Model only: runs the rounds on fresh models -> (totals, the models afterwards, near-threshold pairs seen)"""
    models = models_of(sc)
    done, totals, c, near = [False] * len(models), [], 0, 0
    while not all(done) and c < 400:
        n = calls[c % len(calls)]
        totals.append(sum(min(n, m.mRansacMaxIts - m.mnIterations) for m, d in zip(models, done) if not d and m.N >= m.mRansacMinInliers))
        for s, m in enumerate(models):
            if not done[s]:
                e = m.iterate(n, draws_of(sc, s))
                done[s], near = e[1], near + e[5]
        c += 1
    return totals, models, near


def one_camera_scene():
    def make():
        M_c = M.rig_poses(1)
        return scene(lafida()[:1], M_c, [M.make_pair(np.random.default_rng(2209), M_c, 30, inlier_frac=0.7)], [(0.98, 6, 40)], seed=2209)
    return _once("G/1", make)


def many_camera_scene():
    """nr_cams = 32 (kSim3MaxCams): the calibrations repeat, the correspondences are seen by cameras 0, 15 and 31"""
    def make():
        M32 = M.rig_poses(32)
        use = np.array([0, 15, 31])
        p = M.make_pair(np.random.default_rng(2210), [M32[c] for c in use], 40, inlier_frac=0.7)
        Mt_inv, MtMc_inv = pose_arrays(p["Mt"][0], p["Mt"][1], M32)
        pair = dict(p, cam=use[p["cam"]].astype(np.int32), M_t_inv=Mt_inv, MtMc_inv=MtMc_inv)
        return scene([lafida()[c % 3] for c in range(32)], M32, [pair], [(0.98, 6, 40)], seed=2210)
    return _once("G/32", make)


# ---- H: state ------------------------------------------------------------------------------------------------------------------------------------------
def state_scene():
    """generated draws: three solvers of different sizes"""
    def make():
        rng = np.random.default_rng(2211)
        M_c = M.rig_poses(3)
        return scene(lafida(), M_c, [M.make_pair(rng, M_c, n, inlier_frac=f) for n, f in ((24, 0.8), (40, 0.6), (70, 0.5))], [(0.98, 15, 300)] * 3, seed=2211)
    return _once("H", make)


# ("iterate", n) | ("params", (p, minInliers, maxIterations)) for every solver | ("refused", (...)): a SetRansacParameters the library must refuse
STATE_SCRIPT_DRAWS = [("iterate", 1), ("iterate", 1), ("iterate", 2),       # the NaN identity hypothesis becomes the best one through 0 >= 0, then the success
                      ("refused", (0.98, 15, 300)),                        # 201 iterations wanted, the caller's draws cover 60: refused, nothing changes
                      ("iterate", 3),
                      ("params", (0.98, 31, EXACT_ITERATIONS)), ("iterate", 20), ("iterate", 50),   # from iteration 0 again; the kept mnBestInliers (31) blocks the updates
                      ("params", (0.98, 66, EXACT_ITERATIONS)), ("iterate", 5),                     # minInliers > N: bNoMore at once
                      ("refused", (0.5, 10, 100)),
                      ("params", (0.98, 15, EXACT_ITERATIONS)), ("iterate", 2), ("iterate", 7), ("iterate", 60)]
STATE_SCRIPT_SEED = [("iterate", 3), ("iterate", 1), ("params", (0.98, 20, 300)), ("iterate", 10), ("params", (0.98, 71, 300)), ("iterate", 4),
                     ("params", (0.98, 15, 50)), ("iterate", 25), ("iterate", 300)]


def params_refused(sc, m, s, q):
    """mcs_sim3_set_ransac_parameters refuses iterations the caller's draws do not cover"""
    if sc["draws"] is None or m.N < q[1]:
        return False
    return M.ransac_max_its(q[0], q[1], q[2], m.N) > len(sc["draws"][s])


def compare_best(got, models, label):
    """mcs_sim3_best against the models: R, t, s, T12 under the hypothesis rule (zeros before the first update), best_inliers and iterations exactly"""
    R, t, s, T12, inl, it = got
    for k, m in enumerate(models):
        assert (int(inl[k]), int(it[k])) == (m.mnBestInliers, m.mnIterations), (label, k, inl[k], it[k], m.mnBestInliers, m.mnIterations)
        dev = np.concatenate([T12[k].reshape(16), R[k].reshape(9), t[k].reshape(3), [s[k]]])
        if m.best is None:
            assert (dev == 0.0).all(), (label, k)
        else:
            compare_doubles(dev, np.concatenate([m.best["T12"].reshape(16), m.best["R"].reshape(9), m.best["t"], [m.best["s"]]]), (label, k))


def drive_state(sc, script, device=None):
    """the script on fresh models and, in lockstep, on `device` (an object with iterate(n) -> the tuples of run_rounds, set_params(params) that raises where
    the library refuses, best() -> the arrays of mcs_sim3_best; None: the models alone).  -> (models, near-threshold pairs seen, refusals)"""
    models = models_of(sc)
    ns = len(models)
    near = refusals = 0
    for step, (what, arg) in enumerate(script):
        if what == "iterate":
            out = device.iterate(arg) if device else None
            for s, m in enumerate(models):
                e = m.iterate(arg, draws_of(sc, s))
                near += e[5]
                if device:
                    assert out[s][0] == e[0] and out[s][1] == e[1] and out[s][3] == e[3], (step, s, out[s][:2], out[s][3], e[:2], e[3])
                    assert np.array_equal(out[s][2], e[2]), (step, s)
                    if e[0]:
                        compare_doubles(out[s][4].reshape(16), e[4].reshape(16), (step, s))
        else:
            refused = any(params_refused(sc, m, s, arg) for s, m in enumerate(models))
            assert refused == (what == "refused"), (step, what)
            if device:
                try:
                    device.set_params([arg] * ns)
                    raised = False
                except Exception:
                    raised = True
                assert raised == refused, (step, what)
            if refused:
                refusals += 1
            else:
                for m in models:
                    m.SetRansacParameters(*arg)
        if device:
            compare_best(device.best(), models, step)
    return models, near, refusals


# ---- the comparisons -------------------------------------------------------------------------------------------------------------
def compare_doubles(got, want, label):
    """hypothesis doubles: NaN patterns equal, infinities equal, the finite values to 1e-9 relative of the largest finite one (at least 1)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (label, "NaN pattern", got, want)
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]) and not np.isinf(got[~inf & ~np.isnan(want)]).any(), (label, "infinities", got, want)
    fin = np.isfinite(want)
    if fin.any():
        assert np.allclose(got[fin], want[fin], rtol=1e-9, atol=1e-9 * max(1.0, np.abs(want[fin]).max())), (label, np.abs(got[fin] - want[fin]).max())


LENGTHS = np.zeros(45, bool)
LENGTHS[[3, 7, 11, 19, 23, 27, 41, 42, 43]] = True     # the translations of T12, T21 and t among the 45 doubles


def compare_hypotheses(m, draws, got, first, count, label, unit=1.0):
    """the device's mcs_sim3_hypotheses [first, first + count) against the model: picks exactly; masks bit for bit outside the pairs the model flags as within
    FLAG_BAND of a threshold, and the count off by no more than the number of flagged pairs; the 45 doubles by compare_doubles, lengths in units of `unit`
    (the scene's world scale).  -> flagged pairs seen"""
    picks, cnt, hyp, inl = got
    near_total = 0
    scale = np.where(LENGTHS, 1.0 / unit, 1.0)
    for i in range(count):
        k = first + i
        p, h, einl, near = m.evaluate(k, draws)
        assert list(picks[i]) == p, (label, k)
        assert cnt[i] == inl[i].sum()
        assert np.array_equal(inl[i] & ~near, einl & ~near), (label, k, np.flatnonzero(inl[i] != einl)[:10])
        assert abs(int(cnt[i]) - int(einl.sum())) <= int(near.sum()), (label, k, cnt[i], einl.sum(), near.sum())
        near_total += int(near.sum())
        with np.errstate(all="ignore"):
            compare_doubles(hyp[i] * scale, M.hyp_vector(h) * scale, (label, k))
    return near_total


def run_rounds(b, models, draws, sizes):
    """drive the batch and the models with the same call sizes (a list cycled over the calls) until every solver is done; -> calls made.  The decisions of
    iterate() are compared exactly, so the scene must not hold a pair within FLAG_BAND of its threshold: asserted on the model"""
    ns = len(models)
    done = [False] * ns
    calls = 0
    while not all(done) and calls < 400:
        n = sizes[calls % len(sizes)]
        nit = [0 if done[s] else n for s in range(ns)]
        out = b.iterate(nit)
        for s in range(ns):
            if done[s]:
                assert out[s][:2] == (False, False) and out[s][3] == 0
                continue
            e = models[s].iterate(n, draws[s])
            assert e[5] == 0, ("the model flags near-threshold pairs in this scene", calls, s, e[5])
            assert out[s][0] == e[0] and out[s][1] == e[1] and out[s][3] == e[3], (calls, s, out[s][:2], out[s][3], e[:2], e[3])
            assert np.array_equal(out[s][2], e[2]), (calls, s)
            if e[0]:
                assert np.allclose(out[s][4], e[4], rtol=1e-9, atol=1e-9)
            done[s] = e[1]
        calls += 1
    assert all(done)
    return calls
