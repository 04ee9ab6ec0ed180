"""Hostile frames for PoseOptimization (csrc/mcs_poseopt.hip): the table of scenes that tests/test_poseopt_hostile_cpu.py (the model
states every one of them, and the floors that keep a group from passing vacuously) and tests/test_gpu_hostile_poseopt.py (device == model) both walk.  Plain
module: numpy, poseopt_model and poseopt_scenes only, nothing of the device.

A scene is name -> (builder, kwargs) -> poseopt_model.Problem, as in poseopt_scenes; the name's first letter is its group.  Every seed was found over the
MODEL (tools/poseopt_seed_search.py --hostile prints the table): the scene shows its property and, unless EXCUSED names it, keeps every decision at least
poseopt_model.MARGIN from its edge.

  A  Levenberg-Marquardt control paths: all weights 0 (every solve fails), a negative weight (indefinite H), a failed solve that is ACCEPTED (it counts as
     chi2 = DBL_MAX, which is finite, and with the stale x the denominator of rho is negative, so rho > 0), far starts (rejected trials, every edge flagged
     by the first pass, STOP_NBAD), absorption (rho == 0 after one trial)
  B  Huber multipliers 0, 1e-300, 1e-3, 1e6, 1e200, inf, -1, NaN
  C  level weights inf, 1e308, 1e300, 1e-300, NaN; 1 and MCS_MAX_LEVELS levels
  D  projection geometry: points on the axis in front of and behind camera 0 and at its centre in a rig whose camera-frame point IS the world point, the
     stretched cameras of hostile_cameras with backward polynomials of degree 1 and MCS_MAX_POLY, points at grazing incidence
  E  magnitude: the world times 1e-6, 1e4, 1e8; points at (1e154, 1e154, 0) and (1e200, 0, 0); a point that overflows the first evaluation; Cayley parameters
     of 50; one map point seen by three cameras
  F  non-finite after the first evaluation: see below
  G  launch shape: rigs of 1 and 32 cameras, frames at the 65 536-feature cap, calls of 64 .. 129 problems that interleave the above with controls

THE FIRST EVALUATION'S SCREEN.  A problem is MCS_POSE_NONFINITE (not optimised) when, at the start pose, an edge's residual, Jacobian entry or
weight, the Huber pair (delta, delta^2) or one of the 28 reduced sums (H, b, chi2) is not finite.  So a NaN or infinite weight, a weight of 1e308 (chi2
overflows), the multipliers NaN, inf and 1e200 (delta^2 overflows) are that status, in the model and in the kernel alike; what a later evaluation does is
not screened.

ABSORPTION ("A.absorb") is excused from the margin rule and still exact.  One key at (3e38, -3e38) gives a robust chi2 near 1e39 for its edge; every other
edge's is below 1e5.  The sum of the others is below 1e8 < ulp(1e39) / 2 = 7.6e22 in whatever order they are added (all terms are >= 0, so every partial
sum that excludes the large term is below 1e8, and every partial sum that includes it rounds back to it).  The large term itself moves by less than
ulp / 2 under a step of a few pixels (the step changes the residual of 3e38 by ~1e0, 38 orders below it; float32 3e38 has a 64-bit ulp of 7.6e22 in
the product).  So current and trial chi2 are the SAME double by absorption, not by rounding luck: rho == 0, STOP_TRIALS after one trial, in any summation
order.  The margin metric reads 0 because it measures the distance of the two sums.

GROUP F.  Searched over the model (tools/poseopt_seed_search.py --late): the control (seeds 0 .. 9, starts 0.02, 3, 10, 30) under one or all level weights
of 1e290 .. 1e307, world scales 1e100 .. 1e153, one key of up to float32's maximum, Cayley starts of 1e3 .. 1e154 and one point of up to 1e307; 1 240 runs,
looking for one whose first evaluation passes the screen and whose later trial or build pass holds a non-finite sum (Result.late_nonfinite).  Found, all with a weight of 1e303
or 1e306 on one level (10 of the runs):
  "F.late_trial" (seed 2, start 10, pinned): nine TRIAL passes far from the start have chi2 = +inf; rho = -inf, each is rejected like any other trial and
  the run ends finite, every decision at least 0.71 from its edge.
  Seed 9, start 0.02, weight 1e303 or 1e306 (NOT pinned): four BUILD passes hold +inf in H, their solves fail, and with the stale x the scale of rho comes
  out negative, so rho = (chi - DBL_MAX) / scale > 0 and a failed solve is ACCEPTED at chi = DBL_MAX (g2o tests rho > 0 and isfinite(DBL_MAX)).  But the
  run is rounding noise from its fourth iteration on: the optimiser has driven the huge-weight edges to residuals of ONE ULP of their keys (chi2 ~ 1e140 is
  2 sqrt(w) delta ulp), and H overflows exactly in the passes where such a residual is 0.0, which makes the edge an inlier of weight w.  Whether z - u is
  0 or one ulp hangs on the last bit of atan (libm's here, another library's on the device); at 1e303 even the model's own reversed sums give another
  result (three failed solves, a pose 0.012 apart: test_the_build_pass_candidate_of_group_f_depends_on_the_summation_order).  No device result can be
  held to it, and the margin metric, which knows sums and thresholds, does not see it.  The search found no other build-pass case; none is constructed
  by other means."""
import importlib

import numpy as np

import hostile_cameras as HC
import poseopt_model as PM
import poseopt_scenes as S

synth = importlib.import_module("multicol-slam_amd.synth")

MAX_LEVELS, MAX_POLY, MAX_FEATURES = 16, 16, 65536       # MCS_MAX_LEVELS, MCS_MAX_POLY (include/mcs_c.h), the frame cap of mcs_pose_optimization
HUBERS = {"0": 0.0, "1e-300": 1e-300, "1e-3": 1e-3, "1e6": 1e6, "1e200": 1e200, "inf": np.inf, "-1": -1.0, "nan": np.nan}
WEIGHTS = {"inf": np.inf, "1e308": 1e308, "1e300": 1e300, "1e-300": 1e-300, "nan": np.nan}


def true_pose(seed):
    """the pose lafida_like_scene projected its keys at: its generator's first draws"""
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(0, 0.05, 3), rng.normal(0, 0.3, 3)])


def base(seed=1, n_edges=65, nr=2, **kw):
    """the control: poseopt_scenes' e65 at seed 1"""
    return S.scene(seed, n_edges, nr, **{"n_outliers": 5, "n_null": 30, **kw})


# ---- A
def weights_zero(seed=1):
    pr = base(seed)
    pr.inv_sigma2 = np.zeros_like(pr.inv_sigma2)
    return pr


def weight_at(seed=1, level=3, value=-1.0):
    pr = base(seed)
    pr.inv_sigma2 = pr.inv_sigma2.copy()
    pr.inv_sigma2[level] = value
    assert (pr.octave[pr.edges()] == level).any()
    return pr


def far_start(seed, start):
    return S.scene(seed, 65, 3, n_outliers=5, start=start)


def absorb(seed=1):
    pr = base(seed)
    pr.xy[pr.edges()[7]] = (3e38, -3e38)
    return pr


# ---- B
def huber(seed=1, value=1.0):
    pr = base(seed)
    pr.huber = float(value)
    return pr


# ---- C
def levels(seed, nlevels):
    return S.scene(seed, 65, 2, n_outliers=5, n_null=30, nlevels=nlevels)


# ---- D
def lattice_rig():
    """two Lafida cameras, camera 0 in the rig's origin: with a start pose of exactly 0 its camera-frame point is the world point, no rounding"""
    cams, Mc = S.rig(2)
    Mc = Mc.copy()
    Mc[0] = 0.0
    return cams, Mc


def lattice(seed, points):
    """a frame of the lattice rig started at pose exactly 0, a few centimetres from the pose its keys were projected at, whose first features of camera 0 hold
    the given camera-frame points; the keys of those are their projections at the START (plus noise), so each is an inlier there and the first step moves it
    off its special place"""
    cams, Mc = lattice_rig()
    pr = PM.lafida_like_scene(seed, 65, cams, Mc, n_outliers=5, n_null=30)
    rng = np.random.default_rng(500 + seed)
    pr.pose0 = np.zeros(6)
    near = np.concatenate([rng.normal(0, 0.006, 3), rng.normal(0, 0.02, 3)])
    u, v = PM.project(pr, near, np.arange(pr.n))
    xy = np.stack([u, v], 1) + rng.normal(0, 0.5, (pr.n, 2))
    bad = rng.choice(pr.edges(), 5, replace=False)
    xy[bad] += rng.normal(0, 25.0, (5, 2))
    idx = np.array([i for i in pr.edges() if pr.cam[i] == 0 and i not in bad][:len(points)])
    assert len(idx) == len(points)
    pr.pos[pr.points[idx]] = np.asarray(points, np.float64)
    u, v = PM.project(pr, pr.pose0, idx)
    xy[idx] = np.stack([u, v], 1) + rng.normal(0, 0.5, (len(idx), 2))
    pr.xy = xy.astype(np.float32)
    pr.special = idx
    return pr


def axis_front(seed):
    return lattice(seed, [(0.0, 0.0, 2.0)])


def axis_behind(seed):
    return lattice(seed, [(0.0, 0.0, -2.0)])


def centre(seed):
    return lattice(seed, [(0.0, 0.0, 0.0)])


def grazing(seed):
    """camera-frame z within 1e-12 of 0 at the start pose: theta = atan(-z / norm) within 1e-12 of 0 on either side"""
    return lattice(seed, [(1.5, 0.5, 1e-13), (-2.0, 1.0, -1e-13), (0.5, -3.0, 0.0), (1.0, 1.0, 9e-13), (-1.0, -2.0, -5e-13)])


def stretched_rig():
    """the stretched cameras of hostile_cameras at the Lafida image size, a backward polynomial of degree 1 (d rho / d theta is all zero) and one of degree
    MCS_MAX_POLY; rig poses from a fixed generator"""
    w, h = 754, 480
    cams = [HC.camera(n, w, h) for n in ("flipped", "short", "band160", "corner_br", "shrink")]
    lf = synth.lafida_cameras()
    cams.append(dict(lf[1], invP=list(lf[1]["invP"])[:1]))
    full = list(lf[2]["invP"]) + [0.75, -0.5, 0.25, -0.125]
    assert len(full) == MAX_POLY
    cams.append(dict(lf[2], invP=full))
    rng = np.random.default_rng(77)
    Mc = np.concatenate([rng.normal(0, 0.6, (len(cams), 3)), rng.normal(0, 0.15, (len(cams), 3))], 1)
    return cams, Mc


def stretched(seed, n_edges=130):
    cams, Mc = stretched_rig()
    return PM.lafida_like_scene(seed, n_edges, cams, Mc, n_outliers=8, n_null=30)


# ---- E
def scaled(seed, factor):
    """every length of the scene times `factor`: the keys do not change, the translations and the point table do"""
    pr = base(seed)
    pr.pos = pr.pos * factor
    pr.Mc_min = pr.Mc_min.copy()
    pr.Mc_min[:, 3:] *= factor
    pr.pose0 = pr.pose0.copy()
    pr.pose0[3:] *= factor
    return pr


def one_point(seed, X):
    pr = base(seed)
    pr.pos[pr.points[pr.edges()[11]]] = X
    return pr


def cayley50(seed):
    pr = base(seed)
    pr.pose0[:3] = 50.0
    return pr


def three_cameras(seed):
    """one map point held by a feature of each of the three cameras, every key its projection (plus noise)"""
    pr = S.scene(seed, 65, 3, n_outliers=5, n_null=30)
    e = pr.edges()
    i = [int(e[pr.cam[e] == c][2]) for c in range(3)]
    pr.points[i[1]] = pr.points[i[2]] = pr.points[i[0]]
    u, v = PM.project(pr, true_pose(seed), np.array(i))
    rng = np.random.default_rng(900 + seed)
    pr.xy[i] = (np.stack([u, v], 1) + rng.normal(0, 0.5, (3, 2))).astype(np.float32)
    pr.special = np.array(i)
    return pr


# ---- F
def late(seed, start, weight=1e303):
    pr = base(seed, start=start)
    pr.inv_sigma2 = pr.inv_sigma2.copy()
    pr.inv_sigma2[3] = weight
    return pr


# ---- G
def one_camera(seed):
    return S.scene(seed, 65, 1, n_outliers=5, n_null=30)


def rig32():
    lf = synth.lafida_cameras()
    rng = np.random.default_rng(32)
    return [lf[c % 3] for c in range(32)], np.concatenate([rng.normal(0, 0.8, (32, 3)), rng.normal(0, 0.2, (32, 3))], 1)


def cameras32(seed):
    cams, Mc = rig32()
    pr = PM.lafida_like_scene(seed, 200, cams, Mc, n_outliers=15, n_null=40)
    assert len(set(pr.cam[pr.edges()].tolist())) == 32
    return pr


def at_the_cap(seed, where):
    """a frame of 65 536 features, 65 of them edges: "tail" spreads them over the last 512 indices, "stride" puts them at multiples of 512 (one thread of the
    workgroup owns every edge)"""
    src = S.scene(seed, 65, 2, n_outliers=5)
    n = MAX_FEATURES
    at = (n - 512 + np.sort(np.random.default_rng(seed).choice(512, 65, replace=False))) if where == "tail" else 512 * np.arange(65)
    pr = PM.Problem(np.zeros((n, 2), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.full(n, -1, np.int32), src.pos, src.Mc_min, src.cams,
                    src.inv_sigma2, src.pose0, 1.0)
    pr.xy[at], pr.octave[at], pr.cam[at], pr.points[at] = src.xy, src.octave, src.cam, src.points
    return pr


SCENES = {
    "A.weights_zero": (weights_zero, dict(seed=1)),
    "A.weight_negative": (weight_at, dict(seed=1, level=3, value=-1.0)),
    "A.accepted_failure": (weight_at, dict(seed=7, level=3, value=-1.0)),      # found over seeds 0 .. 15 of the negative weights and multiplier
    "A.far3": (far_start, dict(seed=1, start=3)),
    "A.far10": (far_start, dict(seed=0, start=10)),
    "A.far30": (far_start, dict(seed=0, start=30)),
    "A.absorb": (absorb, dict(seed=1)),
    **{"B.huber_" + k: (huber, dict(seed=4 if k == "1e6" else 1, value=v)) for k, v in HUBERS.items()},             # 1e6: margin 2e-8 at seed 1
    **{"C.weight_" + k: (weight_at, dict(seed=2 if k == "1e300" else 1, level=3, value=v)) for k, v in WEIGHTS.items()},   # 1e300: margin 1e-8 at seed 1
    "C.levels_1": (levels, dict(seed=1, nlevels=1)),
    "C.levels_max": (levels, dict(seed=1, nlevels=MAX_LEVELS)),
    "D.axis_front": (axis_front, dict(seed=0)),
    "D.axis_behind": (axis_behind, dict(seed=0)),
    "D.centre": (centre, dict(seed=0)),
    "D.grazing": (grazing, dict(seed=0)),
    "D.stretched": (stretched, dict(seed=0)),
    "E.scale_1e-6": (scaled, dict(seed=1, factor=1e-6)),
    "E.scale_1e4": (scaled, dict(seed=1, factor=1e4)),
    "E.scale_1e8": (scaled, dict(seed=1, factor=1e8)),
    "E.point_1e154": (one_point, dict(seed=1, X=(1e154, 1e154, 0.0))),
    "E.point_1e200": (one_point, dict(seed=1, X=(1e200, 0.0, 0.0))),
    "E.point_overflow": (one_point, dict(seed=1, X=(1e308, 1e308, 1e308))),
    "E.cayley50": (cayley50, dict(seed=1)),
    "E.three_cameras": (three_cameras, dict(seed=0)),
    "F.late_trial": (late, dict(seed=2, start=10)),
    "G.one_camera": (one_camera, dict(seed=0)),
    "G.cameras32": (cameras32, dict(seed=0)),
    "G.cap_tail": (at_the_cap, dict(seed=0, where="tail")),
    "G.cap_stride": (at_the_cap, dict(seed=0, where="stride")),
}
# name -> why no margin is asked of it.  At most one scene in five, never a whole group (tests/test_poseopt_hostile_cpu.py).
EXCUSED = {
    "A.absorb": "rho == 0 by absorption: the two sums are the same double in any order (module docstring); the metric measures their distance",
    "D.axis_front": "the on-axis point's Jacobian is ~1e14 px per unit, lambda ~1e18 and the second iteration's steps move chi2 by 1e-12 of itself: the trial "
                    "count is rounding noise (margins 6e-12 .. 2e-9 on seeds 0 .. 7); the flags are off their edge (Result.flag_margin)",}
# the scenes whose status is MCS_POSE_NONFINITE by the first evaluation's screen
NONFINITE = ("B.huber_1e200", "B.huber_inf", "B.huber_nan", "C.weight_inf", "C.weight_1e308", "C.weight_nan", "E.point_overflow")


def groups():
    out = {}
    for n in SCENES:
        out.setdefault(n[0], []).append(n)
    return out


_cache = {}


def build(name):
    fn, kw = SCENES[name]
    return fn(**kw)


def model(name, reverse=False):
    """the model's result for a named scene, computed once and shared (callers do not modify it)"""
    if (name, reverse) not in _cache:
        _cache[name, reverse] = PM.optimize(build(name), reverse=reverse)
    return _cache[name, reverse]


def rel(a, b):
    """largest difference of two arrays relative to max(1, |component|); NaN and infinities must sit in the same places with the same sign"""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin], b[~fin], equal_nan=True):
        return np.inf
    return float(np.max(np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin])), initial=0.0))


def spread(name):
    """S.spread's construction, per scene and relative: the model with its edge sums in index order against reversed order, over pose, matrices, lambda, chi2"""
    a, b = model(name), model(name, reverse=True)
    return max(rel(a.pose, b.pose), rel(a.MtMc, b.MtMc), rel(a.MtMc_inv, b.MtMc_inv), rel(a.lam, b.lam), rel(a.chi2, b.chi2))


# ---- G: the interleaved calls.  One call shares rig, cameras and level weights, so the members are the scenes built on the control's rig and weights.
INTERLEAVED = ("B.huber_0", "A.absorb", "B.huber_nan", "E.point_1e154", "B.huber_-1", "E.point_overflow", "B.huber_1e-3", "E.cayley50", "B.huber_inf",
               "E.point_1e200", "B.huber_1e6", "B.huber_1e-300", "B.huber_1e200")
BATCH_SIZES = (64, 65, 128, 129)


def interleaved(n):
    """-> [(name or None for a control, Problem)] of n problems: control, hostile, control, hostile, ... with two different controls"""
    controls = [base(1), base(4)]
    out = []
    for k in range(n):
        if k % 2 == 0:
            out.append((None, controls[(k // 2) % 2]))
        else:
            name = INTERLEAVED[(k // 2) % len(INTERLEAVED)]
            out.append((name, build(name)))
    return out


HOSTILE_LEVELS = {3: -1.0, 5: 1e-300, 6: 1e300}     # the weights of A and C that leave the status 0, as one call's table


def weight_interleaved(n):
    """-> [(kind, Problem)] of n problems under ONE level table that holds the hostile weights above: the controls' edges avoid those levels (their octaves
    are moved to a neighbouring level), every hostile problem keeps exactly one of them"""
    table = base(1).inv_sigma2.copy()
    for lv, w in HOSTILE_LEVELS.items():
        table[lv] = w
    out = []
    for k in range(n):
        pr = base(1 + (k // 2) % 3)
        keep = None if k % 2 == 0 else list(HOSTILE_LEVELS)[(k // 2) % 3]
        for lv in HOSTILE_LEVELS:
            if lv != keep:
                pr.octave[pr.octave == lv] = {3: 2, 5: 4, 6: 7}[lv]
        pr.inv_sigma2 = table
        used = set(pr.octave[pr.edges()].tolist()) & set(HOSTILE_LEVELS)
        assert used == (set() if keep is None else {keep})
        out.append(("control%d" % (1 + (k // 2) % 3) if keep is None else "level%d_%d" % (keep, 1 + (k // 2) % 3), pr))
    return out


def huber_batch():
    """every multiplier of B as one call, one value per problem, beside two controls at 1"""
    return [("control", base(1))] + [("B.huber_" + k, build("B.huber_" + k)) for k in HUBERS] + [("control", base(1))]
