"""Hostile map points, rigs and slot states for the TrackLocalMap frustum search (csrc/mcs_frustum.hip): the table of cases that
tests/test_frustum_hostile_cpu.py (an independent scalar statement, hand-derived answers, every non-vacuity predicate) and tests/test_gpu_hostile_frustum.py
(device == model, both memory kinds) both walk.  Plain module: numpy, frustum_model and the oracle behind it, nothing of the device.

A case is a dict: name, group, scene = (pts, rig, state, desc, mask, frame, assigned) as frustum_model.make_scene returns it, scales (= frame["scales"]), check
(a predicate over the MODEL's output that shows the branch the case is meant to reach is reached), exact (proj_x / proj_y must be bit-equal, 100 %), and
host = None or the word of the message a host-kind call is refused with (the device kind runs the case).

THE EXACT RIG.  Camera models with a backward polynomial of degree 1 (rho = invP[0] whatever theta is, as long as it is finite) and c = 1, d = e = 0, on
MtMc = MtMc_inv = identity plus small exact translations: u = x / norm * rho + u0, v = y / norm * rho + v0, no atan.  A point on the optical axis (x = y = 0,
norm -> 1e-14) has u = u0 and v = v0 EXACTLY, whatever rho: the rounding cases place their values through u0 / v0 this way (-0.0 alone cannot be placed:
0 * 1 + 0 * 0 + -0.0 is +0.0, which rounds like it).  A point (3k, 0, 4k) has norm = 3k, u = rho + u0, v = v0, dist = 5k.  Everything on this rig is the
same IEEE operations in the model and on the device, so every case on it is held bit for bit.

THE MODEL of an out-of-range stale level is the library's documented rule (include/mcs_c.h): such a slot is not searched (the reference would index
mvScaleFactors out of bounds); host-kind calls refuse the call instead."""
import importlib
import math

import numpy as np

import frustum_model as M
import oracle_lib as O
from hostile_windows import cv_round

MAX_LEVELS, MAX_CAMS = 16, 32          # MCS_MAX_LEVELS (include/mcs_c.h), the rig guard of mcs_frustum
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
NAN, INF = float("nan"), float("inf")
SW, SH = 64, 48                        # the small image of the rounding cases (masks of 3 KiB)
BW, BH = 640, 480                      # the image of every other exact-rig case
FLAG_BYTES = (0, 1, 2, 3, 4, 6, 0x80, 0xFE, 0xFF)
SLOT_SHAPES = ((1, 1), (21, 3), (32, 2), (13, 5), (51, 5), (32, 8), (257, 1), (171, 3), (2, 32))    # npoints x nr_cams: 1, 63, 64, 65, 255, 256, 257, 513, 64 slots


def std_scales(n=8):
    """mvScaleFactors as the extractor forms them: products of the float 1.2 widened"""
    sc = [1.0]
    for _ in range(1, n):
        sc.append(sc[-1] * float(np.float32(1.2)))
    return np.array(sc)


# ---------------------------------------------------------------------------------------------- builders
def exact_cam(u0, v0, rho, W, H):
    return dict(c=1.0, d=0.0, e=0.0, u0=float(u0), v0=float(v0), p=[1.0], invP=[float(rho)], width=W, height=H)


def exact_rig(cams, centres=None, masks=None):
    """camera c at `centres[c]` (default: the origin), axes the world's"""
    MtMc = []
    for c in range(len(cams)):
        T = np.eye(4)
        if centres is not None:
            T[:3, 3] = centres[c]
        MtMc.append(T)
    return dict(cams=list(cams), MtMc=MtMc, MtMc_inv=[M.inv_mat(T) for T in MtMc], masks=masks)


def big_rig(nr, rho=100.0, spread=0.25):
    """nr cameras 640 x 480 a quarter of a unit apart along x: every direction projects inside the image (|u - 320| <= 100)"""
    return exact_rig([exact_cam(320.0, 240.0, rho, BW, BH) for _ in range(nr)], [(spread * c, 0.0, 0.0) for c in range(nr)])


def points(pos, min_dist, max_dist, flags=None, normal=None):
    n = len(pos)
    full = lambda v: np.full(n, v, np.float64) if np.isscalar(v) else np.array(v, np.float64)
    return dict(pos=np.ascontiguousarray(np.array(pos, np.float64).reshape(n, 3)),
                normal=np.tile([0.0, 0.0, 1.0], (n, 1)) if normal is None else np.ascontiguousarray(np.array(normal, np.float64).reshape(n, 3)),
                min_dist=full(min_dist), max_dist=full(max_dist), flags=np.zeros(n, np.uint8) if flags is None else np.array(flags, np.uint8))


def garbage_state(n, nr):
    """what an unskipped slot must overwrite or leave: recognisable values"""
    st = M.new_state(n, nr)
    st["proj_x"][:], st["proj_y"][:], st["level"][:], st["view_cos"][:] = -777.25, -555.5, -5, -3.5
    return st


def descriptors(n, dim, seed):
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    m = np.full((n, dim), 0xFF, np.uint8)
    m[rng.random((n, dim)) < 0.1] = 0xF7
    return d, m


def make_frame(cams, scales, targets, dim, seed, extra=6):
    """a frame of the rig `cams`: one feature per target (cam, x, y, octave, desc row, mask row) plus `extra` random ones per camera, grouped by camera in
    target order (mvKeys order decides ties)"""
    rng = np.random.default_rng(seed)
    nr, nl = len(cams), len(scales)
    rows = list(targets)
    for c in range(nr):
        d, m = descriptors(extra, dim, seed * 1000 + c)
        for k in range(extra):
            rows.append((c, rng.uniform(1, cams[c]["width"] - 1), rng.uniform(1, cams[c]["height"] - 1), int(rng.integers(0, nl)), d[k], m[k]))
    rows.sort(key=lambda r: r[0])
    n = len(rows)
    keys = np.zeros(n, O.KP_DTYPE)
    keys["x"], keys["y"], keys["octave"] = [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]
    keys["size"], keys["angle"], keys["class_id"] = 31.0, 0.0, -1
    return dict(keys=keys, desc=np.ascontiguousarray(np.stack([r[4] for r in rows])), mask=np.ascontiguousarray(np.stack([r[5] for r in rows])),
                cam=np.array([r[0] for r in rows], np.int32), width=np.array([c["width"] for c in cams], np.int32),
                height=np.array([c["height"] for c in cams], np.int32), scales=np.array(scales, np.float64), n=n, nr=nr, cams=list(cams))


def flip(row, nbits, seed):
    """`row` with nbits distinct bits flipped"""
    out = row.copy()
    for b in np.random.default_rng(seed).choice(8 * len(row), nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def scene_with_features(pts, rig, scales, state, dim=32, seed=1, stale_targets=True, per_slot=1, near=0.0, extra=6, assigned_share=0.0):
    """the scene whose frame holds, for every slot the model brings into view (and every stale in-view slot with a finite projection and a level inside the
    pyramid), `per_slot` features at its projection (+- near px) at its level, carrying the point's descriptor with 8 * k bits flipped"""
    n, nr = len(pts["pos"]), len(rig["cams"])
    desc, mask = descriptors(n, dim, seed)
    st, vis, ntm, fresh = M.frustum(pts, rig, scales, state)
    rng = np.random.default_rng(seed + 77)
    targets = []
    for i in range(n):
        for c in range(nr):
            if not st["in_view"][i, c] or not (fresh[i, c] or stale_targets):
                continue
            x, y, lv = float(st["proj_x"][i, c]), float(st["proj_y"][i, c]), int(st["level"][i, c])
            if not (math.isfinite(x) and math.isfinite(y) and abs(x) < 1e6 and abs(y) < 1e6 and 0 <= lv < len(scales)):
                continue
            for k in range(per_slot):
                targets.append((c, x + rng.uniform(-near, near), y + rng.uniform(-near, near), lv if k % 2 == 0 else max(lv - 1, 0),
                                flip(desc[i], min(8 * k, 8 * dim - 1), seed + k), mask[i]))
    F = make_frame(rig["cams"], scales, targets, dim, seed, extra)
    assigned = (np.random.default_rng(seed + 5).random(F["n"]) < assigned_share).astype(np.uint8)
    return pts, rig, state, desc, mask, F, assigned


CASES = {}          # name -> builder
_built, _model = {}, {}


def case(name, host=None, exact=True):
    def deco(fn):
        def build():
            scene, check = fn()
            return dict(name=name, group=name.split(".")[0], scene=scene, scales=scene[5]["scales"], check=check, exact=exact, host=host)
        assert name not in CASES, name
        CASES[name] = build
        return fn
    return deco


def get(name):
    if name not in _built:
        _built[name] = CASES[name]()
    return _built[name]


def groups():
    out = {}
    for n in CASES:
        out.setdefault(n.split(".")[0], []).append(n)
    return out


# ---------------------------------------------------------------------------------------------- the model
def searchable_state(state, nlevels):
    """the fields SearchByProjection may read: an in-view slot whose level lies outside the pyramid is not searched (include/mcs_c.h)"""
    st = M.copy_state(state)
    st["in_view"][(st["level"] < 0) | (st["level"] >= nlevels)] = 0
    return st


def search_on_fields(scene, state, th=3.0, nnratio=0.8, desc_masks=True):
    """frustum_model.search_on_state on given fields under the level rule -> (nmatches, match, assigned after)"""
    pts, rig, st0, desc, mask, F, assigned = scene
    asg = np.ascontiguousarray(assigned, np.uint8).copy()
    nm, match = M.search_on_state(pts, searchable_state(state, len(F["scales"])), desc, mask if desc_masks else None, F, asg, th, nnratio)
    return nm, match, asg


def run_model(scene, th=3.0, nnratio=0.8, desc_masks=True):
    """src/cTracking.cpp:978-1011 as frustum_model.search_local_points states it, under the level rule"""
    pts, rig, st0, desc, mask, F, assigned = scene
    st, vis, ntm, fresh = M.frustum(pts, rig, F["scales"], st0)
    nm, match, asg = 0, np.full(st["in_view"].shape, -1, np.int32), np.ascontiguousarray(assigned, np.uint8).copy()
    if ntm > 0:
        nm, match, asg = search_on_fields(scene, st, th, nnratio, desc_masks)
    return dict(state=st, visible_inc=vis, n_to_match=ntm, fresh=fresh, match=match, nmatches=nm, assigned=asg)


def model(name, desc_masks=True):
    """the model's output for a named case, computed once and shared (callers do not modify it)"""
    if (name, desc_masks) not in _model:
        _model[name, desc_masks] = run_model(get(name)["scene"], desc_masks=desc_masks)
    return _model[name, desc_masks]


def searched(scene, out):
    """[n][nr] bool: the slots the search visits"""
    pts, F = scene[0], scene[5]
    if out["n_to_match"] == 0:
        return np.zeros(out["state"]["in_view"].shape, bool)
    return (searchable_state(out["state"], len(F["scales"]))["in_view"] != 0) & ((pts["flags"] & M.LP_BAD) == 0)[:, None]


# ---------------------------------------------------------------------------------------------- bounds
def up(v):
    return math.nextafter(v, INF)


def down(v):
    return math.nextafter(v, -INF)


# (min_dist, max_dist, in view, level) at dist = 5 exactly, 8 standard levels (1.2^7 = 3.58: a ratio above it is clamped to 7)
BOUND_ROWS = [
    (5.0, 9.0, 1, 0),            # dist == minDistance: `<` is false; ratio 1.0 == factor 0
    (up(5.0), 9.0, 0, None),     # one ulp too near
    (down(5.0), 9.0, 1, 1),      # ratio one ulp above 1.0: the next factor
    (1.0, 5.0, 1, 7),            # dist == maxDistance: `>` is false
    (1.0, down(5.0), 0, None),   # one ulp too far
    (1.0, up(5.0), 1, 7),
    (5.0, 5.0, 1, 0),            # the interval is one point
    (6.0, 4.0, 0, None),         # max < min around dist
    (4.0, 3.0, 0, None),         # max < min below dist
    (7.0, 6.0, 0, None),         # max < min above dist
    (1.0, INF, 1, 7),
    (0.0, 9.0, 1, 7),            # ratio +inf: end(), clamped
    (-0.0, 9.0, 1, 0),           # ratio -inf
    (-1.0, 9.0, 1, 0),           # ratio -5
    (5e-324, 9.0, 1, 7),         # the quotient overflows
    (INF, 9.0, 0, None),
    (NAN, 9.0, 1, 0),            # `dist < NaN` is false; NaN ratio: begin()
    (1.0, NAN, 1, 7),            # `dist > NaN` is false
    (NAN, NAN, 1, 0),
    (INF, INF, 0, None),
    (4.0, 2.5e-323, 0, None),
]


@case("bounds.distance_edges")
def _bounds():
    # camera 0 at the origin, camera 1 at (6, 0, 8): the point (3, 0, 4) is (3, 0, 4) and (-3, 0, -4) in them, dist = sqrt((0 + 9) + 0 + 16) = 5 in both
    rig = exact_rig([exact_cam(320.0, 240.0, 100.0, BW, BH)] * 2, [(0.0, 0.0, 0.0), (6.0, 0.0, 8.0)])
    n = len(BOUND_ROWS)
    pts = points([[3.0, 0.0, 4.0]] * n, [r[0] for r in BOUND_ROWS], [r[1] for r in BOUND_ROWS])
    scene = scene_with_features(pts, rig, std_scales(), garbage_state(n, 2))

    def check(out):
        st = out["state"]
        for c, u in ((0, 420.0), (1, 220.0)):      # u = +-1 * rho + u0, v = v0: exact
            assert st["in_view"][:, c].tolist() == [r[2] for r in BOUND_ROWS], c
            for i, r in enumerate(BOUND_ROWS):
                if r[2]:
                    assert (st["proj_x"][i, c], st["proj_y"][i, c], st["level"][i, c]) == (u, 240.0, r[3]), (i, c)
                else:
                    assert (st["proj_x"][i, c], st["level"][i, c]) == (-777.25, -5), (i, c)     # a rejected slot keeps its other fields
        assert st["view_cos"][0, 0] == 4.0 / 5.0 and st["view_cos"][0, 1] == -4.0 / 5.0
    return scene, check


# ---------------------------------------------------------------------------------------------- levels
def quotient_pair(s):
    """(dist, min_dist) with fl(dist / min_dist) == s bit for bit: from fl(s * min_dist), one nextafter step at a time; a min_dist whose quotients step over
    s (they are up to 4 / 3 ulp apart) is given up for the next one"""
    for min_dist in (3.0, 5.0, 7.0, 1.5, 2.5, 6.0, 0.75):
        lo = hi = s * min_dist
        for _ in range(9):
            for cand in (lo, hi):
                if M.fdiv(cand, min_dist) == s:
                    return cand, min_dist
            lo, hi = down(lo), up(hi)
    raise AssertionError("no (dist, min_dist) with quotient %r" % s)


def quotient_neighbours(d, min_dist, s):
    """the nearest doubles below and above d whose quotient is no longer s"""
    lo = d
    while M.fdiv(lo, min_dist) == s:
        lo = down(lo)
    hi = d
    while M.fdiv(hi, min_dist) == s:
        hi = up(hi)
    return lo, hi


def axis_scene(dists, min_dist, max_dist, scales, seed=2, **kw):
    """points on the optical axis of the one camera at the origin: dist = z exactly, u = u0, v = v0"""
    rig = exact_rig([exact_cam(320.0, 240.0, 100.0, BW, BH)])
    pts = points([[0.0, 0.0, z] for z in dists], min_dist, max_dist)
    return scene_with_features(pts, rig, scales, garbage_state(len(dists), 1), seed=seed, **kw)


@case("levels.quotient_equals_a_factor")
def _levels_quotient():
    sc = std_scales()
    dists, mins, want = [], [], []
    for k, s in enumerate(sc.tolist()):
        d, m = quotient_pair(s)
        lo, hi = quotient_neighbours(d, m, s)
        if k == 0:
            lo = d                                                # below factor 0 the point is too near: dist == minDistance twice
        dists += [lo, d, hi]
        mins += [m] * 3
        want += [k, k, min(k + 1, 7)]                             # lower_bound: the first factor that is not < ratio
    scene = axis_scene(dists, mins, 100.0, sc)

    def check(out):
        for k, s in enumerate(sc.tolist()):
            q = [M.fdiv(dists[3 * k + j], mins[3 * k]) for j in range(3)]
            assert q[1] == s and q[2] > s and (k == 0 or sc[k - 1] < q[0] < s), (k, q)
        assert out["state"]["in_view"][:, 0].all() and out["state"]["level"][:, 0].tolist() == want
    return scene, check


@case("levels.ratio_zero_inf_nan")
def _levels_special():
    #        dist  min   max   level
    rows = [(0.0, -1.0, 9.0, 0),        # ratio -0.0 (the only zero a point in range can have: dist >= minDistance)
            (0.0, -INF, 9.0, 0),        # 0 / -inf = -0.0
            (4.0, 0.0, 9.0, 7),         # +inf
            (4.0, -0.0, 9.0, 0),        # -inf
            (0.0, 0.0, 9.0, 0),         # 0 / 0 = NaN: begin()
            (4.0, NAN, 9.0, 0),
            (0.0, -0.0, 9.0, 0)]
    scene = axis_scene([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], std_scales())

    def check(out):
        st = out["state"]
        assert st["in_view"][:, 0].all() and st["level"][:, 0].tolist() == [r[3] for r in rows]
        assert np.isnan(st["view_cos"][[0, 1, 4, 6], 0]).all() and st["view_cos"][2, 0] == 1.0        # dist == 0: 0 / 0
        ratios = [M.fdiv(r[0], r[1]) for r in rows]
        assert ratios[0] == 0.0 and ratios[2] == INF and ratios[3] == -INF and math.isnan(ratios[4]) and math.isnan(ratios[5])
    return scene, check


def sweep_case(name, table):
    """ratios on both sides of and exactly at every finite entry of `table` (min_dist = 2: dist = 2 * s is exact), and far outside"""
    table = np.array(table, np.float64)
    fin = sorted(set(float(s) for s in table if math.isfinite(s) and s > 0))
    ratios = [0.75, 1e-3, 1e6]
    for s in fin:
        ratios += [s, down(s), up(s), s * 1.03, s * 0.97]
    ratios = [r for r in ratios if r >= 0.51]                     # dist >= minDistance / 2 is chosen below

    @case(name)
    def _build():
        dists = [2.0 * r for r in ratios]
        scene = axis_scene(dists, 2.0, INF, table)
        # a point too near (ratio < 1 is only reachable with a table below 1): give those points min_dist through max alone
        scene[0]["min_dist"][:] = 2.0
        scene[0]["max_dist"][:] = INF

        def check(out):
            st = out["state"]
            inside = np.array([2.0 * r >= 2.0 for r in ratios])
            assert np.array_equal(st["in_view"][:, 0].astype(bool), inside)
            lv = st["level"][inside, 0]
            want = [min(M.lower_bound(table.tolist(), M.fdiv(2.0 * r, 2.0)), len(table) - 1) for r, k in zip(ratios, inside) if k]
            assert lv.tolist() == want
            assert len(set(want)) >= min(2, len(table)), want
            rin = [r for r, k in zip(ratios, inside) if k]
            if name.split("_", 1)[1] in ("descending", "nan_inside", "unsorted"):      # the bisection, not a count of the smaller factors
                assert any(w != naive_level(table.tolist(), r) for w, r in zip(want, rin)), name
            if name.endswith("equal"):                                                  # a ratio equal to a repeated factor: its first index
                assert [w for w, r in zip(want, rin) if r == 1.5] == [3] and [w for w, r in zip(want, rin) if r == 2.0] == [6]
        return scene, check
    return ratios


sweep_case("levels.nlevels_1", [1.0])
sweep_case("levels.nlevels_2", std_scales(2))
sweep_case("levels.nlevels_8", std_scales(8))
sweep_case("levels.nlevels_max", std_scales(MAX_LEVELS))
EQUAL_TABLE = [1.0, 1.25, 1.25, 1.5, 1.5, 1.5, 2.0, 2.0]
DESCENDING_TABLE = [4.0, 3.5, 3.0, 2.5, 2.0, 1.5, 1.25, 1.0]
NAN_TABLE = [1.0, 1.25, 1.5, NAN, 2.0, 2.5, 3.0, 3.5]
INF_TABLE = [1.0, 1.25, 1.5, 2.0, 2.5, 3.0, INF]
UNSORTED_TABLE = [1.0, 3.0, 1.5, 2.5, 1.25, 3.5, 2.0, 4.0, 1.1]
for _n, _t in (("equal", EQUAL_TABLE), ("descending", DESCENDING_TABLE), ("nan_inside", NAN_TABLE), ("ends_in_inf", INF_TABLE), ("unsorted", UNSORTED_TABLE)):
    sweep_case("levels.table_" + _n, _t)


def naive_level(table, v):
    """what a linear count of the smaller factors would give: the bisection differs from it on a table that is not ascending"""
    return min(sum(1 for s in table if s < v), len(table) - 1)


# ---------------------------------------------------------------------------------------------- rounding
ROUND_VALUES = {"0.5": 0.5, "1.5": 1.5, "2.5": 2.5, "W-1.5": None, "W-0.5": None, "W-0.49": None, "-0.0": -0.0, "1e-300": 1e-300, "2^31-0.5": 2.0 ** 31 - 0.5,
                "2^31": 2.0 ** 31, "-2^31-1": -2.0 ** 31 - 1, "1e300": 1e300, "-1e300": -1e300, "inf": INF, "-inf": -INF, "nan": NAN,
                "2^32+5": 2.0 ** 32 + 5, "-2^32+5": -2.0 ** 32 + 5, "2^63": 2.0 ** 63}      # the last three: what (int)lrint() and a saturating conversion disagree on
ROUND_CHUNK = 7


def round_value(name, size):
    v = ROUND_VALUES[name]
    return v if v is not None else {"W-1.5": size - 1.5, "W-0.5": size - 0.5, "W-0.49": size - 0.49}[name]


# hand-derived: which values land inside (0 < rint < size), and on which pixel
ROUND_INSIDE = {"1.5": 2, "2.5": 2, "W-1.5": -2}        # -2: size - 2 (size - 1.5 ties to the even size - 2 for the even sizes used here)


def rounding_case(axis, chunk, mode):
    names = list(ROUND_VALUES)[chunk * ROUND_CHUNK:(chunk + 1) * ROUND_CHUNK]
    nr = len(names)
    size, mid = (SW, 24.0) if axis == "u" else (SH, 32.0)

    def build():
        vals = [round_value(k, size) for k in names]
        cams = [exact_cam(v, mid, 8.0, SW, SH) if axis == "u" else exact_cam(mid, v, 8.0, SW, SH) for v in vals]
        target = [(int(cv_round(c["u0"])), int(cv_round(c["v0"]))) for c in cams]      # the pixel of the on-axis point, by the x86 rule
        inb = [0 < t[0] < SW and 0 < t[1] < SH for t in target]
        masks = None
        if mode != "bounds":
            masks = []
            for c in range(nr):
                m = np.zeros((SH, SW), np.uint8) if mode != "dead" else np.full((SH, SW), 255, np.uint8)
                if inb[c]:
                    m[target[c][1], target[c][0]] = 0 if mode == "dead" else 255
                masks.append(None if (mode == "mixed" and c % 2 == 1) else m)
        rig = exact_rig(cams, None, masks)
        # point 0 on the axis: u = u0, v = v0 exactly.  Point 1 = (3, 0, 4) / (0, 3, 4): u = 8 + u0 resp. v = 8 + v0, eight pixels on (further ties).
        pts = points([[0.0, 0.0, 4.0], [3.0, 0.0, 4.0] if axis == "u" else [0.0, 3.0, 4.0]], 3.5, 9.0)
        scene = scene_with_features(pts, rig, std_scales(), garbage_state(2, nr), seed=3)

        def check(out):
            st = out["state"]
            for c, k in enumerate(names):
                want = ROUND_INSIDE.get(k)
                pix = None if want is None else (want if want > 0 else size + want)
                assert inb[c] == (pix is not None) and (pix is None or target[c][0 if axis == "u" else 1] == pix), (k, target[c])
                masked = masks is not None and masks[c] is not None
                live0 = inb[c] and (not masked or mode == "live" or mode == "mixed")
                assert st["in_view"][0, c] == live0, (k, mode)
                if live0:
                    got = st["proj_x"][0, c] if axis == "u" else st["proj_y"][0, c]
                    assert got == vals[c] or (vals[c] == 0 and got == 0), (k, got)             # placed exactly
            # the second point shows the mask is read at the rounded pixel and nowhere else
            p1 = [(int(cv_round(c["u0"] + 8.0)), int(cv_round(c["v0"]))) if axis == "u" else (int(cv_round(c["u0"])), int(cv_round(c["v0"] + 8.0))) for c in cams]
            for c in range(nr):
                inside = 0 < p1[c][0] < SW and 0 < p1[c][1] < SH
                masked = masks is not None and masks[c] is not None
                assert st["in_view"][1, c] == (inside and (not masked or masks[c][p1[c][1], p1[c][0]] > 0)), (names[c], mode)
            assert any(inb) or chunk > 0
        return scene, check
    return build


for _axis in ("u", "v"):
    for _chunk in range((len(ROUND_VALUES) + ROUND_CHUNK - 1) // ROUND_CHUNK):
        for _mode in ("bounds", "live", "dead", "mixed"):
            case("rounding.%s%d_%s" % (_axis, _chunk, _mode), host="mirror mask" if _mode == "mixed" else None)(rounding_case(_axis, _chunk, _mode))


# ---------------------------------------------------------------------------------------------- geometry
def lafida_scene(dim=32, nfeatures=250):
    synth = importlib.import_module("multicol-slam_amd.synth")
    F = M.oracle_frames(dim, 3, nfeatures)[1]
    return F, M.make_rig(F["cams"], 1, True, synth), synth


def on_rays(F, rig, per_cam, depth=3.0, octave_max=1):
    """map points on the bearing rays of features of frame F (in view of that feature's camera at least), with their descriptors"""
    idx = []
    for c in range(F["nr"]):
        idx += np.flatnonzero((F["cam"] == c) & (F["keys"]["octave"] <= octave_max))[:per_cam].tolist()
    idx = np.array(idx)
    pos = np.array([(rig["MtMc"][int(F["cam"][j])] @ np.append(F["rays"][j] * depth, 1.0))[:3] for j in idx])
    return idx, pos


HOSTILE_POS = [(k, v) for k in range(3) for v in (INF, -INF, NAN)]


@case("geometry.lafida_positions", exact=False)
def _geometry_positions():
    F, rig, synth = lafida_scene()
    idx, pos = on_rays(F, rig, 4)
    n0 = len(idx)
    extra = []
    for k, v in HOSTILE_POS:                               # +-inf / NaN in each component of a point that is otherwise in view
        p = pos[0].copy()
        p[k] = v
        extra.append(p)
    axis = [(rig["MtMc"][c] @ np.array([0.0, 0.0, 2.0, 1.0]))[:3] for c in range(3)]       # on each camera's optical axis (up to the rounding of the product)
    centre = [rig["MtMc"][c][:3, 3].copy() for c in range(3)]                                # at each camera's centre: PO = 0 exactly, dist = 0
    # (no point is behind all three of these cameras: they sit behind the rig's origin along their own axes; geometry.exact_positions has one)
    allpos = np.concatenate([pos, extra, axis, centre])
    n = len(allpos)
    minD, maxD = np.full(n, 2.9), np.full(n, 10.0)             # dist = 3 on a unit ray: ratio 1.03, level 1, whose window takes octaves 0 and 1
    minD[n0 + 9:n0 + 12], minD[n0 + 12:n0 + 15] = 1.0, -1.0            # the centre points need minDistance <= 0 to stay in range
    pts = points(allpos, minD, maxD)
    desc, mask = descriptors(n, 32, 4)
    desc[:n0], mask[:n0] = F["desc"][idx], F["mask"][idx]
    scene = (pts, rig, garbage_state(n, 3), desc, mask, F, np.zeros(F["n"], np.uint8))

    def check(out):
        st, fr = out["state"], out["fresh"]
        assert all(fr[k, int(F["cam"][idx[k]])] for k in range(n0)) and out["nmatches"] >= n0 // 2
        assert not fr[n0:n0 + 9].any()                                                     # a non-finite component: NaN projection in every camera
        for c in range(3):
            assert M.dist_to_cam(allpos[n0 + 12 + c], rig["MtMc"][c]) == 0.0
            if fr[n0 + 12 + c, c]:
                assert np.isnan(st["view_cos"][n0 + 12 + c, c]) and st["level"][n0 + 12 + c, c] == 0
        assert sum(fr[n0 + 12 + c, c] for c in range(3)) + fr[n0 + 9:n0 + 12].sum() >= 1
    return scene, check


def exact_geometry(nr=3):
    rig = big_rig(nr)
    pos = [[3.0, 0.0, 4.0]]                                  # in view of every camera
    pos += [[(v if k == j else 1.5) for j in range(3)] for k, v in HOSTILE_POS]
    pos += [[0.0, 0.0, 4.0], [0.25, 0.0, 4.0], [0.5, 0.0, -4.0]]        # on the optical axis of camera 0, 1, 2 (behind camera 2)
    pos += [[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.5, 0.0, 0.0]]         # at the centres
    pos += [[0.1, 0.2, -3.0]]                                # behind every camera (the cameras look along +z)
    return rig, pos


@case("geometry.exact_positions")
def _geometry_exact():
    rig, pos = exact_geometry()
    n = len(pos)
    minD = np.full(n, 2.0)
    minD[13:16] = [-1.0, 0.0, -0.0]
    pts = points(pos, minD, 10.0)
    scene = scene_with_features(pts, rig, std_scales(), garbage_state(n, 3), seed=5)

    def check(out):
        st, fr = out["state"], out["fresh"]
        assert fr[0].all() and not fr[1:10].any()
        for c in range(3):                                   # on the axis: norm == 0 -> 1e-14, u = u0 and v = v0 exactly
            assert fr[10 + c, c] and (st["proj_x"][10 + c, c], st["proj_y"][10 + c, c]) == (320.0, 240.0)
            assert st["view_cos"][10 + c, c] == (1.0 if c < 2 else -1.0)
        # at the centres: dist == 0, the projection is (u0, v0), the cosine 0 / 0; ratios 0 / -1 = -0.0, 0 / 0 and 0 / -0.0 = NaN: level 0
        for c in range(3):
            assert fr[13 + c, c] and st["level"][13 + c, c] == 0 and np.isnan(st["view_cos"][13 + c, c]) and st["proj_x"][13 + c, c] == 320.0
        assert fr[16].all()                                  # behind every camera and in view all the same (the bool of WorldToCamHom_fast is ignored)
    return scene, check


@case("geometry.normals")
def _geometry_normals():
    rig = big_rig(2)
    normals = [[0.0, 0.0, 1.0], [NAN, 0.0, 1.0], [0.0, INF, 0.0], [0.0, 0.0, 0.0], [-INF, INF, NAN], [0.0, 0.0, -1.0], [1e308, 1e308, 1e308]]
    pts = points([[3.0, 0.0, 4.0]] * len(normals), 4.0, 10.0, normal=normals)
    scene = scene_with_features(pts, rig, std_scales(), garbage_state(len(normals), 2), seed=6)

    def check(out):
        vc = out["state"]["view_cos"][:, 0]
        assert out["fresh"].all() and vc[0] == 0.8 and np.isnan(vc[[1, 2, 4]]).all() and vc[3] == 0.0 and vc[5] == -0.8 and vc[6] == INF
    return scene, check


def one_nan_matrix(which):
    def build():
        rig, pos = exact_geometry(4)
        clean = M.frustum(points(pos, 2.0, 10.0), rig, std_scales(), garbage_state(len(pos), 4))
        rig = dict(rig, MtMc=[m.copy() for m in rig["MtMc"]], MtMc_inv=[m.copy() for m in rig["MtMc_inv"]])
        rig[which][2][0, 3] = NAN                            # camera 2 alone
        pts = points(pos, 2.0, 10.0)
        scene = scene_with_features(pts, rig, std_scales(), garbage_state(len(pos), 4), seed=7)

        def check(out):
            st = out["state"]
            for c in (0, 1, 3):                              # the other cameras of the same points: as on the clean rig
                for k in st:
                    assert P_same(st[k][:, c], clean[0][k][:, c]), (k, c)
            if which == "MtMc":                              # a NaN distance passes both comparisons: level 0, NaN cosine, the projection is the clean one
                assert out["fresh"][0, 2] and st["level"][0, 2] == 0 and np.isnan(st["view_cos"][0, 2]) and st["proj_x"][0, 2] == clean[0]["proj_x"][0, 2]
            else:                                            # a NaN projection: out of the mask
                assert not out["fresh"][:, 2].any() and clean[3][0, 2]
        return scene, check
    return build


def P_same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


case("geometry.nan_in_one_MtMc")(one_nan_matrix("MtMc"))
case("geometry.nan_in_one_MtMc_inv")(one_nan_matrix("MtMc_inv"))


@case("geometry.overlapping_cameras")
def _geometry_overlap():
    # 8 cameras that all see every point; points in pairs at the same position, so that in every camera two slots want the same features in slot order
    rig = big_rig(8)
    rng = np.random.default_rng(8)
    base = np.concatenate([rng.uniform(-2, 2, (20, 2)), rng.uniform(3, 5, (20, 1))], axis=1)
    pos = np.repeat(base, 2, axis=0)
    pts = points(pos, 2.5, 10.0)
    pts, rig, st, desc, mask, F, asg = scene_with_features(pts, rig, std_scales(), garbage_state(40, 8), seed=8, per_slot=2)
    desc[1::2], mask[1::2] = desc[0::2], mask[0::2]          # the pair shares its descriptor as well
    scene = (pts, rig, st, desc, mask, F, asg)

    def check(out):
        assert (out["fresh"].sum(axis=1) == 8).all() and out["n_to_match"] == 320
        first, second = out["match"][0::2], out["match"][1::2]
        assert (first >= 0).mean() > 0.8 and ((first >= 0) & (second >= 0) & (first != second)).sum() >= 20      # the second of a pair got another feature
    return scene, check


# ---------------------------------------------------------------------------------------------- flags
@case("flags.every_byte")
def _flags():
    rig = big_rig(2)
    flags = [0] + [b for b in FLAG_BYTES for _ in range(2)]      # point 0 opens the gate; then every byte without and with stale in-view slots
    n = len(flags)
    rng = np.random.default_rng(9)
    pos = np.concatenate([rng.uniform(-2, 2, (n, 2)), rng.uniform(3, 5, (n, 1))], axis=1)
    st = garbage_state(n, 2)
    for i in range(1, n):
        if i % 2 == 0:                                           # stale slots: in view at a place of their own, level 2
            st["in_view"][i], st["level"][i], st["view_cos"][i] = 1, 2, 0.5
            st["proj_x"][i], st["proj_y"][i] = 40.0 + 30.0 * (i // 2), [60.0, 400.0]
    scene = scene_with_features(points(pos, 2.5, 10.0, flags=flags), rig, std_scales(), st, seed=9)

    def check(out):
        fr, mt = out["fresh"], out["match"]
        for i, b in enumerate(flags):
            projected, bad, stale = (b & 3) == 0, bool(b & 1), i >= 1 and i % 2 == 0
            assert fr[i].all() == projected and fr[i].any() == projected, (i, b)
            assert (mt[i] >= 0).all() == ((projected or stale) and not bad), (i, b, mt[i])
            if not projected:
                assert out["state"]["in_view"][i].tolist() == [int(stale)] * 2
        assert fr[[i for i, b in enumerate(flags) if b in (4, 0x80)]].all()      # what `flags == 0` would have skipped
    return scene, check


# ---------------------------------------------------------------------------------------------- stale state
def stale_scene(rows, fresh_points=1, nlevels=8, seed=10, flags=None, feature_at=None):
    """LP_SEEN points whose slot 0 is rows[k] = dict(in_view, level, x, y, cos); `fresh_points` plain points come first and open the gate.  The stale
    slots sit 60 px apart; feature_at[k] = (dx, dy): the point's feature lies there relative to the stale projection (default: on it)"""
    rig = big_rig(1)
    n = fresh_points + len(rows)
    pos = [[0.3 * i, 0.2, 4.0] for i in range(n)]
    fl = [0] * fresh_points + ([M.LP_SEEN] * len(rows) if flags is None else list(flags))
    st = garbage_state(n, 1)
    sc = std_scales(nlevels)
    pts = points(pos, 3.0, 10.0, flags=fl)
    for k, r in enumerate(rows):
        i = fresh_points + k
        st["in_view"][i, 0], st["level"][i, 0], st["view_cos"][i, 0] = r.get("in_view", 1), r.get("level", 1), r.get("cos", 0.5)
        st["proj_x"][i, 0], st["proj_y"][i, 0] = r.get("x", 40.0 + 60.0 * (k % 10)), r.get("y", 60.0 + 90.0 * (k // 10))
    pts, rig, st, desc, mask, F, asg = scene_with_features(pts, rig, sc, st, seed=seed, stale_targets=False)
    # the stale slots' features, placed by hand (the builder above placed the fresh ones)
    targets = []
    for k, r in enumerate(rows):
        i = fresh_points + k
        dx, dy = (0.0, 0.0) if feature_at is None else feature_at[k]
        targets.append((0, 40.0 + 60.0 * (k % 10) + dx, 60.0 + 90.0 * (k // 10) + dy, 1, desc[i], mask[i]))
    fresh_t = [(0, float(F["keys"]["x"][j]), float(F["keys"]["y"][j]), int(F["keys"]["octave"][j]), F["desc"][j], F["mask"][j]) for j in range(F["n"])]
    F = make_frame(rig["cams"], sc, fresh_t + targets, 32, seed, extra=0)
    return (pts, rig, st, desc, mask, F, np.zeros(F["n"], np.uint8)), fresh_points


@case("stale.in_view_truth_values")
def _stale_in_view():
    rows = [dict(in_view=v) for v in (1, 2, 0x80, 0xFF, 0)]
    scene, f = stale_scene(rows)

    def check(out):
        assert out["state"]["in_view"][f:, 0].tolist() == [1, 2, 0x80, 0xFF, 0]           # untouched
        assert (out["match"][f:f + 4, 0] >= 0).all() and out["match"][f + 4, 0] == -1     # any non-zero byte is "in view"
    return scene, check


def stale_levels(name, flags, host):
    @case(name, host=host)
    def _build():
        rows = [dict(level=v) for v in (1, -1, INT_MIN, 8, INT_MAX, 7, 0)]
        scene, f = stale_scene(rows, flags=[flags] * 7)

        def check(out):
            assert out["state"]["level"][f:, 0].tolist() == [1, -1, INT_MIN, 8, INT_MAX, 7, 0]
            assert out["match"][f, 0] >= 0 and (out["match"][f + 1:f + 5, 0] == -1).all() and searched(scene, out)[f:, 0].tolist() == [1, 0, 0, 0, 0, 1, 1]
        return scene, check


stale_levels("stale.levels_outside_the_pyramid", M.LP_SEEN, "level")
stale_levels("stale.levels_outside_with_a_high_flag_bit", M.LP_SEEN | 4, "level")      # bits beyond 0 and 1 do not hide the slot from the host's check


@case("stale.nonfinite_projections")
def _stale_proj():
    rows = [dict()] + [dict(x=v) for v in (NAN, INF, -INF, 1e300, -1e300)] + [dict(y=v) for v in (NAN, INF, -INF, 1e300)] + [dict(x=NAN, y=NAN), dict()]
    scene, f = stale_scene(rows)

    def check(out):
        m = out["match"][f:, 0]
        assert m[0] >= 0 and m[-1] >= 0 and (m[1:-1] == -1).all() and searched(scene, out)[f:, 0].all()      # searched, and the window is empty
    return scene, check


@case("stale.view_cos_radius")
def _stale_cos():
    # RadiusByViewingCos: viewCos > 0.998 ? 2.5 : 4.0, times th = 3 and the level-1 factor 1.2: 9 px or 14.4 px.  The feature lies 11 px off.
    coss = [NAN, 0.998, math.nextafter(0.998, 1.0), INF, -INF, 1.0, 0.5]
    rows = [dict(cos=v) for v in coss]
    scene, f = stale_scene(rows, feature_at=[(11.0, 0.0)] * len(rows))

    def check(out):
        assert (out["match"][f:, 0] >= 0).tolist() == [True, True, False, False, True, False, True]
    return scene, check


@case("stale.gate_nothing_fresh")
def _stale_gate0():
    scene, f = stale_scene([dict(), dict(), dict()], fresh_points=1)
    scene[0]["min_dist"][0] = 50.0                          # the one unskipped point is too near: nToMatch == 0

    def check(out):
        assert out["n_to_match"] == 0 and out["nmatches"] == 0 and (out["match"] == -1).all() and out["state"]["in_view"][:, 0].tolist() == [0, 1, 1, 1]
    return scene, check


@case("stale.gate_one_fresh")
def _stale_gate1():
    scene, f = stale_scene([dict(), dict(), dict()], fresh_points=2)
    scene[0]["min_dist"][1] = 50.0

    def check(out):
        assert out["n_to_match"] == 1 and out["nmatches"] == 4 and (out["match"][:, 0] >= 0).tolist() == [True, False, True, True, True]
    return scene, check


# ---------------------------------------------------------------------------------------------- slot counts
def slot_case(npoints, nr, mode):
    """mode: "all", "none", or the slot that alone is in view.  Camera c sits c / 4 along x, every point at (0, 0, 4): its distance to camera c is
    sqrt(c^2 / 16 + 16), another double for every c, so min_dist == max_dist == that distance lets camera c alone through"""
    def build():
        rig = big_rig(nr)
        dists = [M.dist_to_cam([0.0, 0.0, 4.0], rig["MtMc"][c]) for c in range(nr)]
        assert len(set(dists)) == nr
        minD, maxD = np.full(npoints, 3.5), np.full(npoints, 100.0)
        if mode != "all":
            minD[:], maxD[:] = 9.0, 8.0                      # max < min: never in view
        if isinstance(mode, int):
            i, c = divmod(mode, nr)
            minD[i] = maxD[i] = dists[c]
        pts = points([[0.0, 0.0, 4.0]] * npoints, minD, maxD)
        scene = scene_with_features(pts, rig, std_scales(), garbage_state(npoints, nr), seed=11, per_slot=1 if mode == "all" else 3, near=2.0)

        def check(out):
            fr = out["fresh"].reshape(-1)
            want = np.zeros(npoints * nr, np.uint8)
            if mode == "all":
                want[:] = 1
            elif isinstance(mode, int):
                want[mode] = 1
            assert np.array_equal(fr, want) and out["n_to_match"] == int(want.sum())
            assert (out["nmatches"] > 0) == (mode != "none")
        return scene, check
    return build


def slot_modes(nslots):
    modes = {"all": "all", "none": "none", "first": 0, "last": nslots - 1}
    if nslots > 63:
        modes["lane63"] = 63
    if nslots > 256:
        modes["block2"] = 256
    return modes


for _np, _nr in SLOT_SHAPES:
    for _k, _m in slot_modes(_np * _nr).items():
        if _np * _nr == 1 and _k == "last":
            continue
        case("slots.%dx%d_%s" % (_np, _nr, _k))(slot_case(_np, _nr, _m))


# ---------------------------------------------------------------------------------------------- contention
def contention_case(dim, npoints, interleave, per_cam=24):
    """every point at one position with one descriptor, three cameras: in each camera npoints slots want the same per_cam features (8 * k bits away from the
    descriptor, alternating between the predicted level and the one below it).  interleave: every other point is idle (bad, seen without stale slots, or out
    of range in turn), so active and idle slots alternate through every greedy round"""
    def build():
        rig = big_rig(3)
        flags, minD = np.zeros(npoints, np.uint8), np.full(npoints, 3.5)
        if interleave:
            for i in range(1, npoints, 2):
                kind = (i // 2) % 3
                if kind == 0:
                    flags[i] = M.LP_BAD
                elif kind == 1:
                    flags[i] = M.LP_SEEN
                else:
                    minD[i] = 50.0
        pts = points([[3.0, 0.0, 4.0]] * npoints, minD, 100.0, flags=flags)
        st = M.new_state(npoints, 3)
        one = scene_with_features(points([[3.0, 0.0, 4.0]], 3.5, 100.0), rig, std_scales(), M.new_state(1, 3), dim=dim, seed=12, per_slot=per_cam, near=3.0, extra=4,
                                  assigned_share=0.1)
        desc, mask = np.repeat(one[3], npoints, axis=0), np.repeat(one[4], npoints, axis=0)
        scene = (pts, rig, st, desc, mask, one[5], one[6])

        def check(out):
            active = searched(scene, out)
            assert np.array_equal(active, out["fresh"].astype(bool))
            per = active.sum(axis=0)
            assert (per > per_cam + 4).all(), per                       # more active slots than features in the whole camera, let alone the window
            assert 6 <= out["nmatches"] < int(active.sum())
            if interleave:
                assert active[0::2].all() and not active[1::2].any()
        return scene, check
    return build


case("contention.one_position")(contention_case(32, 100, False))
case("contention.idle_interleaved")(contention_case(32, 200, True))
for _dim in (16, 32, 64):
    case("contention.dim%d" % _dim)(contention_case(_dim, 40, False))
NOMASK_CASES = ["contention.dim16", "contention.dim32", "contention.dim64", "contention.one_position"]      # also run without descriptor masks

# the three sizes the back-to-back test enqueues without a wait in between
BACK_TO_BACK = ("contention.idle_interleaved", "slots.1x1_all", "slots.171x3_all")
