"""No GPU: the hostile cases of tests/hostile_frustum.py.

* A second, literal scalar statement of cMultiFrame::isInFrustum (src/cMultiFrame.cpp:218-270) under the loop of
  cTracking::SearchReferencePointsInFrustum (src/cTracking.cpp:978-999), in Python floats and `math` alone, cvRound by the x86 rule
  (hostile_windows.cv_round) and std::lower_bound as bisect.bisect_left (the same comparisons at the same midpoints).  The model (frustum_model.frustum, which
  projects through the oracle's compiled code) must give the same bits on every case.
* Hand-derived answers on the exact rig; every case's non-vacuity predicate; the size limits of the table.
* The host branch of csrc/mcs_geom.h (tests/cpp/frustum_geom_driver.cpp, compiled as tests/test_geom_cpu.py compiles its driver) on the rounding and
  geometry cases: in_mirror_mask by the x86 rule, by a conversion that saturates as the device's does, and by (int)lrint, each against the statement here."""
import bisect
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import frustum_model as M
import hostile_frustum as H
import oracle_lib as O
from hostile_windows import cv_round

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
NAMES = list(H.CASES)


# ---------------------------------------------------------------------------------------------- the independent statement
def div(a, b):
    if b == 0.0:                                                   # Python raises where IEEE gives +-inf or NaN
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def world_to_img(cam, x, y, z):
    """cCamModelGeneral_::WorldToImg, src/cam_model_omni.cpp:146-161; horner, include/misc.h:115-122"""
    norm = math.sqrt(x * x + y * y)
    if norm == 0.0:
        norm = 1e-14
    theta = math.atan(div(-z, norm))
    rho = 0.0
    for i in range(len(cam["invP"]) - 1, -1, -1):
        rho = rho * theta + cam["invP"][i]
    uu = div(x, norm) * rho
    vv = div(y, norm) * rho
    return uu * cam["c"] + vv * cam["d"] + cam["u0"], uu * cam["e"] + vv + cam["v0"]


def in_mirror_mask(cam, mask, u, v):
    """isPointInMirrorMask(u, v, 0), :163-178; mask None: the library's bounds-only form"""
    ur, vr = int(cv_round(u)), int(cv_round(v))
    if ur >= cam["width"] or ur <= 0 or vr >= cam["height"] or vr <= 0:
        return False
    return mask is None or mask[vr][ur] > 0


def is_in_frustum(P, Pn, minD, maxD, Minv, Tcw, cam, mask, scales):
    """src/cMultiFrame.cpp:218-270 -> None (false) or (u, v, level, viewCos)"""
    pt = [float(P[0]), float(P[1]), float(P[2]), 1.0]
    rot = []
    for r in range(3):                                             # MtMc_inv[c] * pt (cam_system_omni.cpp:124): s = 0; s += m * p
        s = 0.0
        for k in range(4):
            s += float(Minv[r][k]) * pt[k]
        rot.append(s)
    u, v = world_to_img(cam, rot[0], rot[1], rot[2])
    if not in_mirror_mask(cam, mask, u, v):
        return None
    PO = [pt[k] - float(Tcw[k][3]) for k in range(3)]
    dist = math.sqrt(((0.0 + PO[0] * PO[0]) + PO[1] * PO[1]) + PO[2] * PO[2])
    if dist < minD or dist > maxD:
        return None
    viewCos = div(((0.0 + PO[0] * float(Pn[0])) + PO[1] * float(Pn[1])) + PO[2] * float(Pn[2]), dist)
    ratio = div(dist, minD)
    level = bisect.bisect_left(scales, ratio)
    if level >= len(scales):
        level = len(scales) - 1
    return u, v, level, viewCos


def statement(scene):
    """the loop :981-999 -> (state, visible_inc, nToMatch, fresh)"""
    pts, rig, st0, desc, mask, F, asg = scene
    n, nr = len(pts["pos"]), len(rig["cams"])
    st = M.copy_state(st0)
    scales = [float(s) for s in F["scales"]]
    vis, fresh, ntm = np.zeros(n, np.int32), np.zeros((n, nr), np.uint8), 0
    for i in range(n):
        if int(pts["flags"][i]) & 2 or int(pts["flags"][i]) & 1:  # :985-988, the two bits that have a meaning
            continue
        for c in range(nr):
            st["in_view"][i, c] = 0
            r = is_in_frustum(pts["pos"][i], pts["normal"][i], float(pts["min_dist"][i]), float(pts["max_dist"][i]), rig["MtMc_inv"][c], rig["MtMc"][c],
                              rig["cams"][c], None if rig["masks"] is None else rig["masks"][c], scales)
            if r is None:
                continue
            st["in_view"][i, c] = 1
            st["proj_x"][i, c], st["proj_y"][i, c], st["level"][i, c], st["view_cos"][i, c] = r
            fresh[i, c] = 1
            vis[i] += 1
            ntm += 1
    return st, vis, ntm, fresh


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na = np.isnan(a)
    return np.array_equal(na, np.isnan(b)) and np.array_equal(a[~na].view(np.uint64), b[~na].view(np.uint64))


# ---------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("name", NAMES)
def test_model_equals_the_independent_statement_and_the_case_does_its_job(name):
    case, out = H.get(name), H.model(name)
    case["check"](out)                                             # the non-vacuity predicate
    st, vis, ntm, fresh = statement(case["scene"])
    for k in st:
        assert same(st[k], out["state"][k]), k
    assert np.array_equal(vis, out["visible_inc"]) and ntm == out["n_to_match"] and np.array_equal(fresh, out["fresh"])
    assert out["n_to_match"] == int(out["fresh"].sum()) and np.array_equal(out["visible_inc"], out["fresh"].sum(axis=1))
    # what the search may touch: only searched slots hold a match, a feature is given once, and `assigned` grows by exactly the matches
    m, sr = out["match"], H.searched(case["scene"], out)
    assert (m[~sr] == -1).all() and len(set(m[m >= 0].tolist())) == int((m >= 0).sum()) == out["nmatches"]
    before = np.ascontiguousarray(case["scene"][6], np.uint8)
    assert not before[m[m >= 0]].any() and int(out["assigned"].sum()) == int(before.sum()) + out["nmatches"]


def test_the_table_holds_every_group_within_its_limits():
    g = H.groups()
    assert set(g) == {"bounds", "levels", "rounding", "geometry", "flags", "stale", "slots", "contention"}
    for name in NAMES:
        pts, rig, st, desc, mask, F, asg = H.get(name)["scene"]
        n, nr = len(pts["pos"]), len(rig["cams"])
        assert 1 <= n <= 600 and (nr <= 8 or (n, nr) == (2, 32)), name
        assert np.bincount(F["cam"], minlength=nr).max() <= 300 and F["nr"] == nr and desc.shape[1] in (16, 32, 64), name
    slots = sorted({a * b for a, b in H.SLOT_SHAPES})
    assert slots == [1, 63, 64, 65, 255, 256, 257, 513] and {b for a, b in H.SLOT_SHAPES} == {1, 2, 3, 5, 8, 32}
    assert {len(H.get("levels.nlevels_" + k)["scales"]) for k in ("1", "2", "8", "max")} == {1, 2, 8, H.MAX_LEVELS}
    assert all(H.get(n)["exact"] for n in NAMES if n != "geometry.lafida_positions")


def test_flag_bytes_only_bits_0_and_1_count():
    """hand-derived: of {0, 1, 2, 3, 4, 6, 0x80, 0xFE, 0xFF} the bytes 0, 4 and 0x80 are projected; 0, 2, 4, 6, 0x80 and 0xFE may be searched"""
    assert [b for b in H.FLAG_BYTES if not b & 3] == [0, 4, 0x80] and [b for b in H.FLAG_BYTES if not b & 1] == [0, 2, 4, 6, 0x80, 0xFE]
    case, out = H.get("flags.every_byte"), H.model("flags.every_byte")
    fl = case["scene"][0]["flags"]
    assert np.array_equal(out["fresh"].all(axis=1), (fl & 3) == 0)
    # a rule of `flags == 0` (the kernel before this suite) would leave these points unprojected: the case tells the two rules apart
    assert out["fresh"][(fl != 0) & ((fl & 3) == 0)].all() and ((fl != 0) & ((fl & 3) == 0)).sum() == 4


def test_hand_derived_answers_on_the_exact_rig():
    cam = H.exact_cam(320.0, 240.0, 100.0, H.BW, H.BH)
    eye = np.eye(4)
    sc = [float(s) for s in H.std_scales()]
    # (3, 0, 4): norm 3, u = 1 * 100 + 320, v = 240, dist 5, cos 4 / 5; ratio 5 / 4 = 1.25 lies between 1.2 and 1.44: level 2
    assert is_in_frustum([3.0, 0.0, 4.0], [0.0, 0.0, 1.0], 4.0, 9.0, eye, eye, cam, None, sc) == (420.0, 240.0, 2, 0.8)
    # on the axis: norm == 0 -> 1e-14, uu = 0 / 1e-14 * rho = 0: (u0, v0) exactly, behind the camera as well
    assert is_in_frustum([0.0, 0.0, 4.0], [0.0, 0.0, 1.0], 4.0, 9.0, eye, eye, cam, None, sc) == (320.0, 240.0, 0, 1.0)
    assert is_in_frustum([0.0, 0.0, -4.0], [0.0, 0.0, 1.0], 4.0, 9.0, eye, eye, cam, None, sc) == (320.0, 240.0, 0, -1.0)
    # at the centre: dist 0 inside [-1, 9]; 0 / 0 cosine, ratio -0.0
    r = is_in_frustum([0.0, 0.0, 0.0], [0.0, 0.0, 1.0], -1.0, 9.0, eye, eye, cam, None, sc)
    assert r[:3] == (320.0, 240.0, 0) and math.isnan(r[3])
    # round-half-even at the open bounds of a 64 x 48 image, placed through u0 on the axis
    for u0, inside in ((0.5, False), (1.5, True), (2.5, True), (62.5, True), (63.5, False), (63.51, False), (-0.0, False), (1e-300, False), (2.0 ** 31 - 0.5, False),
                       (2.0 ** 31, False), (-2.0 ** 31 - 1, False), (1e300, False), (-1e300, False), (math.inf, False), (-math.inf, False), (math.nan, False),
                       (2.0 ** 32 + 5, False), (2.0 ** 63, False)):
        small = H.exact_cam(u0, 24.0, 8.0, H.SW, H.SH)
        assert (is_in_frustum([0.0, 0.0, 4.0], [0.0, 0.0, 1.0], 3.5, 9.0, eye, eye, small, None, sc) is not None) == inside, u0
        small = H.exact_cam(32.0, u0 if u0 not in (62.5, 63.5, 63.51) else u0 - 16.0, 8.0, H.SW, H.SH)
        assert (is_in_frustum([0.0, 0.0, 4.0], [0.0, 0.0, 1.0], 3.5, 9.0, eye, eye, small, None, sc) is not None) == inside, u0
    assert [int(cv_round(v)) for v in (0.5, 1.5, 2.5, 62.5, 63.5)] == [0, 2, 2, 62, 64]


def test_bisection_on_tables_that_are_not_ascending():
    for table in (H.EQUAL_TABLE, H.DESCENDING_TABLE, H.NAN_TABLE, H.INF_TABLE, H.UNSORTED_TABLE, [1.0]):
        for v in (0.0, -0.0, 0.5, 1.0, 1.25, 1.5, 1.75, 2.0, 2.25, 3.0, 3.5, 4.0, 5.0, math.inf, -math.inf, math.nan):
            assert M.lower_bound(table, v) == bisect.bisect_left(table, v), (table, v)
    assert M.lower_bound(H.DESCENDING_TABLE, 2.25) == 8 and H.naive_level(H.DESCENDING_TABLE, 2.25) == 4       # the bisection sees 2.0 < 2.25 and goes right
    assert M.lower_bound(H.NAN_TABLE, 3.2) == 7 and M.lower_bound(H.NAN_TABLE, 1.6) == 3                       # `NaN < v` is false: the left half


# ---------------------------------------------------------------------------------------------- the host branch of csrc/mcs_geom.h
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the library's floating-point flags (csrc/Makefile), host only"""
    exe = tmp_path_factory.mktemp("frustum_geom") / "frustum_geom_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-I" + CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "frustum_geom_driver.cpp"), "-o", str(exe)])
    return exe


def run_driver(driver, tmp_path, rig, pos):
    nr, n = len(rig["cams"]), len(pos)
    oc = (O.Ocam * nr)(*[O.make_ocam(c) for c in rig["cams"]])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nr, n, C.sizeof(O.Ocam)], np.int32).tobytes() + bytes(oc))
        f.write(np.ascontiguousarray(np.stack(rig["MtMc_inv"]), np.float64).tobytes())
        for c in range(nr):
            m = None if rig["masks"] is None else rig["masks"][c]
            f.write(np.array([0 if m is None else 1], np.int32).tobytes() + (b"" if m is None else np.ascontiguousarray(m, np.uint8).tobytes()))
        f.write(np.ascontiguousarray(pos, np.float64).tobytes())
    subprocess.check_call([str(driver), str(src), str(dst)])
    raw = open(dst, "rb").read()
    assert len(raw) == n * nr * 19
    return np.frombuffer(raw[:n * nr * 16], np.float64).reshape(n, nr, 2), np.frombuffer(raw[n * nr * 16:], np.uint8).reshape(n, nr, 3)


GEOM_CASES = [n for n in NAMES if n.startswith("rounding.") or n.startswith("geometry.")]


@pytest.mark.parametrize("name", GEOM_CASES)
def test_host_branch_of_the_geometry_header_rounds_by_the_x86_rule(driver, tmp_path, name):
    pts, rig = H.get(name)["scene"][:2]
    uv, fl = run_driver(driver, tmp_path, rig, pts["pos"])
    n, nr = fl.shape[:2]
    differs = 0
    for i in range(n):
        for c in range(nr):
            p = pts["pos"][i]
            u, v = world_to_img(rig["cams"][c], *[sum_row(rig["MtMc_inv"][c][r], p) for r in range(3)])
            assert same(np.array([u, v]), uv[i, c]), (i, c)         # the host's atan on both sides
            want = in_mirror_mask(rig["cams"][c], None if rig["masks"] is None else rig["masks"][c], u, v)
            assert fl[i, c, 0] == want and fl[i, c, 1] == want, (i, c, u, v, fl[i, c])      # the x86 rule and the saturating conversion: one answer
            differs += int(fl[i, c, 2] != want)
    # (int)lrint keeps the low 32 bits of a long: 2^32 + 5 becomes pixel 5.  Only the chunk that holds that value shows it.
    assert (differs > 0) == (name.split(".")[1][:2] in ("u2", "v2") and not name.endswith("live")), (name, differs)


def sum_row(row, p):
    s = 0.0
    for k, x in enumerate((float(p[0]), float(p[1]), float(p[2]), 1.0)):
        s += float(row[k]) * x
    return s


def test_every_double_class_is_rejected_alike_by_both_conversions():
    """the open bounds test makes the two conversions indistinguishable: NaN -> 0 or INT_MIN, beyond int -> INT_MAX / INT_MIN or INT_MIN, all outside
    0 < r < W for every W <= INT_MAX; inside int they are the same rint"""
    def saturating(v):
        if v != v:
            return 0
        r = float(np.rint(v))
        return H.INT_MAX if r >= 2.0 ** 31 else H.INT_MIN if r < -2.0 ** 31 else int(r)
    for v in [H.round_value(k, H.SW) for k in H.ROUND_VALUES] + [2.0 ** 31 - 1, 2.0 ** 31 - 1.5, -2.0 ** 31, -2.0 ** 31 - 0.5, 5.0, 5.5, 6.5]:
        a, b = saturating(v), int(cv_round(v))
        for W in (2, 64, H.INT_MAX):
            assert (0 < a < W) == (0 < b < W), (v, W)
        assert a == b or (not 0 < a < H.INT_MAX and not 0 < b < H.INT_MAX), v
