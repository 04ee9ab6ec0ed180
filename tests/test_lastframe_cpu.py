"""No GPU: the frame-to-frame searches of the tracker — cORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th) (src/cORBmatcher.cpp:1990-2118) and
WindowSearch (:326-473).  The conditions the GPU tests put on their scenes (tests/lastframe_scene.py), the reference's quirks on hand-made cases through the
oracle alone (each case fails with the quirk "fixed"), and the library's surface: exports, ABI number, loud refusal of bad arguments, struct layouts, the facade."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import lastframe_scene as LS
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_search_last_frame", "mcs_window_search_frames"]
W, H = np.array([754], np.int32), np.array([480], np.int32)
SC = LS.scales()
INT_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("multicol-slam_amd")
    if not os.path.exists(p._capi.LIB_PATH):
        importlib.import_module("__graft_entry__").build()
    return p


def frame(feats, dim=32, mask=None):
    """one camera; feats: (x, y, octave, angle, descriptor row or the number of leading one-bits)"""
    n = len(feats)
    k = np.zeros(n, O.KP_DTYPE)
    d = np.zeros((n, dim), np.uint8)
    for i, (x, y, o, a, bits) in enumerate(feats):
        k["x"][i], k["y"][i], k["octave"][i], k["angle"][i] = x, y, o, a
        d[i] = np.packbits(np.arange(dim * 8) < bits, bitorder="little") if np.isscalar(bits) else bits
    m = None if mask is None else np.full((n, dim), mask, np.uint8)
    return O.frame_view(k, d, m, np.zeros(n, np.int32), W, H), k


def search_last(cur, last, uv=None, lastMP=None, outlier=None, in_mask=None, assigned=None, th=15.0, dim=32, masks=False, ori=0):
    (fc, kc), ck = cur
    (fl, kl), lk = last
    n = len(lk)
    uv = np.stack([lk["x"], lk["y"]], axis=1).astype(np.float64) if uv is None else np.asarray(uv, np.float64)
    return O.search_by_projection_last(fc, np.zeros(len(ck), np.uint8) if assigned is None else assigned, fl, np.ones(n, np.uint8) if lastMP is None else lastMP,
                                       np.zeros(n, np.uint8) if outlier is None else outlier, uv, np.ones(n, np.uint8) if in_mask is None else in_mask, SC, th, dim,
                                       masks, ori)


# ---------------------------------------------------------------------------------------------- the scenes of the GPU tests
@pytest.mark.parametrize("name", sorted(LS.SCENES))
def test_scene_conditions_of_the_gpu_tests(name):
    c = LS.check_scene(LS.make_pair(**LS.SCENES[name]))
    assert c["matches"] >= 50 and c["dropped"] >= 1 and c["contested"] >= 1 and min(c["skipped"].values()) >= 1, c
    w = LS.check_scene(LS.make_pair(window=True, **LS.SCENES[name]))
    assert w["matches"] >= 50 and w["dropped"] >= 1, w


# ---------------------------------------------------------------------------------------------- quirks, on the oracle alone
@pytest.mark.parametrize("masks,th_high", [(False, 3 * 32), (True, int(np.floor(1.5 * 32)))])
def test_distance_exactly_th_high_is_accepted_and_one_more_is_not(masks, th_high):
    m = 0xFF if masks else None      # all-ones masks: the masked distance (popcount(x & m1) + popcount(x & m2)) >> 1 is the plain one
    last = frame([(100, 100, 2, 0.0, 0)], mask=m)
    for bits, want in ((th_high, 0), (th_high + 1, -1)):
        cur = frame([(101, 100, 2, 0.0, bits)], mask=m)
        nm, mc, asg = search_last(cur, last, masks=masks)
        assert (nm, mc.tolist(), asg.tolist()) == (int(want == 0), [want], [int(want == 0)]), (bits, nm, mc)
        nw, m21 = O.window_search(last[0][0], np.ones(1, np.uint8), cur[0][0], 20, 0, -1, 0.8, 32, masks, 0)
        assert (nw, m21.tolist()) == (int(want == 0), [want])     # bestDist2 stays INT_MAX: the ratio test passes, TH_HIGH decides (:416)


def test_octave_0_searches_levels_0_and_1_only():
    # GetFeaturesInArea(.., -1, 1): "minLevel == -1 && maxLevel == -1" alone means no level check, so octave 0 gives a CHECKED range that ends at level 1
    last = frame([(100, 100, 0, 0.0, 0)])
    nm, mc, _ = search_last(frame([(100, 100, 2, 0.0, 0), (101, 100, 1, 0.0, 5)]), last)
    assert (nm, mc.tolist()) == (1, [-1, 0])                      # the exact copy at octave 2 is not even a candidate
    nm, mc, _ = search_last(frame([(100, 100, 2, 0.0, 0)]), last)
    assert (nm, mc.tolist()) == (0, [-1])
    nm, mc, _ = search_last(frame([(100, 100, 0, 0.0, 3), (100, 100, 1, 0.0, 3)]), last)
    assert mc.tolist() == [0, -1]                                 # both levels in range, strict '<' keeps the first
    # the top octave: [6, 8] holds levels 6 and 7
    nm, mc, _ = search_last(frame([(100, 100, 5, 0.0, 0), (100, 100, 6, 0.0, 9)]), frame([(100, 100, 7, 0.0, 0)]))
    assert mc.tolist() == [-1, 0]


def test_a_point_behind_the_camera_inside_the_mask_is_searched():
    # without a mask image only the bounds test decides: (1, 0.5, -0.05) lies behind the image plane (ptRot.z <= 0) and projects to about (660, 379)
    synth = importlib.import_module("multicol-slam_amd.synth")
    cam = synth.lafida_cameras()[0]
    uv, fl = O.world_to_cam(np.eye(4)[None], [cam], None, np.array([[1.0, 0.5, -0.05]]), np.zeros(1, np.int32))
    assert fl[0] == 3, fl                                         # bit1: behind the camera, bit0: inside
    cur = frame([(float(np.float32(uv[0, 0])), float(np.float32(uv[0, 1])), 3, 0.0, 4)])
    nm, mc, _ = search_last(cur, frame([(10, 10, 3, 0.0, 0)]), uv=uv, in_mask=fl & 1)
    assert (nm, mc.tolist()) == (1, [0])                          # the bool WorldToCamHom_fast returns is ignored (:2020)


def test_a_dropped_match_frees_its_feature():
    # rot = last angle - current angle: three matches in bin 0, two in bin 1, two in bin 3, one in bin 7; ComputeThreeMaxima keeps three bins
    deltas = [0, 2, 4, 35, 36, 95, 96, 205]
    last = frame([(60 + 70 * i, 100, 2, 300.0, np.packbits(np.arange(256) % 8 == i, bitorder="little")) for i in range(8)])
    cur = frame([(60 + 70 * i, 101, 2, 300.0 - deltas[i], np.packbits(np.arange(256) % 8 == i, bitorder="little")) for i in range(8)])
    nm, mc, asg = search_last(cur, last, ori=0)
    assert (nm, mc.tolist(), asg.tolist()) == (8, list(range(8)), [1] * 8)
    nm, mc, asg = search_last(cur, last, ori=1)
    assert (nm, mc.tolist(), asg.tolist()) == (7, list(range(7)) + [-1], [1] * 7 + [0])     # CurrentFrame.mvpMapPoints[...] = NULL, --nmatches (:2110-2111)
    held = np.zeros(8, np.uint8)
    held[7] = 1
    nm, mc, asg = search_last(cur, last, assigned=held, ori=1)
    assert (nm, mc.tolist(), asg.tolist()) == (7, list(range(7)) + [-1], [1] * 8)           # a feature that held a point on entry is never in the histogram


def test_window_search_ignores_previous_matches_of_f2_and_outliers():
    S = LS.make_pair(window=True, **LS.SCENES["3x401"])
    e = LS.expected_window(S, 0)
    st = S["last"]["status"]
    m = e["match21"]
    assert ((m >= 0) & (S["assigned"] != 0)).sum() >= 5           # vpMapPointMatches2 starts from NULLs (:333)
    assert (st[m[m >= 0]] == 2).sum() >= 5                        # mvbOutlier is not read
    assert (st[m[m >= 0]] == 3).sum() >= 5                        # nothing is projected either
    assert not np.isin(st[m[m >= 0]], (0, 1)).any()               # NULL and bad points are skipped (:348-352)
    assert np.array_equal(e["points2"][m >= 0], S["last"]["points"][m[m >= 0]]) and (e["points2"][m < 0] == -1).all()


def test_min_level_0_and_max_level_int_max_filter_nothing():
    f1 = frame([(100, 100, 0, 0.0, 0), (300, 100, 7, 0.0, 0), (500, 100, 3, 0.0, 0)])
    f2 = frame([(101, 100, 0, 0.0, 1), (301, 100, 7, 0.0, 1), (501, 100, 3, 0.0, 1)])
    has = np.ones(3, np.uint8)

    def ws(lo, hi):
        return O.window_search(f1[0][0], has, f2[0][0], 20, lo, -1 if hi == INT_MAX else hi, 0.8, 32, False, 0)[1].tolist()
    assert ws(0, INT_MAX) == [0, 1, 2]                            # bMinLevel = minScaleLevel > 0, bMaxLevel = maxScaleLevel < INT_MAX (:341-342)
    assert ws(1, INT_MAX) == [-1, 1, 2] and ws(0, 6) == [0, -1, 2] and ws(3, 3) == [-1, -1, 2]
    assert ws(-5, INT_MAX) == [0, 1, 2]                           # a negative minimum is "no filter" too


# ---------------------------------------------------------------------------------------------- the library's surface
def test_library_exports_the_new_entry_points(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in pkg._capi.EXPORTS, n
    txt = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    assert L.mcs_abi_version() == int(re.search(r"#define MCS_ABI_VERSION (\d+)", txt).group(1)) == 10
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, txt), n


def test_bad_arguments_are_refused(pkg):
    cap, L = pkg._capi, pkg.lib()
    t, p, r, f = cap.TrackedFrame(), cap.PointTable(), cap.RigView(), cap.FrameView()
    one = np.zeros(1, np.int32)
    assert L.mcs_search_last_frame(None, C.byref(t), C.byref(p), C.byref(r), C.byref(f), 15.0, 32, 0, 0, cap.np_ptr(one), None, cap.np_ptr(one)) == cap.MCS_ERR_INVALID
    assert b"null" in L.mcs_last_error()
    assert L.mcs_window_search_frames(None, C.byref(t), C.byref(p), C.byref(f), 20, 0, INT_MAX, 0.8, 32, 0, 0, cap.np_ptr(one), None, cap.np_ptr(one)) == cap.MCS_ERR_INVALID
    with pytest.raises(pkg.McsError):
        pkg.check(L.mcs_search_last_frame(None, None, None, None, None, 15.0, 32, 0, 0, None, None, None))
    with pytest.raises(pkg.McsError):
        pkg.check(L.mcs_window_search_frames(None, None, None, None, 20, 0, INT_MAX, 0.8, 32, 0, 0, None, None, None))


def test_struct_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "mcs_c.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mcs_tracked_frame), '
                   'offsetof(mcs_tracked_frame, points), offsetof(mcs_tracked_frame, outlier), offsetof(mcs_tracked_frame, n), offsetof(mcs_tracked_frame, stride), '
                   'sizeof(mcs_point_table), offsetof(mcs_point_table, flags), offsetof(mcs_point_table, n)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    T, P = pkg._capi.TrackedFrame, pkg._capi.PointTable
    assert got == [C.sizeof(T), T.points.offset, T.outlier.offset, T.n.offset, T.stride.offset, C.sizeof(P), P.flags.offset, P.n.offset]


def test_facade_driver_compiles_and_links(pkg, tmp_path):
    exe = tmp_path / "facade_driver_lastframe"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_lastframe.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 2       # no arguments: the usage exit, before anything touches a device
