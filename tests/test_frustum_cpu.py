"""No GPU: the model of cMultiFrame::isInFrustum and of cTracking::SearchReferencePointsInFrustum (tests/frustum_model.py) against hand-derived answers, the
conditions the GPU tests put on their scenes, and the library's surface (exports, ABI number, loud refusal of bad arguments, struct layouts, the facade)."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess

import numpy as np
import pytest

import frustum_model as M
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_frustum", "mcs_search_local_points"]
S = [1.0, 1.2, 1.44, 1.728]   # scale factors of the hand-made cases (exact products are not needed: only comparisons)
I4 = np.eye(4)


@pytest.fixture(scope="module")
def pkg():
    p = importlib.import_module("multicol-slam_amd")
    if not os.path.exists(p._capi.LIB_PATH):
        importlib.import_module("__graft_entry__").build()
    return p


def frustum1(P, minD, maxD, Pn=(0.0, 0.0, 1.0), T=I4, uv=(10.0, 20.0), in_mask=True, scales=S):
    return M.is_in_frustum(P, Pn, minD, maxD, T, uv, in_mask, scales)


# ---------------------------------------------------------------------------------------------- isInFrustum, one statement at a time
def test_points_exactly_at_min_and_max_distance_pass():
    # camera centre (1, 2, 3) is column 3 of MtMc; P - centre = (3, 0, 4): dist = sqrt((0 + 9) + 0 + 16) = 5 exactly
    T = np.eye(4)
    T[:3, 3] = [1.0, 2.0, 3.0]
    P = [4.0, 2.0, 7.0]
    r = frustum1(P, 5.0, 9.0, Pn=(0.0, 0.0, 1.0), T=T)
    assert r == (10.0, 20.0, 0, 4.0 / 5.0)        # dist == minDistance: not "<"; ratio 1.0 == S[0] -> lower_bound = 0; viewCos = (3*0 + 0*0 + 4*1) / 5
    r = frustum1(P, 2.5, 5.0, T=T)
    assert r is not None and r[2] == 3            # dist == maxDistance: not ">"; ratio 2.0 > 1.728 -> end() -> clamped to 3
    assert frustum1(P, math.nextafter(5.0, 6.0), 9.0, T=T) is None    # one ulp too near
    assert frustum1(P, 1.0, math.nextafter(5.0, 4.0), T=T) is None    # one ulp too far
    assert frustum1(P, 1.0, 9.0, T=T, in_mask=False) is None          # the mirror mask comes first


def test_ratio_equal_to_a_scale_factor_returns_that_index():
    # dist = 5, minDistance = 5 / 1.44 would round: take dist = 1.44 * 2 = 2.88 along z instead, minDistance = 2 -> ratio = 2.88 / 2 = 1.44 exactly
    assert 2.88 / 2.0 == 1.44
    r = frustum1([0.0, 0.0, 2.88], 2.0, 100.0)
    assert r[2] == 2 and r[3] == 1.0              # lower_bound: first factor that is not < ratio
    assert frustum1([0.0, 0.0, math.nextafter(2.88, 3.0)], 2.0, 100.0)[2] == 3
    assert frustum1([0.0, 0.0, math.nextafter(2.88, 2.0)], 2.0, 100.0)[2] == 2
    assert frustum1([0.0, 0.0, 2.4], 2.0, 100.0)[2] == 1   # 2.4 / 2 = 1.2 exactly


def test_ratio_above_the_top_factor_is_clamped():
    assert frustum1([0.0, 0.0, 50.0], 2.0, 100.0)[2] == len(S) - 1
    assert frustum1([0.0, 0.0, 50.0], 0.0, 100.0)[2] == len(S) - 1     # minDistance == 0: infinite ratio, the top level


def test_nan_ratio_gives_level_0_and_nan_distance_passes():
    # dist = 0 and minDistance = 0: ratio = 0 / 0 = NaN, every `factor < NaN` is false -> begin(); viewCos = 0 / 0 = NaN too
    r = frustum1([0.0, 0.0, 0.0], 0.0, 1.0)
    assert r[2] == 0 and math.isnan(r[3])
    # a NaN position: dist = NaN passes both comparisons of :241, level 0
    r = frustum1([math.nan, 0.0, 1.0], 1.0, 2.0)
    assert r is not None and r[2] == 0 and math.isnan(r[3])


def test_distance_zero_gives_a_nan_viewing_cosine():
    r = frustum1([0.0, 0.0, 0.0], -1.0, 1.0)      # dist = 0 lies inside [-1, 1]; ratio = 0 / -1 = -0.0 -> level 0
    assert r is not None and math.isnan(r[3]) and r[2] == 0


def test_viewing_cos_limit_is_never_applied():
    r = frustum1([0.0, 0.0, 2.0], 1.0, 10.0, Pn=(0.0, 0.0, -1.0))   # the point looks away from the camera: viewCos = -1, still in view (:249-250)
    assert r is not None and r[3] == -1.0


def test_lower_bound_is_the_library_bisection():
    for v in (0.5, 1.0, 1.1, 1.2, 1.3, 1.728, 2.0, math.inf, -math.inf):
        assert M.lower_bound(S, v) == sum(1 for s in S if s < v)
    assert M.lower_bound(S, math.nan) == 0


def one_cam_rig(masks=True):
    synth = importlib.import_module("multicol-slam_amd.synth")
    cam = synth.lafida_cameras()[0]
    return dict(cams=[cam], MtMc=[np.eye(4)], MtMc_inv=[np.eye(4)], masks=[synth.mirror_mask(cam)] if masks else None), cam


def points(pos, minD, maxD, flags=None, normal=None):
    n = len(pos)
    return dict(pos=np.array(pos, float).reshape(n, 3), normal=np.tile([0.0, 0.0, 1.0], (n, 1)) if normal is None else np.array(normal, float),
                min_dist=np.full(n, minD, float) if np.isscalar(minD) else np.array(minD, float),
                max_dist=np.full(n, maxD, float) if np.isscalar(maxD) else np.array(maxD, float), flags=np.zeros(n, np.uint8) if flags is None else np.array(flags, np.uint8))


def test_a_point_behind_the_camera_inside_the_mask_is_in_view():
    # the Lafida mirror circle ends before 90 degrees off axis, so only the bounds test (no mask image) lets a point with ptRot.z <= 0 through:
    # (1, 0.5, -0.05) lies 2.6 degrees behind the image plane and still projects to about (660, 379) of the 754 x 480 image
    rig, cam = one_cam_rig(masks=False)
    pos = np.array([[0.3, 0.2, 1.0], [1.0, 0.5, -0.05], [1.0, 0.5, 0.0], [2.0, 1.0, -1.0], [0.05, 0.02, -1.0], [0.05, 0.02, 1.0]])
    uv, fl = O.world_to_cam(np.stack(rig["MtMc_inv"]), rig["cams"], rig["masks"], pos, np.zeros(len(pos), np.int32))
    behind_inside = np.flatnonzero((fl & 3) == 3)     # bit1: ptRot.z <= 0, the bool WorldToCamHom_fast returns; bit0: inside the mirror mask
    assert len(behind_inside) >= 1, fl
    st, vis, ntm, fresh = M.frustum(points(pos, 0.1, 10.0), rig, S, M.new_state(len(pos), 1))
    assert all(st["in_view"][i, 0] == 1 and vis[i] == 1 for i in behind_inside)
    assert np.array_equal(fresh[:, 0], fl & 1) and ntm == int((fl & 1).sum())
    i = int(behind_inside[0])
    assert st["proj_x"][i, 0] == uv[i, 0] and st["proj_y"][i, 0] == uv[i, 1]


def test_a_rejected_slot_keeps_its_other_fields_and_a_skipped_point_everything():
    rig, cam = one_cam_rig()
    pos = [[0.05, 0.02, 1.0]] * 5
    st0 = M.new_state(5, 1)
    st0["in_view"][:], st0["proj_x"][:], st0["proj_y"][:], st0["level"][:], st0["view_cos"][:] = 1, 11.5, 12.5, 2, 0.25
    #            in view   too near  too far   bad          seen
    pts = points(pos, [0.5, 5.0, 0.1, 0.5, 0.5], [5.0, 9.0, 0.2, 5.0, 5.0], flags=[0, 0, 0, M.LP_BAD, M.LP_SEEN])
    st, vis, ntm, fresh = M.frustum(pts, rig, S, st0)
    assert st["in_view"][:, 0].tolist() == [1, 0, 0, 1, 1] and vis.tolist() == [1, 0, 0, 0, 0] and ntm == 1
    for k in ("proj_x", "proj_y", "level", "view_cos"):
        assert np.array_equal(st[k][1:], st0[k][1:]), k       # rejected (in_view cleared only) and skipped (nothing written)
    assert st["proj_x"][0, 0] != 11.5 and st["level"][0, 0] == 3     # dist = 1.0014, ratio 2.003 > 1.728: end(), clamped


# ---------------------------------------------------------------------------------------------- SearchReferencePointsInFrustum: stale flags, the gate, bad points
@pytest.fixture(scope="module")
def tiny():
    """one camera, frame 1 of the synthetic rig; map point k sits on the bearing ray of feature k of that frame and carries its descriptor"""
    fr = M.oracle_frames(32, 1, 300)
    F = fr[1]
    synth = importlib.import_module("multicol-slam_amd.synth")
    rig = M.make_rig(F["cams"], 1, True, synth)
    idx = np.flatnonzero(F["keys"]["octave"] <= 1)[:6]
    pos = np.array([(rig["MtMc"][0] @ np.append(F["rays"][j] * 3.0, 1.0))[:3] for j in idx])
    return F, rig, idx, pos


def stale_state(F, idx, n):
    st = M.new_state(n, 1)
    for k in range(n):
        j = idx[k]
        st["in_view"][k, 0], st["proj_x"][k, 0], st["proj_y"][k, 0] = 1, float(F["keys"]["x"][j]), float(F["keys"]["y"][j])
        st["level"][k, 0], st["view_cos"][k, 0] = int(F["keys"]["octave"][j]), 1.0
    return st


def test_stale_flags_of_a_seen_point_are_searched(tiny):
    F, rig, idx, pos = tiny
    n = len(idx)
    # point 0 comes into view in this call; points 1.. were seen in this frame: the frustum loop skips them, their flags of earlier frames stay set
    # (dist = 3 on a unit ray, minDistance = 2.9: ratio 1.03 -> level 1, whose window takes octaves 0 and 1)
    pts = points(pos, 2.9, 10.0, flags=[0] + [M.LP_SEEN] * (n - 1))
    out = M.search_local_points(pts, rig, stale_state(F, idx, n), F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8))
    assert out["n_to_match"] == 1 and out["fresh"][:, 0].tolist() == [1] + [0] * (n - 1)
    assert out["match"][:, 0].tolist() == idx.tolist()       # every stale slot found its own feature (distance 0)
    assert out["nmatches"] == n and out["assigned"][idx].all()


def test_nothing_is_searched_when_no_slot_came_into_view(tiny):
    F, rig, idx, pos = tiny
    n = len(idx)
    pts = points(pos, 50.0, 100.0, flags=[0] + [M.LP_SEEN] * (n - 1))    # point 0 is too near: nToMatch = 0
    out = M.search_local_points(pts, rig, stale_state(F, idx, n), F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8))
    assert out["n_to_match"] == 0 and out["nmatches"] == 0 and (out["match"] == -1).all() and not out["assigned"].any()
    assert out["state"]["in_view"][:, 0].tolist() == [0] + [1] * (n - 1)    # the stale flags are still there, the gate (:1001) kept the search away


def test_a_bad_point_with_a_stale_flag_is_not_searched(tiny):
    F, rig, idx, pos = tiny
    n = len(idx)
    pts = points(pos, 2.9, 10.0, flags=[0, M.LP_BAD, M.LP_SEEN, M.LP_BAD | M.LP_SEEN] + [0] * (n - 4))
    out = M.search_local_points(pts, rig, stale_state(F, idx, n), F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8))
    want = idx.copy()
    want[[1, 3]] = -1
    assert out["match"][:, 0].tolist() == want.tolist() and out["nmatches"] == n - 2
    assert out["state"]["in_view"][[1, 3], 0].tolist() == [1, 1]            # untouched


def test_scene_conditions_of_the_gpu_tests():
    """checked here, before any GPU run: every branch of isInFrustum has a slot, every level is predicted, 10 .. 90 % of the unskipped slots are in view,
    stale slots are searched and matched"""
    for sc in M.SCENES.values():
        pts, rig, st, desc, mask, F, asg = M.make_scene(**sc)
        out = M.search_local_points(pts, rig, st, desc, mask, F, asg)
        M.check_scene(pts, rig, out)
        # the first 24 points sit exactly on a distance bound in one camera and are in view there
        assert (out["fresh"][:24].sum(axis=1) >= 1).sum() >= 12


# ---------------------------------------------------------------------------------------------- the library's surface
def test_library_exports_the_new_entry_points(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in pkg._capi.EXPORTS, n
    txt = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    assert L.mcs_abi_version() == int(re.search(r"#define MCS_ABI_VERSION (\d+)", txt).group(1))
    for n in NAMES:
        assert re.search(r"\bint %s\(" % n, txt), n


def test_bad_arguments_are_refused(pkg):
    cap, L = pkg._capi, pkg.lib()
    p, r, s, f = cap.LocalPoints(), cap.RigView(), cap.TrackState(), cap.FrameView()
    one = np.zeros(1, np.int32)
    assert L.mcs_frustum(None, C.byref(p), C.byref(r), None, 8, C.byref(s), 0, None, cap.np_ptr(one)) == cap.MCS_ERR_INVALID
    assert b"null" in L.mcs_last_error()
    assert L.mcs_search_local_points(None, C.byref(p), C.byref(r), C.byref(s), None, None, 32, C.byref(f), 3.0, 0.8, 32, 0, None, None, None, None) == cap.MCS_ERR_INVALID
    with pytest.raises(pkg.McsError):
        pkg.check(L.mcs_search_local_points(None, None, None, None, None, None, 32, None, 3.0, 0.8, 32, 0, None, None, None, None))


def test_struct_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "mcs_c.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(mcs_local_points), offsetof(mcs_local_points, n), '
                   'sizeof(mcs_rig_view), offsetof(mcs_rig_view, nr_cams), sizeof(mcs_track_state)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    cap = pkg._capi
    assert got == [C.sizeof(cap.LocalPoints), cap.LocalPoints.n.offset, C.sizeof(cap.RigView), cap.RigView.nr_cams.offset, C.sizeof(cap.TrackState)]
    assert (cap.LP_BAD, cap.LP_SEEN) == (M.LP_BAD, M.LP_SEEN)


def test_facade_search_reference_points_in_frustum_compiles(tmp_path):
    src = tmp_path / "lm.cpp"
    src.write_text('#include "mcs/mcs_facade.hpp"\n'
                   '#include <unordered_map>\n'
                   'struct MP { double X[3]; bool bad; long mnLastFrameSeen; int vis;\n'
                   '  std::vector<bool> mbTrackInView; std::vector<double> mTrackProjX, mTrackProjY, mTrackViewCos;\n'
                   '  std::vector<int> mnTrackScaleLevel; std::vector<uint64_t> d;\n'
                   '  MultiColSLAM::Vec3d GetWorldPos() { return MultiColSLAM::Vec3d{{X[0], X[1], X[2]}}; } MultiColSLAM::Vec3d GetNormal() { return GetWorldPos(); }\n'
                   '  double GetMinDistanceInvariance() { return 1.0; } double GetMaxDistanceInvariance() { return 9.0; } bool isBad() { return bad; }\n'
                   '  void IncreaseVisible() { ++vis; } const uint64_t* GetDescriptorPtr() { return d.data(); } const uint64_t* GetDescriptorMaskPtr() { return d.data(); } };\n'
                   'struct FR { MultiColSLAM::cMultiCamSys_ camSystem; long mnId; std::vector<MP*> mvpMapPoints; std::vector<MultiColSLAM::KeyPoint> mvKeys;\n'
                   '  std::unordered_map<size_t, int> keypoint_to_cam, cont_idx_to_local_cam_idx; std::vector<double> mvScaleFactors; std::vector<uint64_t> d;\n'
                   '  const uint64_t* GetDescriptorRowPtr(int, int r) const { return &d[4 * r]; } const uint64_t* GetDescriptorMaskRowPtr(int, int r) const { return &d[4 * r]; } };\n'
                   'int use(MultiColSLAM::Context& c, FR& F, std::vector<MP*>& local) {\n'
                   '  int n = MultiColSLAM::SearchReferencePointsInFrustum<FR, MP>(c, F, local);\n'
                   '  return n + MultiColSLAM::SearchReferencePointsInFrustum<FR, MP>(c, F, local, 3.0, 0.8, 32, true); }\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])
