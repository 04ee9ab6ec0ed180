"""The argument checks of the grid-window search family (csrc/mcs_window_guard.hip: mcs_search_by_projection, mcs_window_match, mcs_window_best,
mcs_world_to_cam, mcs_rotation_consistency, mcs_frustum, mcs_search_local_points, mcs_search_last_frame, mcs_window_search_frames) on their own, without a
GPU, through tests/cpp/window_guard_driver.cpp.  Driver and guard translation unit are compiled by hipcc in host-only mode with the library's
floating-point flags (as tests/test_extract_plan_cpu.py does); the program makes no HIP call.

The table below was written from the entry points as they stood before the checks were gathered in one file: code and text per case, every text of every
entry point at least once, and, where a case violates two checks ("a+b"), the text of the one that came first.  Shapes: 4 frame features, 3 probes / tracked
features / map points, 2 cameras, 3 levels."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
OK, INVALID, UNSUPPORTED = 0, -1, -4
NULL = "null argument"
DIM = "dim must be 16, 32 or 64"
FRAME_SIZES = "bad sizes (frame features must be <= 65536)"
MASKS = "masks must be given for both sides or neither"
STRIDE = "descriptor stride must be >= dim and a multiple of 4"
LEVEL = "projection level outside [0, nlevels)"
SIZES = "bad sizes"
DEGREE, IMAGE, MIRROR = "bad polynomial degree", "bad image size", "null mirror mask"
RULE, ASSIGNED, MAX_DIST = "unknown window rule", "frame->assigned is required", "max_dist must be >= 0"
ROTATION = "bad variant / sizes / strides"
DEFERRED_LOCAL = "the frustum test and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)"
DEFERRED_TRACKED = "the probes and the search run in order: switch deferred searches off (mcs_ctx_set_async_search)"
RIG = "bad sizes (rig and frame must agree on the cameras)"
POINT, CAMERA, OCTAVE = "map point id outside [0, points->n)", "camera index outside [0, nr_cams)", "key octave outside [0, nlevels)"

EXPECTED = {
    # mcs_search_by_projection
    "projection.ok": (OK, ""), "projection.null": (INVALID, NULL), "projection.dim": (INVALID, DIM), "projection.sizes": (INVALID, FRAME_SIZES),
    "projection.nlevels": (INVALID, FRAME_SIZES), "projection.masks": (INVALID, MASKS), "projection.stride": (INVALID, STRIDE),
    "projection.level": (INVALID, LEVEL), "projection.level_device": (OK, ""),
    "projection.dim+sizes": (INVALID, DIM), "projection.sizes+masks": (INVALID, FRAME_SIZES), "projection.masks+stride": (INVALID, MASKS),
    "projection.stride+level": (INVALID, STRIDE),
    # mcs_window_match / mcs_window_best
    "window.ok": (OK, ""), "window.null": (INVALID, NULL), "window.rule": (INVALID, RULE), "window.rule+dim": (INVALID, RULE), "window.dim": (INVALID, DIM),
    "window.sizes": (INVALID, FRAME_SIZES), "window.dim+sizes": (INVALID, DIM), "window.sizes+masks": (INVALID, FRAME_SIZES),
    "window.masks+stride": (INVALID, MASKS), "window.stride+assigned": (INVALID, STRIDE), "window.assigned": (INVALID, ASSIGNED),
    "window.initialize_unassigned": (OK, ""),
    "best.ok": (OK, ""), "best.max_dist": (INVALID, MAX_DIST), "best.max_dist+null": (INVALID, MAX_DIST), "best.independent_unassigned": (OK, ""),
    "best.skip_taken_unassigned": (INVALID, ASSIGNED),
    # mcs_world_to_cam / mcs_rotation_consistency
    "world_to_cam.ok": (OK, ""), "world_to_cam.null": (INVALID, NULL), "world_to_cam.sizes": (INVALID, SIZES), "world_to_cam.degree": (INVALID, DEGREE),
    "world_to_cam.image": (INVALID, IMAGE),
    "rotation.ok": (OK, ""), "rotation.null": (INVALID, NULL), "rotation.variant": (INVALID, ROTATION), "rotation.stride": (INVALID, ROTATION),
    # mcs_frustum
    "frustum.ok": (OK, ""), "frustum.null": (INVALID, NULL), "frustum.cams": (INVALID, SIZES), "frustum.nlevels": (INVALID, SIZES),
    "frustum.null_array": (INVALID, NULL), "frustum.degree": (INVALID, DEGREE), "frustum.image": (INVALID, IMAGE), "frustum.mirror": (INVALID, MIRROR),
    "frustum.degree_device": (OK, ""), "frustum.empty+degree": (OK, ""), "frustum.stale_level": (OK, ""),
    # mcs_search_local_points
    "local.ok": (OK, ""), "local.null_frame": (INVALID, NULL), "local.null": (INVALID, NULL), "local.cams+dim": (INVALID, SIZES), "local.dim": (INVALID, DIM),
    "local.sizes": (INVALID, FRAME_SIZES), "local.masks": (INVALID, MASKS), "local.stride": (INVALID, STRIDE), "local.deferred+stride": (INVALID, STRIDE),
    "local.deferred": (UNSUPPORTED, DEFERRED_LOCAL), "local.null_array": (INVALID, NULL), "local.empty_null_array": (OK, ""),
    "local.mirror+level": (INVALID, MIRROR), "local.level": (INVALID, LEVEL), "local.level_unseen": (OK, ""), "local.level_out_of_view": (OK, ""),
    "local.level_device": (OK, ""),
    # mcs_search_last_frame
    "last.ok": (OK, ""), "last.null_rig": (INVALID, NULL), "last.null": (INVALID, NULL), "last.dim": (INVALID, DIM), "last.sizes": (INVALID, FRAME_SIZES),
    "last.cams": (INVALID, FRAME_SIZES), "last.rig": (INVALID, RIG), "last.rig+masks": (INVALID, RIG), "last.masks": (INVALID, MASKS),
    "last.stride": (INVALID, STRIDE), "last.deferred": (UNSUPPORTED, DEFERRED_TRACKED), "last.null_array": (INVALID, NULL), "last.null_scales": (INVALID, NULL),
    "last.empty_null_array": (OK, ""), "last.degree": (INVALID, DEGREE), "last.image": (INVALID, IMAGE), "last.mirror": (INVALID, MIRROR),
    "last.point": (INVALID, POINT), "last.point+camera": (INVALID, POINT), "last.camera": (INVALID, CAMERA), "last.null_point+camera": (OK, ""),
    "last.camera+octave": (INVALID, CAMERA), "last.octave": (INVALID, OCTAVE), "last.octave_device": (OK, ""),
    # mcs_window_search_frames
    "frames.ok": (OK, ""), "frames.octave": (OK, ""), "frames.degree": (OK, ""), "frames.dim+sizes": (INVALID, DIM), "frames.sizes+masks": (INVALID, FRAME_SIZES),
    "frames.masks+stride": (INVALID, MASKS), "frames.deferred": (UNSUPPORTED, DEFERRED_TRACKED), "frames.point": (INVALID, POINT),
    "frames.camera": (INVALID, CAMERA), "frames.null_table": (INVALID, NULL),
}


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    exe = tmp_path_factory.mktemp("guards") / "window_guard_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "window_guard_driver.cpp"), os.path.join(CSRC, "mcs_window_guard.hip"), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, rc, text = line.split("\t")
        assert name not in out
        out[name] = (int(rc), text)
    return out


def test_every_case_ran(results):
    assert sorted(results) == sorted(EXPECTED)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_guard(results, name):
    print(name, results[name])
    assert results[name] == EXPECTED[name]


def test_every_text_of_the_family_is_covered():
    texts = {t for _, t in EXPECTED.values()}
    assert texts >= {NULL, DIM, FRAME_SIZES, MASKS, STRIDE, LEVEL, SIZES, DEGREE, IMAGE, MIRROR, RULE, ASSIGNED, MAX_DIST, ROTATION, DEFERRED_LOCAL, DEFERRED_TRACKED,
                     RIG, POINT, CAMERA, OCTAVE}


def test_each_text_is_written_once():
    """the entry points keep no second copy of a check: each text of the family is a literal of the guard file alone (the polynomial degree's of mcs_host.h,
    where the extractor's camera conversion shares it)"""
    family = [os.path.join(CSRC, n) for n in ("mcs_window_guard.hip", "mcs_window.h", "mcs_capi_window.hip", "mcs_capi_track.hip", "mcs_host.h")]
    src = {p: open(p).read() for p in family}
    for text in {t for _, t in EXPECTED.values() if t}:
        lit = '"%s"' % text
        counts = {os.path.basename(p): s.count(lit) for p, s in src.items() if lit in s}
        assert counts == {"mcs_host.h" if text == DEGREE else "mcs_window_guard.hip": 1}, (text, counts)
