"""CPU-side checks of the covisibility store's boundary: the library exports every mcs_covis_* / row-helper entry point and _capi.EXPORTS lists them, the
C++ facade class compiles, and creating a store without a GPU raises instead of falling back to anything."""
import ctypes as C
import importlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_covis_create", "mcs_covis_destroy", "mcs_covis_clear", "mcs_covis_size", "mcs_covis_slots", "mcs_covis_set_keyframe", "mcs_covis_set_keyframe_pose",
         "mcs_covis_erase_keyframe", "mcs_covis_set_keyframe_bad", "mcs_covis_set_points_bad", "mcs_covis_update_reference", "mcs_covis_update_connections",
         "mcs_gather_rows", "mcs_scatter_rows"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


def test_library_exports_the_store_and_the_row_helpers(pkg):
    L = pkg.lib()
    for n in NAMES:
        assert hasattr(L, n), "libmcs_hip.so does not export %s" % n
        assert n in pkg._capi.EXPORTS, "_capi.EXPORTS does not list %s" % n
    hdr = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    for n in NAMES:
        assert ("int %s(" % n) in hdr, n


def test_facade_use_compiles(tmp_path):
    src = tmp_path / "covis_use.cpp"
    src.write_text('#include "mcs/mcs_facade.hpp"\n'
                   'struct KF { long unsigned int mnId; };\n'
                   'int use(MultiColSLAM::Context& c) {\n'
                   '  MultiColSLAM::cCovisibility<KF> s(c, 8, 16, 100);\n'
                   '  KF a{1}, b{2}; const double t[3] = {0, 0, 0};\n'
                   '  s.SetKeyFrame(&a, {0, 1, 2, -1}); s.SetKeyFrame(&b, {0, 1, 2, 3}); s.SetPose(&a, t); s.SetBadFlag(&b); s.SetPointsBad({3});\n'
                   '  std::vector<int32_t> fp = {0, 1, 2, 3};\n'
                   '  auto r = s.UpdateReference(fp, t, 50);\n'
                   '  auto u = s.UpdateConnections(&a);\n'
                   '  s.EraseKeyFrame(&b); s.clear();\n'
                   '  return (int)r.mvpLocalMapPoints.size() + (int)u.mvOrderedWeights.size() + s.size() + s.slots() + (r.mpReferenceKF ? 1 : 0) + (u.unchanged ? 1 : 0);\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_create_without_a_gpu_raises(pkg):
    n = C.c_int32(-1)
    rc = pkg.lib().mcs_device_count(C.byref(n))
    h = C.c_void_p()
    assert pkg.lib().mcs_covis_create(None, 4, 4, 4, C.byref(h)) != 0 and not h.value     # no context, no store
    with pytest.raises(pkg.McsError):
        pkg._capi.check(pkg.lib().mcs_covis_create(None, 4, 4, 4, C.byref(h)))
    if rc == 0 and n.value > 0:
        return                                                                            # a GPU is present: the rest is the GPU suite's
    FE = importlib.import_module("multicol-slam_amd.frontend")
    with pytest.raises(pkg.McsError):
        FE.cCovisibility(4, 4, 4)
