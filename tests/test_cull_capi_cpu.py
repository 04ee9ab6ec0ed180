"""CPU-side checks of the culling entry points' boundary: the library exports mcs_covis_set_keyframe_octaves / _cull_keyframes / _observations / _cull_points,
_capi.EXPORTS lists them, mcs_c.h declares them, the ABI revision of library and header agree, the four facade members compile, and a call without a store
returns an error instead of crashing."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mcs_covis_set_keyframe_octaves", "mcs_covis_cull_keyframes", "mcs_covis_observations", "mcs_covis_cull_points"]


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


def test_library_exports_the_culling_calls(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    for n in NAMES:
        assert hasattr(L, n), "libmcs_hip.so does not export %s" % n
        assert n in pkg._capi.EXPORTS, "_capi.EXPORTS does not list %s" % n
        assert ("int %s(" % n) in hdr, n


def test_abi_revision(pkg):
    hdr = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    want = int(re.search(r"#define MCS_ABI_VERSION (\d+)", hdr).group(1))
    assert pkg.lib().mcs_abi_version() == want                                    # the four calls are additive: a host finds them with dlsym


def test_facade_use_compiles(tmp_path):
    src = tmp_path / "cull_use.cpp"
    src.write_text('#include "mcs/mcs_facade.hpp"\n'
                   'struct KF { long unsigned int mnId; };\n'
                   'int use(MultiColSLAM::Context& c) {\n'
                   '  MultiColSLAM::cCovisibility<KF> s(c, 8, 16, 100);\n'
                   '  KF a{1}, b{2}, cur{3};\n'
                   '  s.SetKeyFrame(&a, {0, 1, 2, -1}); s.SetKeyFrame(&b, {0, 1, 2, 3});\n'
                   '  s.SetOctaves(&a, {0, 1, 2, 3});\n'
                   '  std::vector<KF*> local = {&b, &a};\n'
                   '  auto r = s.KeyFrameCulling(local);\n'
                   '  auto r2 = s.KeyFrameCulling(local, {1, 0}, 10);\n'
                   '  for (KF* k : r.vpToSetBad) s.EraseKeyFrame(k);\n'
                   '  std::vector<int32_t> n = s.Observations({0, 1, 2});\n'
                   '  std::vector<int32_t> recent = {0, 1};\n'
                   '  std::vector<int32_t> v = s.MapPointCulling(&cur, recent, {1, 2}, {3, 4}, {1, 2});\n'
                   '  return (int)r.vBadPoints.size() + (int)r2.vpToBeErased.size() + (int)n.size() + (int)v.size() + (int)recent.size() + r.verdict[0] + r.nMPs[0] +\n'
                   '         r.nRedundantObservations[0];\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


def test_calls_without_a_store_return_an_error(pkg):
    L = pkg.lib()
    ids, o4, i4, i8, u1 = np.array([1, 2], np.int64), np.zeros(8, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int64), np.zeros(2, np.uint8)
    p = lambda a: a.ctypes.data
    assert L.mcs_covis_cull_keyframes(None, 2, p(ids), None, 4, 0, p(o4), p(o4), p(o4), p(o4), p(o4)) == pkg._capi.MCS_ERR_INVALID
    assert L.mcs_covis_cull_keyframes(None, 0, None, None, 0, 1, None, None, None, None, None) == pkg._capi.MCS_ERR_INVALID
    assert L.mcs_covis_set_keyframe_octaves(None, 1, p(u1), 2, 0) == pkg._capi.MCS_ERR_INVALID
    assert L.mcs_covis_observations(None, p(i4), 2, 0, p(o4)) == pkg._capi.MCS_ERR_INVALID
    assert L.mcs_covis_cull_points(None, 5, 2, p(i4), p(i4), p(i4), p(i8), 0, p(o4)) == pkg._capi.MCS_ERR_INVALID
    with pytest.raises(pkg.McsError):
        pkg._capi.check(L.mcs_covis_cull_keyframes(None, 2, p(ids), None, 4, 0, p(o4), p(o4), p(o4), p(o4), p(o4)))
