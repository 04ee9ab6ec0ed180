"""CPU: the boundary of mcs_optimize_essential_graph — the library exports it, _capi.EXPORTS lists it, include/mcs_c.h declares it and MCS_ABI_VERSION stays
10 (the entry point is additive: look it up with dlsym); the diagnostics record has the header's layout; and every argument check of
csrc/mcs_essgraph_guard.hip, run alone through tests/cpp/essgraph_guard_driver.cpp (host logic only)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
INVALID, CAPACITY, UNSUPPORTED = -1, -3, -4

GUARDS = {
    "valid": (0, ""), "null_ctx": (INVALID, "null"), "kind": (INVALID, "memory kind"), "negative": (INVALID, "bad sizes"), "null_out": (INVALID, "null"),
    "kfs_4097": (CAPACITY, "4096 keyframes"), "edges": (CAPACITY, "2^17 edges"), "points": (CAPACITY, "2^22 points"), "free_512": (0, ""),
    "free_513": (CAPACITY, "512 free"), "free_513.device": (CAPACITY, "512 free"), "deferred": (UNSUPPORTED, "deferred searches"),
    "edge.beyond": (INVALID, "edge vertex"), "edge.negative": (INVALID, "edge vertex"), "edge.self": (INVALID, "with itself"), "edge.device": (0, ""),
    "ref.beyond": (INVALID, "pt_ref"), "ref.minus2": (INVALID, "pt_ref"), "ref.device": (0, ""),
}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


def test_the_entry_point_is_exported_declared_and_additive(pkg):
    L, cap = pkg.lib(), pkg._capi
    assert hasattr(L, "mcs_optimize_essential_graph") and "mcs_optimize_essential_graph" in cap.EXPORTS
    txt = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    assert re.search(r"\bint\s+mcs_optimize_essential_graph\s*\(", txt) and re.search(r"#define\s+MCS_ABI_VERSION\s+10\b", txt)
    assert L.mcs_abi_version() == 10
    for k, name in enumerate(("MCS_EG_OK", "MCS_EG_NONFINITE", "MCS_EG_NO_FREE_VERTEX", "MCS_EG_FAILED")):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, k), txt)
    assert (cap.EG_OK, cap.EG_NONFINITE, cap.EG_NO_FREE_VERTEX, cap.EG_FAILED) == (0, 1, 2, 3)
    assert C.sizeof(cap.EgDiag) == cap.EG_DIAG_DTYPE.itemsize == 120 and cap.EgDiag.lam.offset == 104 == cap.EG_DIAG_DTYPE.fields["lam"][1]


def test_a_null_context_is_refused(pkg):
    assert pkg.lib().mcs_optimize_essential_graph(None, 0, None, None, None, None, 0, None, None, None, 0, None, None, pkg._capi.MEM_HOST, None, None, None, None) == INVALID


def test_guards(tmp_path):
    exe = tmp_path / "essgraph_guard_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "essgraph_guard_driver.cpp"),
                           os.path.join(CSRC, "mcs_essgraph_guard.hip"), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, rc, text = line.split("\t")
        out[name] = (int(rc), text)
    assert sorted(out) == sorted(GUARDS)
    for name, (rc, text) in GUARDS.items():
        assert out[name][0] == rc and text in out[name][1], (name, out[name])


def test_facade_driver_compiles_and_links(pkg, tmp_path):
    """MultiColSLAM::cOptimizer::OptimizeEssentialGraph of include/mcs/mcs_facade.hpp instantiates over the stand-ins of tests/cpp/facade_driver_essgraph.cpp
    under -Wall -Werror and links against the library (tests/test_gpu_essgraph_facade.py runs it)"""
    exe = tmp_path / "facade_driver_essgraph"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_essgraph.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)], stderr=subprocess.DEVNULL) == 2     # the usage line; no device is touched
