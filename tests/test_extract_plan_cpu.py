"""The extractor's plan (csrc/mcs_plan.hip: level geometry, FAST cells, slot / dense / selection ranges, oct-tree roots, resize taps, mask maps) on its own,
without a GPU, through tests/cpp/plan_driver.cpp.  The driver and the plan's translation unit are compiled by hipcc in host-only mode with the library's
floating-point flags (plain g++ cannot read csrc/mcs_common.h: its structs hold HIP streams and events and carry __host__ __device__ members); the program makes no HIP call.

Shapes: 754x480 (Lafida), 160x120, 400x300 and a portrait 120x400 at scale 1.2, 160x120 at 2.0 and 2.5, 345x532 at 1.5 (only its top levels lack an oct-tree
root), AGAST types 0-3.  Each asks for 8 levels; where the geometry does not hold 8 (160x120 at 1.2: level 6 would be 40 rows, below the 44-px border) the plan is
checked with as many as fit, and one level more must be refused as too small."""
import ctypes as C
import os
import subprocess

import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
INVALID, UNSUPPORTED = -1, -4
TOO_SMALL = ("image too small for the requested number of levels (a level is narrower than its 44-px border, or level 0 has no 30-px FAST cell) "
             "or too large")
OCTREE = "aspect ratio / features per level outside the oct-tree kernel's capacity (nIni <= 32, nfeatures_level+3 <= 2048)"
LEVEL_FIELDS = ("w h nfeat nIni nCols nRows wCell hCell capc cellBase slotBase denseBase denseCap selBase selCap tabX tabY colsOk mapX mapY stride").split()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan") / "plan_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "plan_driver.cpp"),
                           os.path.join(CSRC, "mcs_plan.hip"), "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k != "MCS_PYR_CHAIN"}
    cache = {}

    def run(w, h, nlevels=8, sf=1.2, nfeatures=1000, agast=0, typ=2):
        key = (w, h, nlevels, sf, nfeatures, agast, typ)
        if key not in cache:
            cache[key] = parse(subprocess.check_output([str(exe)] + [str(v) for v in key], env=env).decode())
        return cache[key]
    return run


def parse(text):
    lines = text.splitlines()
    rc = int(lines[0].split()[1])
    if rc != 0:
        assert lines[1].startswith("err ")
        return dict(rc=rc, err=lines[1][4:])
    p = dict(rc=0, levels=[], cells=[], taps=[], maps=[])
    for ln in lines[1:]:
        kind, vals = ln.split(" ", 1)
        vals = [int(v) for v in vals.split()]
        if kind == "hd":
            p.update(zip("nlevels kpCap cellsPerImage slotsPerImage densePerImage selPerImage pyrBytes ncells ntaps nmaps".split(), vals))
        elif kind == "umax":
            p["umax"] = vals
        elif kind == "level":
            p["levels"].append(dict(zip(LEVEL_FIELDS, vals)))
        elif kind == "cell":
            p["cells"].append(dict(zip("level x0 y0 cw ch slot".split(), vals)))
        elif kind == "tap":
            p["taps"].append(tuple(vals))
        else:
            assert kind == "map"
            p["maps"].append(vals[0])
    assert len(p["levels"]) == p["nlevels"] and len(p["cells"]) == p["ncells"] and len(p["taps"]) == p["ntaps"] and len(p["maps"]) == p["nmaps"]
    return p


def oracle_levels(w, h, sf, nlevels, nfeatures):
    ws, hs, nf = (C.c_int * nlevels)(), (C.c_int * nlevels)(), (C.c_int * nlevels)()
    O.lib().orc_level_sizes(w, h, C.c_float(sf), nlevels, ws, hs)
    O.lib().orc_features_per_level(nfeatures, C.c_float(sf), nlevels, nf)
    return list(ws), list(hs), list(nf)


def levels_that_fit(w, h, sf, want=8):
    """the largest level count <= want whose every level keeps at least one pixel inside its 22-px borders (EDGE_THRESHOLD - 3 on either side)"""
    ws, hs, _ = oracle_levels(w, h, sf, want, 1000)
    n = 0
    while n < want and ws[n] - 44 >= 1 and hs[n] - 44 >= 1:
        n += 1
    return n


SHAPES = [(754, 480, 1.2, 0, 2), (160, 120, 1.2, 0, 2), (400, 300, 1.2, 0, 2), (160, 120, 2.0, 0, 2), (160, 120, 2.5, 0, 2), (120, 400, 1.2, 0, 2),
          (345, 532, 1.5, 0, 2), (400, 300, 1.2, 1, 0), (400, 300, 1.2, 1, 1), (400, 300, 1.2, 1, 2), (400, 300, 1.2, 1, 3)]


@pytest.mark.parametrize("w,h,sf,agast,typ", SHAPES)
def test_plan(driver, w, h, sf, agast, typ):
    nl = levels_that_fit(w, h, sf)
    assert nl >= 1
    if nl < 8:
        more = driver(w, h, nl + 1, sf, 1000, agast, typ)
        assert (more["rc"], more["err"]) == (UNSUPPORTED, TOO_SMALL)
    p = driver(w, h, nl, sf, 1000, agast, typ)
    assert p["rc"] == 0 and p["nlevels"] == nl
    L = p["levels"]
    # level sizes, feature quotas, the orientation disc: the oracle's
    ws, hs, nf = oracle_levels(w, h, sf, nl, 1000)
    assert [l["w"] for l in L] == ws and [l["h"] for l in L] == hs and [l["nfeat"] for l in L] == nf
    um = (C.c_int * 17)()
    O.lib().orc_umax(um)
    assert p["umax"] == list(um)
    # oct-tree roots and the rows per image
    for l in L:
        assert l["nIni"] == round((l["w"] - 44) / (l["h"] - 44))   # cvRound of the inner region's aspect ratio (both round half to even)
    assert p["kpCap"] == sum(max(l["nfeat"] + 3, 4 * l["nIni"]) for l in L)
    # cells: slot ranges disjoint, in level order, ending at slotsPerImage; a cell that is not skipped lies inside its level
    end, ncell = 0, 0
    for i, l in enumerate(L):
        assert l["cellBase"] == ncell and l["slotBase"] == end
        cells = p["cells"][ncell:ncell + l["nCols"] * l["nRows"]]
        assert len(cells) == l["nCols"] * l["nRows"]
        if l["w"] - 44 < 30 or l["h"] - 44 < 30:   # less than one 30-px cell inside the borders: an empty level
            assert i > 0 and (l["nCols"], l["nRows"], l["wCell"], l["hCell"], l["capc"]) == (0, 0, 0, 0, 0)
        else:
            assert l["nCols"] >= 1 and l["nRows"] >= 1 and l["capc"] >= 1
        for c in cells:
            assert c["level"] == i and c["slot"] == end
            end += l["capc"]
            if c["cw"] > 0 and c["ch"] > 0:
                assert 0 <= c["x0"] and c["x0"] + c["cw"] <= l["w"] and 0 <= c["y0"] and c["y0"] + c["ch"] <= l["h"]
        ncell += len(cells)
    assert end == p["slotsPerImage"] and ncell == p["cellsPerImage"] == len(p["cells"])
    for base, cap, total in (("denseBase", "denseCap", "densePerImage"), ("selBase", "selCap", "selPerImage")):
        end = 0
        for l in L:
            assert l[base] == end and l[cap] >= 0
            end += l[cap]
        assert end == p[total]
    for l in L:
        assert l["denseCap"] == l["nCols"] * l["nRows"] * l["capc"] and l["selCap"] >= l["nfeat"] + 3
    # taps: sources inside the level below, weights summing to 2048 (sat_short saturates at +-32767 / -32768 only)
    assert L[0]["colsOk"] == 0 and L[0]["tabX"] == L[0]["tabY"] == 0
    ntap = 0
    for i in range(1, nl):
        l, P = L[i], L[i - 1]
        assert l["tabX"] == ntap and l["tabY"] == ntap + l["w"]
        for taps, lim in ((p["taps"][l["tabX"]:l["tabX"] + l["w"]], P["w"]), (p["taps"][l["tabY"]:l["tabY"] + l["h"]], P["h"])):
            for ofs, a0, a1 in taps:
                assert 0 <= ofs <= lim - 1
                if a0 not in (-32768, 32767) and a1 not in (-32768, 32767):
                    assert a0 + a1 == 2048
        ntap += l["w"] + l["h"]
    assert ntap == len(p["taps"])
    # mask maps: level-0 coordinates
    nmap = 0
    for l in L:
        assert l["mapX"] == nmap and l["mapY"] == nmap + l["w"]
        assert all(0 <= v < w for v in p["maps"][l["mapX"]:l["mapX"] + l["w"]])
        assert all(0 <= v < h for v in p["maps"][l["mapY"]:l["mapY"] + l["h"]])
        nmap += l["w"] + l["h"]
    assert nmap == len(p["maps"])


def test_cases_reach_the_special_levels(driver):
    """the shapes above do hold what they are there for: an empty level, levels without an oct-tree root next to levels with one, AGAST's other cell capacity"""
    p = driver(160, 120, 2, 2.5)
    assert (p["levels"][1]["w"], p["levels"][1]["h"]) == (64, 48) and p["levels"][1]["nCols"] == 0 and p["ncells"] == p["levels"][0]["nCols"] * p["levels"][0]["nRows"]
    assert all(l["nIni"] == 0 for l in driver(120, 400, levels_that_fit(120, 400, 1.2))["levels"])
    roots = [l["nIni"] for l in driver(345, 532, levels_that_fit(345, 532, 1.5), 1.5)["levels"]]
    assert roots[0] == 1 and roots[-1] == 0
    fast = driver(400, 300)["levels"][0]
    assert fast["capc"] == ((fast["wCell"] + 1) // 2) * ((fast["hCell"] + 1) // 2)
    for typ, border in ((0, 1), (1, 3), (2, 2), (3, 3)):
        l = driver(400, 300, 8, 1.2, 1000, 1, typ)["levels"][0]
        assert l["capc"] == ((l["wCell"] + 6 - 2 * border) * (l["hCell"] + 6 - 2 * border) + 1) // 2
        c = driver(400, 300, 8, 1.2, 1000, 1, typ)["cells"][0]
        assert (c["x0"], c["y0"]) == (22 + border, 22 + border)


@pytest.mark.parametrize("args,code,text", [
    ((160, 120, 8, 1.2, 1000), UNSUPPORTED, TOO_SMALL),      # level 6 is 40 rows
    ((60, 60, 1, 1.2, 1000), UNSUPPORTED, TOO_SMALL),        # level 0 without a 30-px cell
    ((754, 480, 8, 1.2, 20000), UNSUPPORTED, OCTREE),        # 4341 features on level 0
    ((4000, 120, 1, 1.2, 1000), UNSUPPORTED, OCTREE),        # 3956 x 76 inside the borders: 52 roots
    ((4140, 480, 1, 1.2, 1000), UNSUPPORTED, TOO_SMALL),     # 4096 px inside the borders
    ((480, 4140, 1, 1.2, 1000), UNSUPPORTED, TOO_SMALL),
])
def test_refusals(driver, args, code, text):
    p = driver(*args)
    assert (p["rc"], p.get("err")) == (code, text)
