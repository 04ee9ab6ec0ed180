"""Hostile inputs for the detection chain (FAST / AGAST cells, masks, oct-tree, orientation): seeded numpy generators, and the table of cases that
tests/test_oracle_hostile_cpu.py (oracle == the definition / the reference's own code, and the conditions that keep a case from passing vacuously) and
tests/test_gpu_hostile_inputs.py (device == oracle, bit for bit) both walk.  Plain module: numpy and the CPU oracle only, nothing of the device.

What the usual synthetic scene never gives the kernels (csrc/mcs_fast.hip, mcs_octree.hip, mcs_orient.h):
  noise      uniform 0..255: hundreds of compass survivors and kept corners per cell — several trips of the survivor loops (a trip is one workgroup: 128 / 256 entries)
  binary     0 / 255 per pixel: v +- t and the 8-bit score at their limits (score 254), corners at threshold 254, none at 255
  dots4      isolated dots on a flat field: every candidate has the same response (the oct-tree chooses among equals), m10 = m01 = 0 -> fastAtan2(0, 0)
  dots5inv   the same in negative on a 5-px grid (the bright side of the segment test)
  checker4   4 x 4 checkerboard: no corner at all on level 0, corners only where the resize blends the squares
  plateau    noise quantised to four grey levels: equal differences, equal scores next to each other (strict-greater suppression)
  const255   nothing anywhere, at the top of the grey range
Masks (the kernels' rule is `!= 0` through the composed nearest-neighbour map): zero, ones (value 1), randval (0 or 1..255 per pixel), left_dead (whole cells dead,
the boundary inside cells), only_under / its complement (only the level-0 pixels the mask pyramid samples under chosen candidates are live / dead)."""
import ctypes as C
import importlib

import numpy as np

import oracle_lib as O

synth = importlib.import_module("multicol-slam_amd.synth")

SEED = 1
IMAGES = ("noise", "binary", "dots4", "dots5inv", "checker4", "plateau", "const255")
MASKS = ("zero", "ones", "randval", "left_dead", "only_under", "not_under")
MIN_BORDER = 22   # EDGE_THRESHOLD - 3: the candidates' and the oct-tree's origin inside a level


def _noise_binary(h, w, seed):
    rng = np.random.default_rng(seed)          # one generator, noise first
    noise = rng.integers(0, 256, (h, w)).astype(np.uint8)
    binary = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
    return noise, binary


def image(name, h, w, seed=SEED):
    if name == "noise":
        return _noise_binary(h, w, seed)[0]
    if name == "binary":
        return _noise_binary(h, w, seed)[1]
    if name == "dots4":
        img = np.zeros((h, w), np.uint8)
        img[::4, ::4] = 255
        return img
    if name == "dots5inv":
        img = np.full((h, w), 255, np.uint8)
        img[1::5, 2::5] = 0
        return img
    if name == "checker4":
        yy, xx = np.mgrid[0:h, 0:w]
        return ((((yy // 4) + (xx // 4)) & 1) * 255).astype(np.uint8)
    if name == "plateau":
        return (_noise_binary(h, w, seed)[0] // 64 * 64).astype(np.uint8)
    if name == "const255":
        return np.full((h, w), 255, np.uint8)
    raise KeyError(name)


def mask(name, h, w, seed=SEED):
    """the masks that need nothing but the size (only_under / not_under: only_under())"""
    if name == "full":
        return np.full((h, w), 255, np.uint8)
    if name == "zero":
        return np.zeros((h, w), np.uint8)
    if name == "ones":
        return np.ones((h, w), np.uint8)
    if name == "randval":
        rng = np.random.default_rng(seed + 1000)
        live = rng.integers(0, 2, (h, w))
        return (live * rng.integers(1, 256, (h, w))).astype(np.uint8)
    if name == "left_dead":
        m = np.full((h, w), 255, np.uint8)
        m[:, :w // 2] = 0
        return m
    raise KeyError(name)


def level_sizes(w, h, scaleFactor=1.2, nlevels=8, **_):
    ws, hs = (C.c_int * nlevels)(), (C.c_int * nlevels)()
    L = O.lib()
    L.orc_level_sizes.restype = None
    L.orc_level_sizes.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.orc_level_sizes(w, h, scaleFactor, nlevels, ws, hs)
    return [(ws[i], hs[i]) for i in range(nlevels)]


def mask_sources(h, w, sizes):
    """per level an int array of the level's shape: the flat level-0 index of the mask pixel that level's mask pixel is a copy of — index images (three byte planes)
    pushed through orc_resize_nearest level by level, exactly as the oracle builds its mask pyramid"""
    assert h * w < (1 << 24) and sizes[0] == (w, h)
    idx = np.arange(h * w, dtype=np.int64).reshape(h, w)
    planes = [np.ascontiguousarray(((idx >> (8 * k)) & 255).astype(np.uint8)) for k in range(3)]
    out = [idx]
    pw, ph = w, h
    for lw, lh in sizes[1:]:
        nxt = []
        for p in planes:
            d = np.zeros((lh, lw), np.uint8)
            O.lib().orc_resize_nearest(O.ptr(p), pw, ph, pw, O.ptr(d), lw, lh, lw)
            nxt.append(d)
        planes, pw, ph = nxt, lw, lh
        out.append(sum(planes[k].astype(np.int64) << (8 * k) for k in range(3)))
    return out


def only_under(h, w, sizes, cands, complement=False):
    """cands: (level, x, y) in level pixels.  Live = exactly the level-0 pixels the mask pyramid samples at those positions (complement: everything but those)"""
    src = mask_sources(h, w, sizes)
    m = np.full(h * w, 255 if complement else 0, np.uint8)
    for l, x, y in cands:
        m[src[l][y, x]] = 0 if complement else 200
    return m.reshape(h, w)


def cam_for(w, h):
    return synth.scaled_camera(synth.lafida_cameras()[0], w, h)


def run_oracle(img, msk, cam, **params):
    """-> (oracle extractor with its taps, keypoints, descriptors, descriptor masks)"""
    ex = O.Extractor(**params)
    ex.cap = params.get("nfeatures", 1000) + 128 * params.get("nlevels", 8) + 64   # room for 4 * nIni keys per level whatever the quota
    kps, d, dm = ex(img, msk, O.make_ocam(cam))
    return ex, kps, d, dm


def chosen_candidates(oex, nlevels, per_level=6):
    """some kept candidates of every level of an (unmasked) oracle run, spread over the level: (level, x, y) in level pixels"""
    out = []
    for l in range(nlevels):
        c = oex.candidates(l)
        pick = c[::max(1, len(c) // per_level)][:per_level]
        out += [(l, int(k["x"]) + MIN_BORDER, int(k["y"]) + MIN_BORDER) for k in pick]
    return out


def make_mask(name, img, cam, params):
    h, w = img.shape
    if name is None:
        return None
    if name in ("only_under", "not_under"):
        oex = run_oracle(img, None, cam, **params)[0]
        nl = params.get("nlevels", 8)
        return only_under(h, w, level_sizes(w, h, **params), chosen_candidates(oex, nl), complement=name == "not_under")
    return mask(name, h, w)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
DETECTORS = {"fast9_16": dict(useAgast=0, fastAgastType=2), "fast7_12": dict(useAgast=0, fastAgastType=1), "fast5_8": dict(useAgast=0, fastAgastType=0),
             "agast5_8": dict(useAgast=1, fastAgastType=0), "agast7_12d": dict(useAgast=1, fastAgastType=1), "agast7_12s": dict(useAgast=1, fastAgastType=2),
             "oast9_16": dict(useAgast=1, fastAgastType=3)}
MODES = {"orb": dict(do_dBrief=0, learnMasks=0), "dbrief": dict(do_dBrief=1, learnMasks=0), "mdbrief": dict(do_dBrief=1, learnMasks=1)}
# (width, height, pyramid).  Which k_fast_cells instance serves an extractor follows from the LARGEST cell of all its levels (launch_fast):
#   g160  levels 160x120 / 133x100 / 111x83, cells 39x38, 45x56, 34x39: the 60-px FAST instance (256 threads) and the 64-px AGAST instance; six cells on level 0
#   g103  one 59 x 59 cell, the widest there is: 63 processed pixels for AGAST_5_8, the last column the 6-bit column code holds
#   g193  levels 193x193 / 161x161, cells 38x38 and 39x39: the 40-px FAST instance (128 threads) and the 44-px AGAST instance (43 rows of three 16-px segments for
#         AGAST_5_8: 129 segments, the only way to a second trip of the compass pass)
#   g260  scale factor 2.5 (k_resize_cols refuses it: k_resize_level serves) and 2.0 (the last k_resize_cols takes)
GEOMS = {"g160": (160, 120, dict(nlevels=3, scaleFactor=1.2)), "g103": (103, 103, dict(nlevels=1, scaleFactor=1.2)),
         "g193": (193, 193, dict(nlevels=2, scaleFactor=1.2)), "g260_25": (260, 200, dict(nlevels=2, scaleFactor=2.5)),
         "g260_20": (260, 200, dict(nlevels=2, scaleFactor=2.0))}
BASE = dict(nfeatures=200, descSize=32, fastThreshold=20)


def _p(geom, det, mode="mdbrief", **over):
    return dict(BASE, **GEOMS[geom][2], **DETECTORS[det], **MODES[mode], **over)


def case(geom, img, msk, params):
    return dict(geom=geom, image=img, mask=msk, params=params)


def cases_detectors(det):
    """a: every detector on every image"""
    out = [case("g160", "noise", None, _p("g160", det, fastThreshold=1))]
    out += [case("g160", im, None, _p("g160", det)) for im in ("noise", "binary", "dots4", "dots5inv", "plateau")]
    out += [case("g103", "noise", None, _p("g103", det))]
    out += [case("g193", "noise", None, _p("g193", det, fastThreshold=t)) for t in (1, 20)]
    return out


def threshold_cases():
    return [(det, t) for det in DETECTORS for t in ((1, 254) if DETECTORS[det]["useAgast"] else (0, 254, 255))]


def cases_thresholds(det, t):
    """b: the ends of the threshold range (FAST accepts 0..255, AGAST 1..254)"""
    return [case("g160", im, None, _p("g160", det, fastThreshold=t)) for im in ("binary", "noise")]


ANGLE_VARIANTS = {"orb": dict(mode="orb"), "dbrief": dict(mode="dbrief"), "mdbrief": dict(mode="mdbrief"), "mdbrief16": dict(mode="mdbrief", descSize=16),
                  "mdbrief64": dict(mode="mdbrief", descSize=64), "nfeat20": dict(mode="mdbrief", nfeatures=20)}


def cases_angle_ties(variant):
    """c: angle exactly 0, every response equal"""
    p = _p("g160", "fast9_16", **ANGLE_VARIANTS[variant])
    return [case("g160", im, None, p) for im in (("dots4",) if variant == "nfeat20" else ("dots4", "dots5inv"))]


PYRAMID_DETECTORS = ("fast9_16", "agast7_12s")


def cases_pyramid(geom, det):
    """d: scale factors 2.5 and 2.0"""
    return [case(geom, im, None, _p(geom, det)) for im in ("noise", "binary")]


MASK_DETECTORS = ("fast9_16", "fast5_8", "agast7_12s")


def cases_masks(det):
    """e: every mask on noise"""
    return [case("g160", "noise", m, _p("g160", det)) for m in MASKS]


STALE_BATCH = [("noise", "randval"), ("const255", "ones"), ("dots4", "full"), ("binary", "left_dead"), ("noise", "zero"), ("checker4", "full")]


def cases_stale():
    """f: one extractor, dense and empty images in one batch and one after the other"""
    return [case("g160", im, m, _p("g160", "fast9_16")) for im, m in STALE_BATCH] + [case("g160", "const255", None, _p("g160", "fast9_16"))]


def all_cases():
    """every geometry x image x mask x parameter case of tests/test_gpu_hostile_inputs.py, once each, grouped for the CPU file's parametrisation"""
    groups = {}
    for det in DETECTORS:
        groups["a-" + det] = cases_detectors(det)
    for det, t in threshold_cases():
        groups["b-%s-%d" % (det, t)] = cases_thresholds(det, t)
    for v in ANGLE_VARIANTS:
        groups["c-" + v] = cases_angle_ties(v)
    for g in ("g260_25", "g260_20"):
        for det in PYRAMID_DETECTORS:
            groups["d-%s-%s" % (g, det)] = cases_pyramid(g, det)
    for det in MASK_DETECTORS:
        groups["e-" + det] = cases_masks(det)
    groups["f"] = cases_stale()
    return groups


def inputs(c):
    """-> image, mask (or None), camera of a case"""
    w, h, _ = GEOMS[c["geom"]]
    img, cam = image(c["image"], h, w), cam_for(w, h)
    return img, make_mask(c["mask"], img, cam, c["params"]), cam
