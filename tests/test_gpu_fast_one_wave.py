"""FAST 9/16 on cells of up to 40 px is one wave per cell with a bounded survivor list (csrc/mcs_fast.hip: FastThreads, kFastListCap): device against oracle, bit for
bit, on cells built for every path of that instance — `tap_candidates` (position, response, order) per level, and end to end every keypoint field as bits,
descriptors, descriptor masks and rays (the way tests/test_gpu_hostile_inputs.py does it).  The last test (not gpu) proves on the CPU that every input does its job.

A survivor is a pixel that passes the compass test (two ADJACENT compass points, 3 px away, both darker than v - t or both brighter than v + t).  Two textures give a
cell an exact survivor count:
  dots      bright dots on the lattice  x + 2 y = 0 (mod 4)  of a black image.  None of the sixteen ring offsets is a lattice vector, so a dot's whole ring is
            background (a corner, score 254); the difference of two adjacent compass offsets is (+-3, +-3), no lattice vector either, so a background pixel never sees
            two adjacent compass points lit; no two dots touch, so every dot survives the suppression.  Survivors = corners = kept candidates = the dots, for ANY subset
            of the lattice; a 40 x 40 cell holds 400 lattice points, its slot capacity exactly.
  checker   a 1-px checkerboard: all four compass points of a pixel have the other colour, so EVERY pixel is a survivor, and none is a corner (the ring alternates).
  smooth    127 + 45 (cos(2 pi x / 16) + cos(2 pi y / 16)) at threshold 0: 1363 of a 40 x 40 cell's 1600 pixels have a non-zero FAST score, next to each other.
Counts 1, 64, 65 and 400 are dots; the list's capacity (1024) and the capacity + 1 are 25 rows of checkerboard (1000 survivors) and 24 / 25 dots seven rows below
it; "every pixel of the cell" is a cell of checkerboard, 1600 survivors.

What is asserted about a cell is independent of how the kernel cuts it into trips: a survivor count <= the capacity stays on the list (0 / 255 noise at threshold
0: ~900 survivors, many trips of every loop); a count above it MUST leave the list path somewhere — the capacity + 1, the checkerboard cell, "noise_tail" (0 / 255
noise under 22 rows of checkerboard: corners among the unlisted survivors) and the smooth texture, where more pixels have a non-zero FAST score (closed form of the
kernel's header comment, a lower bound on the survivors) than the list holds, so the walk of the score tile suppresses among many ADJACENT scores.

Geometry (30-px grid on the level minus its 22-px border; cell = ceil(inner / floor(inner / 30))): a 40-px cell needs an inner size of 118 or 119 px, THREE cells
(163 x 163: cells of 40, 40, 33); four cell columns are at most 38 px wide (193 px: 38, 38, 38, 29); a last column narrower than 16 px needs 13 columns (435 px: 13 px,
one partly valid segment); a last row of 3 rows / 1 row needs 23 / 25 cell rows (735 / 795 px).  Those two images are as small as the grid allows."""
import os
import re

import numpy as np
import pytest

import hostile_inputs as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 1024   # kFastListCap of csrc/mcs_fast.hip (checked below)
MB = H.MIN_BORDER


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


# ---- geometry: the FAST cells of a level (src/mdBRIEFextractorOct.cpp:886-906 as csrc/mcs_plan.hip restates it) -------------------------------------------------------
def cells(w, h):
    """-> [(x0, y0, cw, ch)] in cell row-major order: the processed pixels of every cell, in level coordinates"""
    maxBX, maxBY = w - MB, h - MB
    wd, ht = maxBX - MB, maxBY - MB
    nC, nR = wd // 30, ht // 30
    wC, hC = -(-wd // nC), -(-ht // nR)
    out = []
    for i in range(nR):
        for j in range(nC):
            iniY, iniX = MB + i * hC, MB + j * wC
            maxY, maxX = min(iniY + hC + 6, maxBY), min(iniX + wC + 6, maxBX)
            skip = iniY >= maxBY - 3 or iniX >= maxBX - 6
            out.append((iniX + 3, iniY + 3, 0 if skip else max(0, maxX - iniX - 6), 0 if skip else max(0, maxY - iniY - 6)))
    return out


# ---- the definitions in numpy ----------------------------------------------------------------------------------------------------------------------------------------------
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]   # (dx, dy), k = 0..15


def ring_diffs(img, cell):
    """d[k] = v - I[k] for every pixel of the cell: (16, ch, cw)"""
    x0, y0, cw, ch = cell
    I = img.astype(np.int32)
    v = I[y0:y0 + ch, x0:x0 + cw]
    return np.stack([v - I[y0 + dy:y0 + dy + ch, x0 + dx:x0 + dx + cw] for dx, dy in RING])


def compass(img, cell, t):
    """the compass test of csrc/mcs_fast.hip (fast_quick): two adjacent compass points both darker or both brighter -> bool (ch, cw)"""
    d = ring_diffs(img, cell)[[0, 4, 8, 12]]
    hi, lo = d > t, d < -t
    return np.any([hi[k] & hi[(k + 1) % 4] for k in range(4)], 0) | np.any([lo[k] & lo[(k + 1) % 4] for k in range(4)], 0)


def scores(img, cell, t):
    """the closed form of the kernel's header comment: A = max over the 16 arcs of 9 contiguous k of min d, B = the same of -d; score = max(A, B) - 1 where max(A, B) > t"""
    d = ring_diffs(img, cell)
    A = np.max([np.min([d[(k + j) % 16] for j in range(9)], 0) for k in range(16)], 0)
    B = np.max([np.min([-d[(k + j) % 16] for j in range(9)], 0) for k in range(16)], 0)
    best = np.maximum(A, B)
    return np.where(best > t, best - 1, 0)


# ---- the images ----------------------------------------------------------------------------------------------------------------------------------------------------------
def lattice(cell):
    x0, y0, cw, ch = cell
    return [(x, y) for y in range(y0, y0 + ch) for x in range(x0, x0 + cw) if (x + 2 * y) % 4 == 0]


def dots(img, cell, k):
    for x, y in lattice(cell)[:k]:
        img[y, x] = 255


def checker(img, cell, rows):
    x0, y0, cw, ch = cell
    yy, xx = np.mgrid[y0:y0 + rows, x0:x0 + cw]
    img[y0:y0 + rows, x0:x0 + cw] = ((xx + yy) & 1) * 255


def binary(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, (h, w)) * 255).astype(np.uint8)


S = 163   # 3 x 3 cells: (40, 40, 33) x (40, 40, 33); cells 0, 1, 3, 4 are 40 x 40
COUNTS = {0: 1, 1: 64, 3: 65, 4: 0, 2: 10, 7: 330, 8: 7}                     # "dots": cell -> survivors (cell 7 is 40 x 33: all of its 330 lattice points)
FULL = {0: CAP, 1: CAP + 1, 3: 1600, 2: 0, 5: 0}                             # "full": cell -> survivors; cell 4 is "noise_tail"


def image(name):
    cs = cells(S, S)
    if name == "dots":
        img = np.zeros((S, S), np.uint8)
        for c, k in COUNTS.items():
            dots(img, cs[c], k)
        return img
    if name == "lattice400":
        img = np.zeros((S, S), np.uint8)
        dots(img, cs[4], 400)
        return img
    if name == "full":
        img = np.zeros((S, S), np.uint8)
        checker(img, cs[0], 25)
        checker(img, cs[1], 25)
        checker(img, cs[3], 40)
        checker(img, cs[4], 22)                                              # noise_tail: 22 rows of checkerboard, 0 / 255 noise in the 18 rows below
        x0, y0, cw, ch = cs[4]
        img[y0 + 22:y0 + ch, x0:x0 + cw] = binary(ch - 22, cw, 5)
        for c in (0, 1):                                                     # dots in rows 32..35 bring the checkerboard's count to the exact figure
            need = FULL[c] - int(compass(img, cs[c], 20).sum())
            pts = [p for p in lattice(cs[c]) if cs[c][1] + 32 <= p[1] < cs[c][1] + 36]
            assert 0 < need <= len(pts), (c, need)
            for x, y in pts[:need]:
                img[y, x] = 255
        return img
    if name == "empty":
        return np.zeros((S, S), np.uint8)
    if name == "smooth":
        yy, xx = np.mgrid[0:S, 0:S]
        return np.round(127 + 45 * (np.cos(2 * np.pi * xx / 16) + np.cos(2 * np.pi * yy / 16))).astype(np.uint8)
    if name == "binary":
        return H.image("binary", S, S)
    if name == "four_cols":
        return H.image("noise", S, 193)
    if name == "thin3":
        return H.image("noise", 735, 435)
    if name == "thin1":
        return H.image("noise", 795, 435)
    raise KeyError(name)


def params(t, nlevels):
    return dict(H.BASE, nlevels=nlevels, scaleFactor=1.2, fastThreshold=t, **H.DETECTORS["fast9_16"], **H.MODES["mdbrief"])


# name -> (threshold, levels); the groups are one extractor and ONE batch each
CASES = {"dots": (20, 1), "lattice400": (20, 1), "full": (20, 1), "empty": (20, 1), "smooth": (0, 1), "binary": (0, 2), "four_cols": (20, 2), "thin3": (20, 1), "thin1": (20, 1)}
GROUPS = {"counts": ["dots", "empty", "full", "lattice400", "empty"], "smooth_t0": ["smooth"], "binary_t0": ["binary"], "four_cols": ["four_cols"], "thin3": ["thin3"], "thin1": ["thin1"]}

_ORACLE = {}


def oracle_of(name):
    """the oracle's run of a case, computed once: (image, camera, extractor with its taps, keypoints, descriptors, descriptor masks)"""
    if name not in _ORACLE:
        img = image(name)
        cam = H.cam_for(img.shape[1], img.shape[0])
        t, nl = CASES[name]
        oex, kps, d, dm = H.run_oracle(img, None, cam, **params(t, nl))
        _ORACLE[name] = (img, cam, oex, kps, d, dm)
    return _ORACLE[name]


# ---- device against oracle -------------------------------------------------------------------------------------------------------------------------------------------------
def check(G, ex, i, got, name, tag):
    img, cam, oex, kps, d, dm = oracle_of(name)
    for l in range(CASES[name][1]):
        x, y, s = ex.tap_candidates(i, l)
        k = oex.candidates(l)
        assert len(x) == len(k), (tag, "candidates of level", l, len(x), len(k))
        diff = G.first_diff(np.stack([x, y, s], 1), np.stack([k["x"], k["y"], k["response"]], 1).astype(np.int32))
        assert diff is None, (tag, "candidates of level", l, diff)
    rays = np.zeros((len(kps), 3))
    if len(kps):
        G.O.lib().orc_rays(G.O.make_ocam(cam), G.O.ptr(kps), len(kps), G.O.ptr(rays))
    gk, gd, gm, gr = got
    assert len(gk) == len(kps), (tag, "keypoints", len(gk), len(kps))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert G.first_diff(gk[f].view(np.uint32), kps[f].view(np.uint32)) is None, (tag, f, G.first_diff(gk[f].view(np.uint32), kps[f].view(np.uint32)))
    assert G.first_diff(gd, d) is None, (tag, "descriptors", G.first_diff(gd, d))
    assert G.first_diff(gm, dm) is None, (tag, "descriptor masks", G.first_diff(gm, dm))
    assert G.first_diff(np.asarray(gr).view(np.uint64), rays.view(np.uint64)) is None, (tag, "rays")
    return len(oex.candidates(0))


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_one_wave_cells_equal_the_oracle(G, group):
    names = GROUPS[group]
    t, nl = CASES[names[0]]
    imgs = [oracle_of(n)[0] for n in names]
    h, w = imgs[0].shape
    ex = G.mcs.Extractor(G.ctx(), w, h, max_batch=len(names), **params(t, nl))
    runs = [list(range(len(names)))]
    if len(names) > 1:
        runs.append(runs[0][::-1])   # the same batch in reverse order: every slot gets what its neighbour had
    total = 0
    for order in runs:
        res = ex.extract_host([imgs[j] for j in order], None, [G.mcs.make_ocam(oracle_of(names[j])[1]) for j in order])
        ex.status()
        for i, j in enumerate(order):
            total += check(G, ex, i, res[i], names[j], "%s slot %d %s" % (group, i, names[j]))
    ex.close()
    assert total > 0


# ---- CPU: the inputs do their job ------------------------------------------------------------------------------------------------------------------------------------------
def kept_in(cands, cell):
    x0, y0, cw, ch = cell
    x, y = cands["x"].astype(int) + MB, cands["y"].astype(int) + MB
    return int(((x >= x0) & (x < x0 + cw) & (y >= y0) & (y < y0 + ch)).sum())


def test_inputs_do_their_job():
    src = open(os.path.join(ROOT, "multicol-slam_amd", "csrc", "mcs_fast.hip")).read()
    assert int(re.search(r"kFastListCap = (\d+);", src).group(1)) == CAP
    cs = cells(S, S)
    assert [c[2:] for c in cs] == [(40, 40), (40, 40), (33, 40), (40, 40), (40, 40), (33, 40), (40, 33), (40, 33), (33, 33)]   # the widest cell of the instance
    assert all(len(lattice(cs[c])) == 400 for c in (0, 1, 3, 4))

    # dots: survivors = corners = kept candidates, cell by cell; 0, 1, 64 (one full trip of the suppression loop), 65, and 400 = every slot of the cell
    img, _, oex, kps, _, _ = oracle_of("dots")
    for c, cell in enumerate(cs):
        k = COUNTS.get(c, 0)
        assert int(compass(img, cell, 20).sum()) == k and int((scores(img, cell, 20) > 0).sum()) == k and kept_in(oex.candidates(0), cell) == k, ("dots", c)
    assert len(oex.candidates(0)) == sum(COUNTS.values()) and (oex.candidates(0)["response"] == 254).all() and {0, 1, 64, 65} <= set(COUNTS.values())
    img, _, oex, kps, _, _ = oracle_of("lattice400")
    assert int(compass(img, cs[4], 20).sum()) == 400 and kept_in(oex.candidates(0), cs[4]) == 400 and len(oex.candidates(0)) == 400

    # the capacity itself fits the list; one more cannot, and the dots are what the cell then has to find without it
    img, _, oex, kps, _, _ = oracle_of("full")
    for c, k in FULL.items():
        assert int(compass(img, cs[c], 20).sum()) == k, ("full", c, int(compass(img, cs[c], 20).sum()))
    dot_rows = lambda c: (cs[c][0], cs[c][1] + 32, 40, 4)   # (the checkerboard's first row holds corners too: its white pixels have nine black ring pixels above and beside them)
    assert kept_in(oex.candidates(0), dot_rows(0)) == CAP - 1000 and kept_in(oex.candidates(0), dot_rows(1)) == CAP + 1 - 1000
    # every pixel of a cell, next to an empty one; and noise under the checkerboard: kept corners among the unlisted survivors
    assert kept_in(oex.candidates(0), cs[2]) == 0 and int(compass(img, cs[5], 20).sum()) == 0
    x0, y0, cw, ch = cs[4]
    assert int(compass(img, cs[4], 20).sum()) > CAP + 100 and kept_in(oex.candidates(0), (x0, y0 + 23, cw, ch - 23)) >= 5
    assert len(kps) > 20

    # the smooth texture at threshold 0: in every 40 x 40 cell more pixels have a non-zero FAST score than the list holds (a lower bound on the survivors, so the
    # cell certainly leaves the list path), they lie next to each other, and the suppression keeps a few of them
    img, _, oex, kps, _, _ = oracle_of("smooth")
    for c in (0, 1, 3, 4):
        sc = scores(img, cs[c], 0) > 0
        assert int(sc.sum()) > CAP and int(sc.sum()) <= int(compass(img, cs[c], 0).sum()), (c, int(sc.sum()))
        assert int((sc[:, 1:] & sc[:, :-1]).sum()) > CAP and kept_in(oex.candidates(0), cs[c]) >= 5, c
    assert len(kps) > 50

    # 0 / 255 noise at threshold 0, two levels: ~900 survivors in every 40-px cell, within the capacity (long lists: many trips of the arc score and the suppression loop)
    img, _, oex, kps, _, _ = oracle_of("binary")
    for c in (0, 1, 3, 4):
        assert 800 < int(compass(img, cs[c], 0).sum()) <= CAP, c
        assert int((scores(img, cs[c], 0) > 0).sum()) >= 10
    assert H.level_sizes(S, S, 1.2, 2) == [(163, 163), (136, 136)] and len(oex.candidates(0)) > 100 and len(oex.candidates(1)) > 50 and len(kps) > 100

    # four cell columns (38, 38, 38, 29) beside rows of 40, served by the 40-px instance on both levels; noise: more kept corners than one trip of 64 in a cell
    assert H.level_sizes(193, S, 1.2, 2) == [(193, 163), (161, 136)]
    cs4 = cells(193, S)
    assert [c[2] for c in cs4[:4]] == [38, 38, 38, 29] and max(max(c[2:]) for c in cs4 + cells(161, 136)) == 40
    img, _, oex, kps, _, _ = oracle_of("four_cols")
    assert max(kept_in(oex.candidates(0), c) for c in cs4) > 64 and len(oex.candidates(1)) > 100

    # a last column of 13 px (one partly valid segment) and a last row of 3 rows / 1 row, with candidates in them
    for name, h, rows, last in (("thin3", 735, 23, 3), ("thin1", 795, 25, 1)):
        ct = cells(435, h)
        assert len(ct) == 13 * rows and ct[12][2] == 13 and ct[-1][2:] == (13, last) and ct[-2][2:] == (31, last) and max(max(c[2:]) for c in ct) == 31
        img, _, oex, kps, _, _ = oracle_of(name)
        assert sum(kept_in(oex.candidates(0), c) for c in ct[12::13]) >= 20, name                 # the narrow column
        assert sum(kept_in(oex.candidates(0), c) for c in ct[-13:]) >= (5 if last == 3 else 1), name   # the short row
        assert len(kps) > 100
