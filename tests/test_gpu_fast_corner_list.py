"""The one-wave FAST 9/16 instance suppresses and emits over a CORNER list (csrc/mcs_fast.hip, pass 2: the survivors with a score, compacted to the front of the
survivor list in list order by two ballots and a running total): device against oracle, bit for bit, on cells built for that compaction — `tap_candidates`
(position, response, order) and end to end every keypoint field as bits, descriptors, descriptor masks and rays, the way tests/test_gpu_fast_one_wave.py does it
(its geometry, numpy definitions and dots are reused here).  Every cell of every image lists 1024 survivors or fewer: the list path (the overflow cases are in that
file).  The last test (not gpu) proves on the CPU that every input has the survivor counts, corner counts and parities it claims.

One level of 163 x 163: 3 x 3 cells of (40, 40, 33) x (40, 40, 33) px.  The survivor list is row-major over the cell's pixels, pass 2 gives a lane the entries 2 m
and 2 m + 1 and takes 128 entries per trip, pass 3 takes 64 corners per trip.

  band      rows of a 1-px checkerboard of LOW amplitude (0 / 40) over the whole width of a cell and 3 px beyond it on both sides, from 3 rows outside the grid (the
            image's border, which no cell processes) k rows into the cell, followed by one row of 0 / 23 and one of 0 / 6.  All four compass points of a pixel have
            the other colour, so the k + 1 rows of 0 / 40 and 0 / 23 are survivors (40 and 23 > t = 20): S = cw (k + 1).  None is a corner: a dark centre's compass
            points are dark, so no arc of 9 is brighter; a bright centre's ring is bright at the twelve other places of the rows above and beside it, and of the two
            ring pixels one row further in (k = 3 and 13 from a top band), which are 17 below the centre at most: no arc of 9 is darker by more than 20.  The 3
            columns beyond the cell belong to the neighbour (cells 1 and 7), which sees the band's end there: corners of its own, whatever the oracle says.
            A band enters a cell of the top row from above and a cell of the bottom row from below.
  dots      (that file's) bright dots on the lattice x + 2 y = 0 (mod 4): survivors = corners (score 254) = kept candidates.  Below a top band (4 rows away) the dots
            follow the band's survivors in the list; above a bottom band they lead it.
So a cell with a band of S survivors and D dots lists ns = S + D survivors and nc = D corners; the oracle keeps exactly the D dots, in row-major order, and
  top band:     dot j is list entry S + j  (S odd: dot 0 is the SECOND entry of its lane's pair, after a non-corner; S even: dots pair up, "both"),
  bottom band:  dot j is list entry j      (D odd: the last dot is the FIRST entry of its pair, before a non-corner),
  corner list:  dot j is entry j either way; 64 dots are one trip of pass 3, 65 are two.
ns odd: the last lane of pass 2 reads its entry twice (the last dot of a top band with S + D odd: it must be listed once; a band survivor of a bottom band).
The dots of a top band of S = 200, 231 (360, 330) survivors are list entries that cross 256 (384): the running total is carried from one pass-2 trip into the next.

  smooth    a 24 x 24 patch of that file's smooth texture on black at threshold 0, in two cells: hundreds of ADJACENT corners, with equal and with unequal scores, on
            the list path (strict-greater suppression among neighbours from the corner list; the whole texture overflows the list in that file).
  mask      a mirror mask that is dead under one dot in the middle of a cell's emission order (dot 30 of 65 without a band, dot 64 of 65 — the second pass-3 trip —
            under a band)."""
import numpy as np
import pytest

import hostile_inputs as H
import test_gpu_fast_one_wave as W

S = W.S
CS = W.cells(S, S)
TOP, BOTTOM = (0, 2), (6, 8)
AMP, STEP = 40, 17


def band(img, c, k):
    """k full rows of the band inside cell c (+ the row of 0 / 23: survivors, + the row of 0 / 6: none) -> the rows of the cell it touches"""
    x0, y0, cw, ch = CS[c]
    xx = np.arange(x0 - 3, x0 + cw + 3)
    for r, amp in enumerate([AMP] * (k + 3) + [AMP - STEP, AMP - 2 * STEP]):
        y = y0 - 3 + r if c in TOP else y0 + ch + 2 - r
        img[y, xx] = np.where((xx + y) & 1, amp, 0)
    return k + 2


def dot_points(c, k, D):
    """the first D lattice points of cell c that keep 4 rows from its band"""
    x0, y0, cw, ch = CS[c]
    skip = k + 2 + 4 if k is not None and c in TOP else 0
    pts = [p for p in W.lattice(CS[c]) if p[1] >= y0 + skip]
    assert len(pts) >= D and (D == 0 or k is None or c in TOP or pts[D - 1][1] < y0 + ch - (k + 2) - 4), (c, k, D)
    return pts[:D]


# image -> {cell: (band rows k or None, dots D)}; S = cw * (k + 1)
LAYOUT = {
    "zero_corners": {0: (3, 0), 2: (7, 0), 6: (3, 0)},                       # 160, 264, 160 survivors, no corner
    "trips_a": {0: (4, 64), 2: (6, 65), 6: (3, 7), 8: (4, 8)},              # 200 + 64 | 231 + 65 (S odd) | 7 dots + 160 (D odd, ns odd) | 8 dots + 165 (ns odd)
    "trips_b": {0: (8, 65), 2: (9, 64), 6: (1, 65), 8: (0, 1)},             # 360 + 65 | 330 + 64 | 65 dots + 80 | 1 dot + 33
    "parity": {0: (3, 9), 2: (2, 10), 4: (None, 2), 6: (0, 1), 8: (1, 3)},  # 160 + 9 (ns odd, last a corner) | 99 + 10 (S odd, ns odd, last a corner) | ...
    "masked": {0: (4, 65), 4: (None, 65)},
}
MASKED = {0: 64, 4: 30}   # "masked": cell -> the dot under the dead mask pixel


def survivors_of(c, k):
    return 0 if k is None else CS[c][2] * (k + 1)


def image(name):
    img = np.zeros((S, S), np.uint8)
    if name == "smooth_patch":
        full = W.image("smooth")
        for c, (ox, oy) in {0: (7, 9), 4: (8, 8)}.items():   # (cell 4: the patch starts on the texture's period; cell 0: off it)
            x0, y0 = CS[c][0] + ox, CS[c][1] + oy
            img[y0:y0 + 24, x0:x0 + 24] = full[y0:y0 + 24, x0:x0 + 24]
        return img
    for c, (k, D) in LAYOUT[name].items():
        if k is not None:
            band(img, c, k)
        for x, y in dot_points(c, k, D):
            img[y, x] = 255
    return img


def mask_of(name):
    if name != "masked":
        return None
    m = np.full((S, S), 255, np.uint8)
    for c, j in MASKED.items():
        k, D = LAYOUT[name][c]
        x, y = dot_points(c, k, D)[j]
        m[y, x] = 0
    return m


CASES = {n: 20 for n in LAYOUT}
CASES["smooth_patch"] = 0
GROUPS = {"t20": list(LAYOUT), "smooth_t0": ["smooth_patch"]}

_ORACLE = {}


def oracle_of(name):
    if name not in _ORACLE:
        img, msk = image(name), mask_of(name)
        cam = H.cam_for(S, S)
        oex, kps, d, dm = H.run_oracle(img, msk, cam, **W.params(CASES[name], 1))
        _ORACLE[name] = (img, msk, cam, oex, kps, d, dm)
    return _ORACLE[name]


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


def check(G, ex, i, got, name, tag):
    img, msk, cam, oex, kps, d, dm = oracle_of(name)
    x, y, s = ex.tap_candidates(i, 0)
    k = oex.candidates(0)
    assert len(x) == len(k), (tag, "candidates", len(x), len(k))
    diff = G.first_diff(np.stack([x, y, s], 1), np.stack([k["x"], k["y"], k["response"]], 1).astype(np.int32))
    assert diff is None, (tag, "candidates", diff)
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
    return len(k)


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_corner_list_cells_equal_the_oracle(G, group):
    names = GROUPS[group]
    ex = G.mcs.Extractor(G.ctx(), S, S, max_batch=len(names), **W.params(CASES[names[0]], 1))
    runs = [list(range(len(names)))]
    if len(names) > 1:
        runs.append(runs[0][::-1])   # the same batch in reverse order: every slot gets what its neighbour had
    total = 0
    for order in runs:
        inp = [oracle_of(names[j]) for j in order]
        masks = None if all(o[1] is None for o in inp) else [o[1] if o[1] is not None else H.mask("full", S, S) for o in inp]
        res = ex.extract_host([o[0] for o in inp], masks, [G.mcs.make_ocam(o[2]) for o in inp])
        ex.status()
        for i, j in enumerate(order):
            total += check(G, ex, i, res[i], names[j], "%s slot %d %s" % (group, i, names[j]))
    ex.close()
    assert total > 0


# ---- CPU: the inputs do their job ------------------------------------------------------------------------------------------------------------------------------------------
def listed(img, cell, t):
    """the survivor list of a cell (row-major) as flags: is the entry a corner"""
    return (W.scores(img, cell, t) > 0)[W.compass(img, cell, t)]


def cands_in(cands, cell):
    x0, y0, cw, ch = cell
    x, y = cands["x"].astype(int) + W.MB, cands["y"].astype(int) + W.MB
    return cands[(x >= x0) & (x < x0 + cw) & (y >= y0) & (y < y0 + ch)]


def test_inputs_do_their_job():
    assert [CS[c][2:] for c in (0, 2, 4, 6, 8)] == [(40, 40), (33, 40), (40, 40), (40, 33), (33, 33)]
    seen = set()
    for name, layout in LAYOUT.items():
        img, msk, cam, oex, kps, d, dm = oracle_of(name)
        for c, cell in enumerate(CS):
            fl = listed(img, cell, 20)
            assert len(fl) <= W.CAP, (name, c, len(fl))                                    # the list path, every cell
            assert int((W.scores(img, cell, 20) > 0).sum()) == int(fl.sum()), (name, c)    # (a pixel with a score is a survivor)
            if c not in layout:
                if c not in (1, 7):   # (the bands' neighbours)
                    assert len(fl) == 0, (name, c)
                    seen.add("no survivor")
                continue
            k, D = layout[c]
            Sv = survivors_of(c, k)
            want = [False] * Sv + [True] * D if c in TOP or k is None else [True] * D + [False] * Sv
            assert fl.tolist() == want, (name, c, len(fl), int(fl.sum()))                  # ns = S + D, nc = D, and where the corners are in the list
            kc = cands_in(oex.candidates(0), cell)
            dead = MASKED.get(c) if name == "masked" else None
            pts = [p for j, p in enumerate(dot_points(c, k, D)) if j != dead]
            assert [(int(q["x"]) + W.MB, int(q["y"]) + W.MB) for q in kc] == pts and (kc["response"] == 254).all(), (name, c)   # the kept candidates: the dots, in order
            pairs = [(bool(fl[i]), bool(fl[i + 1]) if i + 1 < len(fl) else None) for i in range(0, len(fl), 2)]   # what the lanes of pass 2 hold
            if D == 0 and Sv > 128:
                seen.add("zero corners")
            for lo, hi in ((128, 256), (256, 384)):
                if D in (64, 65) and lo < Sv <= hi and Sv + D > hi:
                    seen.add("%d corners, list past %d, across a pass-2 trip" % (D, lo))
            if (False, True) in pairs:
                seen.add("second entry only")
            if (True, False) in pairs:
                seen.add("first entry only")
            if (True, True) in pairs:
                seen.add("both entries")
            if len(fl) % 2 and Sv > 0:
                seen.add("odd list, last a corner" if fl[-1] else "odd list, last no corner")
            if dead is not None:
                seen.add("mask, trip %d of the emission" % (dead // 64))
    assert seen == {"no survivor", "zero corners", "second entry only", "first entry only", "both entries", "odd list, last a corner", "odd list, last no corner",
                    "mask, trip 0 of the emission", "mask, trip 1 of the emission"} | {"%d corners, list past %d, across a pass-2 trip" % (D, lo) for D in (64, 65) for lo in (128, 256)}, seen
    # 64 / 65 corners with 129 ... and 257 ... survivors in front of them, each of the four
    assert {(survivors_of(c, k), D) for n in ("trips_a", "trips_b") for c, (k, D) in LAYOUT[n].items() if c in TOP} == {(200, 64), (231, 65), (360, 65), (330, 64)}

    # the smooth patch at threshold 0: adjacent corners with equal and with unequal scores, kept candidates among them, on the list path
    img, msk, cam, oex, kps, d, dm = oracle_of("smooth_patch")
    for c, cell in enumerate(CS):
        fl = listed(img, cell, 0)
        assert len(fl) <= W.CAP, ("smooth_patch", c, len(fl))
        if c in (0, 4):
            sc = W.scores(img, cell, 0)
            both = (sc[:, 1:] > 0) & (sc[:, :-1] > 0)
            assert int(fl.sum()) > 128 and len(fl) > int(fl.sum()), (c, len(fl), int(fl.sum()))   # several trips of both lists, and survivors that are no corners
            assert int((both & (sc[:, 1:] == sc[:, :-1])).sum()) >= 5 and int((both & (sc[:, 1:] != sc[:, :-1])).sum()) >= 50, c
            assert len(cands_in(oex.candidates(0), cell)) >= 3, c
    assert len(kps) >= 6
