"""CPU: the expected values of tests/test_gpu_hostile_inputs.py are right, independently of the device.

  1. the oracle's FAST 9/16 equals the brute-force segment-test definition on every hostile image, at both ends of the threshold range;
  2. where oracle/_ref is built, the oracle equals the reference's own extractor code, bit for bit, on every case the GPU file runs (the reference needs a mask: an
     all-255 one where the case has none, and the oracle's result without a mask equals its result with that one);
  3. the inputs do what they are there for (dense cells, equal responses, angle 0, saturated scores, half-dead masks ...), so no GPU case passes vacuously."""
import os
import sys

import numpy as np
import pytest

import hostile_inputs as H
import oracle_lib as O
from test_oracle_primitives_independent import fast_by_definition

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
have_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")
GROUPS = H.all_cases()


def same_extraction(a, b):
    (ka, da, ma), (kb, db, mb) = a, b
    return len(ka) == len(kb) and all(np.array_equal(ka[f].view(np.uint32), kb[f].view(np.uint32)) for f in ka.dtype.names) and np.array_equal(da, db) and np.array_equal(ma, mb)


@pytest.mark.parametrize("name", H.IMAGES)
def test_oracle_fast_9_16_is_the_segment_test_on_hostile_images(name):
    img = H.image(name, 66, 90)
    total = 0
    for t in (0, 1, 20, 253, 254, 255):
        out = np.zeros(8192, O.KP_DTYPE)
        n = O.lib().orc_fast9_16(O.ptr(img), img.shape[1], img.shape[0], img.shape[1], None, 0, t, O.ptr(out), len(out))
        assert n <= len(out)
        got = [(int(k["x"]), int(k["y"]), int(k["response"])) for k in out[:n]]
        assert got == fast_by_definition(img, t), (name, t)
        total += n
    assert (total > 0) == (name not in ("checker4", "const255")), (name, total)   # (a 4 x 4 checkerboard has no 9-arc anywhere)


@have_ref
@pytest.mark.parametrize("group", list(GROUPS))
def test_oracle_equals_reference_code_on_every_gpu_case(group):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_compare as R
    for c in GROUPS[group]:
        img, msk, cam = H.inputs(c)
        _, k, d, m = H.run_oracle(img, msk, cam, **c["params"])
        full = H.mask("full", *img.shape)
        ref = R.run_ref(img, np.ascontiguousarray(msk if msk is not None else full), cam, **c["params"])
        assert same_extraction(ref, (k, d, m)), (group, c["geom"], c["image"], c["mask"], len(ref[0]), len(k))
        if msk is None:
            _, k2, d2, m2 = H.run_oracle(img, full, cam, **c["params"])
            assert same_extraction((k, d, m), (k2, d2, m2)), (group, c["geom"], c["image"], "no mask != all-255 mask")


# ---- input conditions (the oracle alone) -----------------------------------------------------------------------------------------------------------------------------
def run(geom, image, mask=None, det="fast9_16", **over):
    c = H.case(geom, image, mask, H._p(geom, det, **over))
    img, msk, cam = H.inputs(c)
    oex, k, d, m = H.run_oracle(img, msk, cam, **c["params"])
    return oex, k, c


def cell_counts(cands, w_cell, h_cell):
    """FAST: kept candidates per cell (a cell's candidates lie in its own wCell x hCell pixels; AGAST views overlap, so there this counts by position)"""
    cx, cy = cands["x"].astype(int) // w_cell, cands["y"].astype(int) // h_cell
    return np.bincount(cy * 64 + cx)


def test_noise_fills_the_cells_of_both_fast_instances_beyond_one_trip():
    # 60-px instance, 256 threads (g160: its largest cell is 45 x 56): 39 x 38 cells on level 0, 3 x 2 of them
    oex, _, _ = run("g160", "noise")
    assert len(oex.candidates(0)) >= 129 * 6          # [801]: more KEPT corners than 128 per cell on average; the survivors of the compass test are several times that
    # one 59 x 59 cell: more kept candidates than one 256-thread trip
    for det, least in (("fast9_16", 257), ("agast5_8", 257)):
        oex, _, _ = run("g103", "noise", det=det)
        assert len(oex.candidates(0)) >= least, (det, len(oex.candidates(0)))
    # 40-px instance, 128 threads (g193: cells 38 x 38 and 39 x 39): a single cell keeps more than one trip
    for t in (1, 20):
        oex, _, _ = run("g193", "noise", fastThreshold=t)
        assert cell_counts(oex.candidates(0), 38, 38).max() >= 129 and cell_counts(oex.candidates(1), 39, 39).max() >= 129, t
    # ... and odd list lengths occur (the tail of the paired score loop): kept counts of both parities among the cells
    assert len(set(int(v) & 1 for v in cell_counts(oex.candidates(0), 38, 38))) == 2


def test_dots_give_angle_zero_equal_responses_and_the_capacity_edge():
    oex, k, _ = run("g160", "dots4")
    assert int((k["angle"].view(np.uint32) == 0).sum()) >= 50           # [80] +0.0f exactly: fastAtan2(0, 0)
    assert len(np.unique(oex.candidates(0)["response"])) == 1 and len(oex.candidates(0)) > 200
    oex, k, _ = run("g160", "dots4", nfeatures=20)
    assert len(k) > 20                                                  # [24]: a level returns up to quota + 3 / 4 * nIni keys
    oex, k, _ = run("g160", "dots5inv")
    assert len(np.unique(oex.candidates(0)["response"])) == 1 and int((k["angle"].view(np.uint32) == 0).sum()) >= 50


def test_binary_saturates_the_score_and_threshold_255_finds_nothing():
    for det in ("fast9_16", "fast7_12", "fast5_8"):
        _, k, _ = run("g160", "binary", det=det, fastThreshold=254)
        assert len(k) > 0 and (k["response"] == 254).all(), det         # [81 for 9/16]
        _, k, _ = run("g160", "binary", det=det, fastThreshold=255)
        assert len(k) == 0, det
    for det in ("agast5_8", "agast7_12d", "agast7_12s", "oast9_16"):
        _, k, _ = run("g160", "binary", det=det, fastThreshold=254)
        assert len(k) > 0 and (k["response"] == 254).all(), det


def test_checkerboard_has_corners_only_above_level_0():
    oex, k, _ = run("g160", "checker4")
    assert len(oex.candidates(0)) == 0 and len(oex.candidates(1)) > 0 and len(k) > 0


def test_masks_cut_what_they_should():
    free, _, c = run("g160", "noise")
    nl = c["params"]["nlevels"]
    n_free = [len(free.candidates(l)) for l in range(nl)]
    rv, _, _ = run("g160", "noise", "randval")
    assert 0.3 < len(rv.candidates(0)) / n_free[0] < 0.7                # [414 of 801]
    m = H.mask("randval", 120, 160)
    assert ((m > 0) & (m < 255)).sum() > 1000 and (m == 1).any()        # live pixels are not 255
    ld, _, _ = run("g160", "noise", "left_dead")
    x = ld.candidates(0)["x"] + H.MIN_BORDER
    assert x.min() >= 80 and ((x >= 80) & (x < 100)).any()             # the left cell column is dead; the boundary (x = 80) lies inside the middle one (61 .. 99)
    zero, k, _ = run("g160", "noise", "zero")
    assert len(k) == 0
    chosen = H.chosen_candidates(free, nl)
    assert all(sum(1 for c_ in chosen if c_[0] == l) >= 5 for l in range(nl))
    under, k, _ = run("g160", "noise", "only_under")
    for l in range(nl):
        want = set((x, y) for ll, x, y in chosen if ll == l)
        got = set(zip((under.candidates(l)["x"].astype(int) + H.MIN_BORDER).tolist(), (under.candidates(l)["y"].astype(int) + H.MIN_BORDER).tolist()))
        assert want <= got and len(under.candidates(l)) >= len(want), l
    live = (H.inputs(H.case("g160", "noise", "only_under", c["params"]))[1] != 0).sum()
    assert 0 < live <= len(chosen)
    notu, _, _ = run("g160", "noise", "not_under")
    for l in range(nl):
        got = set(zip((notu.candidates(l)["x"].astype(int) + H.MIN_BORDER).tolist(), (notu.candidates(l)["y"].astype(int) + H.MIN_BORDER).tolist()))
        assert not (got & set((x, y) for ll, x, y in chosen if ll == l)), l
        assert len(got) >= n_free[l] - len(chosen)


def test_geometries_have_the_cells_they_are_there_for():
    assert H.level_sizes(160, 120, 1.2, 3) == [(160, 120), (133, 100), (111, 83)]
    assert H.level_sizes(103, 103, 1.2, 1) == [(103, 103)]              # inner width 103 - 44 = 59: one 59-px cell
    assert H.level_sizes(193, 193, 1.2, 2) == [(193, 193), (161, 161)]  # inner 149 -> 4 cells of 38; inner 117 -> 3 cells of 39
    assert H.level_sizes(260, 200, 2.5, 2) == [(260, 200), (104, 80)] and H.level_sizes(260, 200, 2.0, 2) == [(260, 200), (130, 100)]
