"""CPU: the expected values of tests/test_gpu_hostile_cameras.py are right, independently of the device.

  1. the oracle's dBRIEF / mdBRIEF descriptors and masks equal an independent numpy statement of what a descriptor is (hostile_cameras.describe_by_definition), bit
     for bit, on every camera x geometry x mask case and for descriptor sizes 16 / 32 / 64;
  2. the cases reach what they are there for — samples outside the staged patch, in the frame, beyond the frame, beyond the 81 x 81 capture window, pattern points
     outside the G(s) table — and the Lafida controls reach none of the sampling regimes (why the suite never went there before);
  3. where oracle/_ref is built, the oracle equals the reference's own extractor on every case without a sample beyond the frame.  Beyond the frame the reference
     reads outside its buffer (deviation (2) of DESIGN.md section 2): those cases are never handed to it."""
import os
import sys

import numpy as np
import pytest

import hostile_cameras as HC
import hostile_inputs as H
from test_oracle_hostile_cpu import same_extraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
have_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")
VARIANTS = [(m, ds) for m in ("dbrief", "mdbrief") for ds in HC.DESC_SIZES]


def all_cases(geom, mode="mdbrief", ds=32):
    return HC.cases(geom, mode, ds) + HC.small_cases(geom, mode, ds)


@pytest.mark.parametrize("mode,ds", VARIANTS)
@pytest.mark.parametrize("geom", list(HC.GEOMS))
def test_oracle_equals_the_definition(geom, mode, ds):
    compared = 0
    for c in all_cases(geom, mode, ds):
        r = HC.oracle_run(c, keep=(mode, ds) == ("mdbrief", 32))
        d, m, left_out = HC.describe_by_definition(r["levels"], r["keys"], r["inputs"][2], ds, mode)
        n = len(r["kps"])
        assert left_out.sum() <= 0.01 * n, (HC.tag_of(c), int(left_out.sum()), n)   # expected: none (3e-6 per keypoint)
        ok = ~left_out
        assert np.array_equal(d[ok], r["desc"][ok]), (HC.tag_of(c), "descriptors", int((d[ok] != r["desc"][ok]).any(axis=1).sum()), n)
        assert np.array_equal(m[ok], r["dmask"][ok]), (HC.tag_of(c), "masks", int((m[ok] != r["dmask"][ok]).any(axis=1).sum()), n)
        if mode == "dbrief":
            assert not r["dmask"].any()
        compared += int(ok.sum())
    assert compared > 10000, compared


def regime_totals(cs):
    tot = {k: 0 for k in HC.REGIMES}
    for c in cs:
        for k, v in HC.counts(HC.classify_case(c)).items():
            tot[k] += v
    return tot


@pytest.mark.parametrize("geom", list(HC.GEOMS))
def test_the_cases_reach_every_regime_and_the_controls_none(geom):
    cs = all_cases(geom)
    tot = regime_totals(cs)
    print(geom, tot)
    assert tot["in_level_outside_patch"] >= 50 and tot["in_frame"] >= 20 and tot["beyond_frame"] >= 5 and tot["beyond_40"] >= 50 and tot["s_above_table"] >= 1, tot
    assert tot["non_finite"] == 0
    # the capture-slot path: few keypoints in all (the slot holds 64), some of them with a sample outside the 81 x 81 window
    small = [c for c in cs if len(HC.oracle_run(c)["kps"]) <= 64]
    assert any(HC.classify_case(c)["beyond_40"].any() for c in small), [HC.tag_of(c) for c in small]
    # ... and few keypoints with frame samples inside the window and none outside it: the capture alone serves them
    assert any(HC.classify_case(c)["in_frame"].any() and not HC.classify_case(c)["beyond_40"].any() for c in small)
    for c in cs:
        if c["camera"] in HC.CONTROLS:
            cl = HC.counts(HC.classify_case(c))
            assert len(HC.oracle_run(c)["kps"]) > 100
            assert cl["outside_patch"] == cl["in_frame"] == cl["beyond_frame"] == cl["beyond_40"] == 0, (HC.tag_of(c), cl)


def test_camera_table_is_what_it_says():
    w, h = 160, 120
    base = HC.camera("lafida0", w, h)
    for name in ("s115", "shear", "s160", "s320", "shrink"):          # a centred principal point: only the affine terms change
        cam = HC.camera(name, w, h)
        assert (cam["u0"], cam["v0"], cam["p"], cam["invP"]) == (base["u0"], base["v0"], base["p"], base["invP"])
    assert (HC.camera("corner_br", w, h)["u0"], HC.camera("corner_br", w, h)["v0"]) == (w - 27.5, h - 26.5)
    assert HC.camera("flipped", w, h)["p"][0] > 0 > base["p"][0] and len(HC.camera("short", w, h)["invP"]) == 6
    assert len(set(repr(sorted(HC.camera(n, w, h).items())) for n in HC.CAMERAS)) == len(HC.CAMERAS) >= 8
    assert H.level_sizes(400, 300, 1.2, 4) == [(400, 300), (333, 250), (278, 208), (231, 174)]


@have_ref
@pytest.mark.parametrize("mode,ds", [("mdbrief", 16), ("mdbrief", 32), ("mdbrief", 64), ("dbrief", 32)])
@pytest.mark.parametrize("geom", list(HC.GEOMS))
def test_oracle_equals_reference_code_where_no_sample_leaves_the_frame(geom, mode, ds):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import ref_compare as R
    pinned = []
    for c in all_cases(geom, mode, ds):
        r = HC.oracle_run(c, keep=(mode, ds) == ("mdbrief", 32))
        nl = c["params"]["nlevels"]
        cl = HC.classify([r["oex"].level_size(l) for l in range(nl)], r["keys"], r["inputs"][2], ds, mode)
        if cl["beyond_frame"].any():
            continue                                   # the reference would read outside its buffer: not run at all
        img, msk, cam = r["inputs"]
        ref = R.run_ref(img, np.ascontiguousarray(msk if msk is not None else H.mask("full", *img.shape)), cam, **c["params"])
        assert same_extraction(ref, (r["kps"], r["desc"], r["dmask"])), (HC.tag_of(c), len(ref[0]), len(r["kps"]))
        pinned.append(HC.counts(cl))
    assert sum(p["in_level_outside_patch"] for p in pinned) >= 50 and sum(p["in_frame"] for p in pinned) >= 20, pinned
