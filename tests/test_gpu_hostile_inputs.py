"""-m gpu: the detection chain on hostile inputs (tests/hostile_inputs.py), device against oracle, bit for bit: per-level images (raw and blurred), candidates
(position, response, order), the oct-tree's selection, and end to end every keypoint field as bits, descriptors, descriptor masks and rays.
tests/test_oracle_hostile_cpu.py pins the expected values (definition, the reference's own code) and checks that every input does what it is there for.

  a  every detector (FAST 9_16 / 7_12 / 5_8, AGAST types 0..3) on noise, 0/255 noise, dot grids and plateaus: dense cells (several trips of k_fast_cells' survivor
     loops in every instance), saturated pixels and scores, the widest cell (59 px; 63 processed pixels for AGAST_5_8)
  b  the ends of the threshold range (FAST 0 / 254 / 255, AGAST 1 / 254)
  c  angle exactly 0 and a level full of equal responses, in every descriptor mode and size, and at the nfeat + 3 / 4 * nIni edge of the keypoint capacity
  d  scale factor 2.5 (k_resize_level by default) and 2.0 (the last k_resize_cols takes)
  e  masks: zero, the value 1, random values, dead cells, live pixels only under chosen candidates / everywhere else; one mask through the three ways in
  f  one extractor, dense and empty images mixed in a batch and run one after the other"""
import ctypes as C

import numpy as np
import pytest

import hostile_inputs as H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


_ORACLE = {}


def oracle_of(G, c):
    """the oracle's run of a case, computed once: (inputs, extractor with its taps, keypoints, descriptors, descriptor masks, rays)"""
    key = (c["geom"], c["image"], c["mask"], tuple(sorted(c["params"].items())))
    if key not in _ORACLE:
        img, msk, cam = H.inputs(c)
        oex, kps, d, dm = H.run_oracle(img, msk, cam, **c["params"])
        rays = np.zeros((len(kps), 3))
        if len(kps):
            G.O.lib().orc_rays(G.O.make_ocam(cam), G.O.ptr(kps), len(kps), G.O.ptr(rays))
        _ORACLE[key] = ((img, msk, cam), oex, kps, d, dm, rays)
    return _ORACLE[key]


def oracle_blurred(G, oex, level):
    """the oracle blurs a level only when it has keypoints (the reference does); the device blurs every level: the same 5 x 5 box over the reflect-101 frame"""
    if len(oex.selected(level)):
        return oex.level_image(level, blurred=True)
    raw, b = oex.level_image(level), 25
    h, w = raw.shape
    buf = np.zeros((h + 2 * b, w + 2 * b), np.uint8)
    buf[b:b + h, b:b + w] = raw
    G.O.lib().orc_border_reflect101(G.O.ptr(buf), w, h, w + 2 * b, b)
    G.O.lib().orc_box5_inplace(C.c_void_p(buf.ctypes.data + b * buf.strides[0] + b), w, h, w + 2 * b)
    return buf[b:b + h, b:b + w].copy()


def check_outputs(G, got, c, tag):
    """end to end: every keypoint field as bits, descriptors, descriptor masks, rays"""
    _, oex, kps, d, dm, rays = oracle_of(G, c)
    gk, gd, gm, gr = got
    assert len(gk) == len(kps), (tag, "keypoints", len(gk), len(kps))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert G.first_diff(gk[f].view(np.uint32), kps[f].view(np.uint32)) is None, (tag, f, G.first_diff(gk[f].view(np.uint32), kps[f].view(np.uint32)))
    assert G.first_diff(gd, d) is None, (tag, "descriptors", G.first_diff(gd, d))
    assert G.first_diff(gm, dm) is None, (tag, "descriptor masks", G.first_diff(gm, dm))
    assert G.first_diff(np.asarray(gr).view(np.uint64), rays.view(np.uint64)) is None, (tag, "rays")


def check_stages(G, ex, i, c, tag):
    """image i of the extractor's last batch, stage by stage: the first stage that differs names the kernel"""
    _, oex, kps, d, dm, rays = oracle_of(G, c)
    for l in range(c["params"]["nlevels"]):
        assert G.first_diff(ex.tap_level(i, l), oex.level_image(l)) is None, (tag, "level", l, G.first_diff(ex.tap_level(i, l), oex.level_image(l)))
        assert G.first_diff(ex.tap_level(i, l, blurred=True), oracle_blurred(G, oex, l)) is None, (tag, "blurred level", l)
    for l in range(c["params"]["nlevels"]):
        x, y, s = ex.tap_candidates(i, l)
        k = oex.candidates(l)
        assert len(x) == len(k), (tag, "candidates of level", l, len(x), len(k))
        diff = G.first_diff(np.stack([x, y, s], 1), np.stack([k["x"], k["y"], k["response"]], 1).astype(np.int32))
        assert diff is None, (tag, "candidates of level", l, diff)
    for l in range(c["params"]["nlevels"]):
        x, y, s = ex.tap_selected(i, l)
        k = oex.selected(l)
        diff = G.first_diff(np.stack([x + H.MIN_BORDER, y + H.MIN_BORDER, s], 1), np.stack([k["x"], k["y"], k["response"]], 1).astype(np.int32))
        assert diff is None, (tag, "oct-tree selection of level", l, diff)


def tag_of(c):
    p = c["params"]
    return "%s/%s/%s t=%d det=%d.%d" % (c["geom"], c["image"], c["mask"], p["fastThreshold"], p["useAgast"], p["fastAgastType"])


def run_batches(G, cases):
    """the cases grouped by geometry and parameters: one extractor and ONE batch per group (the images of a batch differ, their masks too)"""
    groups = {}
    for c in cases:
        groups.setdefault((c["geom"], tuple(sorted(c["params"].items()))), []).append(c)
    n = 0
    for (geom, _), cs in groups.items():
        w, h, _ = H.GEOMS[geom]
        inp = [oracle_of(G, c)[0] for c in cs]
        masks = None if all(m is None for _, m, _ in inp) else [m if m is not None else H.mask("full", h, w) for _, m, _ in inp]
        ex = G.mcs.Extractor(G.ctx(), w, h, max_batch=len(cs), **cs[0]["params"])
        res = ex.extract_host([im for im, _, _ in inp], masks, [G.mcs.make_ocam(cam) for _, _, cam in inp])
        ex.status()
        for i, c in enumerate(cs):
            check_stages(G, ex, i, c, tag_of(c))
            check_outputs(G, res[i], c, tag_of(c))
            n += len(res[i][0])
        ex.close()
    return n


@pytest.mark.parametrize("det", list(H.DETECTORS))
def test_detectors_on_hostile_images(G, det):
    assert run_batches(G, H.cases_detectors(det)) > 1500


@pytest.mark.parametrize("det,t", H.threshold_cases())
def test_threshold_extremes(G, det, t):
    n = run_batches(G, H.cases_thresholds(det, t))
    assert (n == 0) == (t == 255), n


@pytest.mark.parametrize("variant", list(H.ANGLE_VARIANTS))
def test_angle_zero_and_mass_ties(G, variant):
    assert run_batches(G, H.cases_angle_ties(variant)) > 20


@pytest.mark.parametrize("det", H.PYRAMID_DETECTORS)
@pytest.mark.parametrize("geom", ["g260_25", "g260_20"])
def test_pyramid_paths_at_large_scale_factors(G, geom, det):
    assert run_batches(G, H.cases_pyramid(geom, det)) > 300


@pytest.mark.parametrize("det", H.MASK_DETECTORS)
def test_masks(G, det):
    cases = H.cases_masks(det)
    run_batches(G, cases)                       # one batch: every image has its own mask
    w, h, _ = H.GEOMS["g160"]
    zero = [c for c in cases if c["mask"] == "zero"][0]
    ex = G.mcs.Extractor(G.ctx(), w, h, max_batch=1, **zero["params"])
    (img, msk, cam), _, kps, _, _, _ = oracle_of(G, zero)
    got = ex.extract_host([img], [msk], [G.mcs.make_ocam(cam)])[0]
    ex.status()                                 # a clean status, and nothing at all
    assert len(got[0]) == 0 and len(kps) == 0 and all(len(ex.tap_candidates(0, l)[0]) == 0 for l in range(3))
    ex.close()


@pytest.mark.parametrize("det", H.MASK_DETECTORS)
def test_mask_delivery_paths_agree(G, det):
    """the same mask per call from host memory, resident on the device (set_masks), and in a device-kind call with padded mask rows"""
    c = [c for c in H.cases_masks(det) if c["mask"] == "randval"][0]
    (img, msk, cam), oex, kps, d, dm, rays = oracle_of(G, c)
    h, w = img.shape
    oc = [G.mcs.make_ocam(cam)]
    ex = G.mcs.Extractor(G.ctx(), w, h, max_batch=1, **c["params"])
    a = ex.extract_host([img], [msk], oc)[0]
    check_stages(G, ex, 0, c, "host mask")
    check_outputs(G, a, c, "host mask")
    ex.set_masks([msk])
    b = ex.extract_host([img], "resident", oc)[0]
    check_stages(G, ex, 0, c, "resident mask")
    check_outputs(G, b, c, "resident mask")
    stride = w + 14
    padded = np.full((h, stride), 77, np.uint8)    # live bytes between the rows: a reader with the wrong stride keeps candidates it should drop
    padded[:, :w] = msk
    cap = ex.cap
    d_img, d_msk = G.DevBuf(img), G.DevBuf(padded)
    d_nkp, d_kps = G.DevBuf(np.zeros(1, np.int32)), G.DevBuf(np.zeros((1, cap), G.mcs.KP_DTYPE))
    d_desc, d_dm, d_rays = G.DevBuf(np.zeros((1, cap, 32), np.uint8)), G.DevBuf(np.zeros((1, cap, 32), np.uint8)), G.DevBuf(np.zeros((1, cap, 3)))
    ex.extract_device(1, d_img.ptr.value, w * h, w, d_msk.ptr.value, h * stride, stride, oc, d_nkp.ptr.value, d_kps.ptr.value, d_desc.ptr.value, d_dm.ptr.value,
                      d_rays.ptr.value)
    G.ctx().synchronize()
    ex.fix_ties()                                  # device-kind rows get the host's rounding at the cvRound ties on request (tests/test_gpu_tiefix.py)
    ex.status()
    n = int(d_nkp.read()[0])
    assert n == len(kps)
    check_stages(G, ex, 0, c, "device mask, padded rows")
    check_outputs(G, (d_kps.read()[0, :n], d_desc.read()[0, :n], d_dm.read()[0, :n], d_rays.read()[0, :n]), c, "device mask, padded rows")
    ex.close()


def test_stale_state_and_mixed_batches(G):
    """dense, empty and fully masked images side by side in a batch, then the same in reverse order (every slot gets what its neighbour had), then one empty image:
    nothing of an earlier image or call may survive in the counts, lists and level buffers"""
    cases = H.cases_stale()
    batch, single = cases[:6], cases[6]
    w, h, _ = H.GEOMS["g160"]
    ex = G.mcs.Extractor(G.ctx(), w, h, max_batch=6, **batch[0]["params"])
    for order in (batch, batch[::-1]):
        inp = [oracle_of(G, c)[0] for c in order]
        res = ex.extract_host([im for im, _, _ in inp], [m for _, m, _ in inp], [G.mcs.make_ocam(cam) for _, _, cam in inp])
        ex.status()
        for i, c in enumerate(order):
            check_stages(G, ex, i, c, "slot %d %s" % (i, tag_of(c)))
            check_outputs(G, res[i], c, "slot %d %s" % (i, tag_of(c)))
    assert sum(len(oracle_of(G, c)[2]) == 0 for c in batch) == 2 and sum(len(oracle_of(G, c)[2]) >= 100 for c in batch) == 4
    (img, _, cam) = oracle_of(G, single)[0]
    res = ex.extract_host([img], None, [G.mcs.make_ocam(cam)])
    ex.status()
    check_stages(G, ex, 0, single, "single empty image after dense batches")
    check_outputs(G, res[0], single, "single empty image after dense batches")
    assert len(res[0][0]) == 0
    ex.close()
