"""-m gpu: the descriptor stage on hostile camera models (tests/hostile_cameras.py), device against oracle, bit for bit, through the C ABI: every keypoint field as
bits, descriptors, descriptor masks and rays.  tests/test_oracle_hostile_cameras_cpu.py pins the expected values (an independent definition, the reference's own
code) and checks that the cases reach every regime they are there for.  Every batch holds ALL cameras of the table side by side (14 distinct camera tables).

  default mode     the fast pass with its verdicts "sample outside the staged patch" and "pattern point outside the G(s) table", the fallback list through the exact
                   pass (Sampler::at beyond its first branch: blurred level, reflect-101 frame, clamp), a camera beyond the band through the pre-list alone
  exact-only mode  every keypoint through the exact pass; guard band 1e-4: a mixed list
  sizes and modes  descSize 16 / 32 / 64, dBRIEF and mdBRIEF; ORB as control (its offsets never leave the patch, its output ignores c, d, e)
  MCS_LIST_SPLIT=0 the one-wave list kernel on the same cases, in a fresh process
  camera change    stretched, Lafida, stretched again in one extractor (per-camera G(s) tables, the captured graph of a small batch)
  rounding ties    band 0.5 px and exact-only, so every row that leaves is the host code's: whole-level download (> 64 listed), the capture slot (<= 64 listed:
                   windows of border keypoints), a sample outside the 81 x 81 window (host-kind: falls back to the levels; pipelined: MCS_ERR_UNSUPPORTED)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_cameras as HC
import hostile_inputs as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMS = list(HC.GEOMS)
BAND = 2.0 ** -24     # the default guard band; the fast pass serves a camera whose bound is at most half of it


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


def bound_of(G, cam, ds=32):
    oc, b = G.mcs.make_ocam(cam), C.c_double()
    G.mcs.check(G.mcs.lib().mcs_describe_fast_bound(C.byref(oc), ds, C.byref(b)))
    return b.value


def check_outputs(G, got, c, tag):
    r = HC.oracle_run(c)
    gk, gd, gm, gr = got
    tag = (tag, HC.tag_of(c))
    assert len(gk) == len(r["kps"]), (tag, "keypoints", len(gk), len(r["kps"]))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert G.first_diff(gk[f].view(np.uint32), r["kps"][f].view(np.uint32)) is None, (tag, f, G.first_diff(gk[f].view(np.uint32), r["kps"][f].view(np.uint32)))
    assert G.first_diff(gd, r["desc"]) is None, (tag, "descriptors", G.first_diff(gd, r["desc"]))
    assert G.first_diff(gm, r["dmask"]) is None, (tag, "descriptor masks", G.first_diff(gm, r["dmask"]))
    if gr is not None:
        assert G.first_diff(np.asarray(gr).view(np.uint64), r["rays"].view(np.uint64)) is None, (tag, "rays")


def extractor_for(G, cs, max_batch=None):
    w, h = HC.GEOMS[cs[0]["geom"]][:2]
    assert all(HC.key_of(c)[3] == HC.key_of(cs[0])[3] for c in cs)
    return G.mcs.Extractor(G.ctx(), w, h, max_batch=max_batch or len(cs), **cs[0]["params"])


def run_batch(G, ex, cs, tag=""):
    """ONE host-kind batch of the cases (their cameras side by side), every image against its oracle run; -> keypoints in all"""
    inp = [HC.oracle_run(c)["inputs"] for c in cs]
    masks = None if all(m is None for _, m, _ in inp) else [m if m is not None else H.mask("full", *im.shape) for im, m, _ in inp]
    res = ex.extract_host([im for im, _, _ in inp], masks, [G.mcs.make_ocam(cam) for _, _, cam in inp])
    ex.status()
    for i, c in enumerate(cs):
        check_outputs(G, res[i], c, "%s image %d" % (tag, i))
    return sum(len(r[0]) for r in res)


def must_take_the_exact_pass(c):
    """keypoints the fast pass cannot serve, by the numpy classification: a sample outside the staged patch or a pattern point outside the G(s) table"""
    cl = HC.classify_case(c)
    return int((cl["outside_patch"] | cl["s_above_table"] | cl["s_below_table"]).sum())


# ---- default mode --------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_default_mode_all_cameras_in_one_batch(G, geom):
    w, h = HC.GEOMS[geom][:2]
    cs = HC.cases(geom)
    bounds = {n: bound_of(G, HC.camera(n, w, h)) for n in HC.CAMERAS}
    outside = {n: sum(HC.counts(HC.classify_case(c))["outside_patch"] for c in cs if c["camera"] == n) for n in HC.CAMERAS}
    served = [n for n in HC.STRETCHED if bounds[n] <= 0.5 * BAND and outside[n] > 0]
    assert len(served) >= 2, (bounds, outside)
    # c = 3.2 stays inside the band (bound 2.5e-9 .. 5.1e-9 px at these sizes, the band's half is 3.0e-8): the fast pass serves s320 and corner320, and hands
    # nearly all of their keypoints on by the "outside the patch" verdict
    assert bounds["s320"] <= 0.5 * BAND and bounds["corner320"] <= 0.5 * BAND and bounds["band160"] > BAND
    ex = extractor_for(G, cs)
    nk = run_batch(G, ex, cs, "default")
    n_exact = ex.describe_stats()[0]
    expect = sum(len(HC.oracle_run(c)["kps"]) if c["camera"] == "band160" else must_take_the_exact_pass(c) for c in cs)
    assert nk > n_exact >= expect > 1000, (nk, n_exact, expect)
    ex.close()
    # camera by camera in one small extractor (without a mask, with the mirror mask): what the device reports per camera
    pair = [HC.case(geom, "lafida0", m) for m in HC.MASKS]
    ex = extractor_for(G, pair)
    for n in HC.CAMERAS:
        pair = [HC.case(geom, n, m) for m in HC.MASKS]
        before = ex.describe_stats()[0]
        nk = run_batch(G, ex, pair, "camera by camera")
        n_exact = ex.describe_stats()[0] - before
        regimes = {k: sum(HC.counts(HC.classify_case(c))[k] for c in pair) for k in HC.REGIMES}
        print("hostile camera %s %-10s bound %.3e px  keypoints %4d  exact pass %4d  %s" % (geom, n, bounds[n], nk, n_exact, regimes))
        assert n_exact >= sum(must_take_the_exact_pass(c) for c in pair), (n, n_exact)
        if n == "band160":
            assert n_exact == nk > 100, (n_exact, nk)     # beyond the band: listed before the fast pass runs, every keypoint through k_describe_list
        if n in HC.CONTROLS:
            assert n_exact < 0.1 * nk, (n, n_exact, nk)   # the exception on the cameras the suite knew
    ex.close()


# ---- exact-only mode, and a mixed list ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_exact_only_and_a_mixed_list(G, geom):
    cs = HC.cases(geom)
    ex = extractor_for(G, cs)
    ex.set_describe(exact_only=True)
    nk = run_batch(G, ex, cs, "exact only")
    ex.set_describe(exact_only=False, guard_eps=1e-4)     # (every camera's bound is below half of this band: band160 takes the fast pass here)
    before = ex.describe_stats()[0]
    assert run_batch(G, ex, cs, "guard band 1e-4") == nk
    n_exact = ex.describe_stats()[0] - before
    assert sum(must_take_the_exact_pass(c) for c in cs) < n_exact < nk, (n_exact, nk)
    ex.close()


# ---- descriptor sizes and modes ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,ds", [("dbrief", 16), ("dbrief", 32), ("dbrief", 64), ("mdbrief", 16), ("mdbrief", 64)])
@pytest.mark.parametrize("geom", GEOMS)
def test_descriptor_sizes_and_modes(G, geom, mode, ds):
    cs = HC.cases(geom, mode, ds, masks=(None,))
    ex = extractor_for(G, cs)
    assert run_batch(G, ex, cs, "%s %d" % (mode, ds)) > 3000
    assert ex.describe_stats()[0] >= sum(must_take_the_exact_pass(c) for c in cs) > 500
    ex.close()


@pytest.mark.parametrize("geom", GEOMS)
def test_orb_control_ignores_the_affine_terms(G, geom):
    cs = HC.cases(geom, "orb", 32, masks=(None,))
    ex = extractor_for(G, cs)
    inp = [HC.oracle_run(c)["inputs"] for c in cs]
    res = ex.extract_host([im for im, _, _ in inp], None, [G.mcs.make_ocam(cam) for _, _, cam in inp])
    ex.status()
    for i, c in enumerate(cs):
        check_outputs(G, res[i], c, "orb")
        assert G.first_diff(res[i][0], res[0][0]) is None and G.first_diff(res[i][1], res[0][1]) is None and not res[i][2].any(), c["camera"]
    names = [c["camera"] for c in cs]
    assert G.first_diff(res[names.index("s160")][3], res[names.index("lafida0")][3]) is not None    # ... except for the rays
    ex.close()


# ---- the one-wave list kernel --------------------------------------------------------------------------------------------------------------------------------------------
def test_one_wave_list_kernel_in_a_fresh_process():
    """MCS_LIST_SPLIT=0: the fallback list through k_describe_list (a wave per keypoint) instead of k_describe_list_split — the same cases, the same oracle"""
    e = dict(os.environ, MCS_LIST_SPLIT="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_hostile_cameras.py"), "-m", "gpu", "-q", "-x", "-k",
                        "default_mode_all_cameras or exact_only_and_a_mixed"], env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-1000:]
    assert "4 passed" in r.stdout, r.stdout[-500:]


# ---- camera change in one extractor --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_camera_change_between_calls(G, geom):
    stretched, lafida = HC.cases(geom, cams=HC.STRETCHED), HC.cases(geom, cams=HC.CONTROLS)
    ex = extractor_for(G, stretched)
    for i, cs in enumerate((stretched, lafida, stretched)):
        run_batch(G, ex, cs, "call %d" % i)
    ex.close()
    # a small batch (its launch sequence is captured once and replayed): the cameras change under the same graph
    ex = extractor_for(G, [HC.case(geom, "s320", m) for m in HC.MASKS])
    for i, n in enumerate(("s320", "lafida0", "s320", "corner320", "lafida1", "band160", "corner320")):
        run_batch(G, ex, [HC.case(geom, n, m) for m in HC.MASKS], "small call %d" % i)
    ex.close()


# ---- rounding ties: every row from the host code -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_ties_host_kind_whole_level_download(G, geom):
    """(a) more than 64 listed keypoints: the host recomputes from downloaded levels (fix_ties), frame and clamp included"""
    cs = HC.cases(geom, masks=(None,))
    ex = extractor_for(G, cs)
    ex.set_describe(exact_only=True)
    ex.set_tie_band(0.5)
    nk = run_batch(G, ex, cs, "band 0.5")
    listed, fixed, band = ex.tie_counts()
    assert band == 0.5 and listed == fixed == nk > 64, (listed, fixed, nk)
    ex.close()


@pytest.mark.parametrize("geom", GEOMS)
def test_ties_host_kind_capture_slot_and_window_miss(G, geom):
    """(b) at most 64 listed keypoints: recomputed from the 81 x 81 windows the device captured — next to a corner principal point the windows of border keypoints hold
    frame samples; (d) on the cameras that stretch the pattern beyond 40 px a sample misses its window: the call falls back to the levels (still resident in a
    host-kind call) and returns MCS_OK with the oracle's rows"""
    small = HC.small_cases(geom)
    ex = extractor_for(G, small[:1], max_batch=1)
    ex.set_describe(exact_only=True)
    ex.set_tie_band(0.5)
    frame_in_window = misses = 0
    for c in small:
        cl = HC.classify_case(c)
        before = ex.tie_counts()[:2]
        nk = run_batch(G, ex, [c], "capture slot")      # (raises on any error code: the window miss must not surface)
        listed, fixed, _ = ex.tie_counts()
        assert listed - before[0] == fixed - before[1] == nk and 0 < nk <= 64, (HC.tag_of(c), listed, fixed, nk)
        if cl["beyond_40"].any():
            misses += 1
        elif cl["in_frame"].any():
            frame_in_window += 1
    assert misses >= 2 and frame_in_window >= 1, (misses, frame_in_window)
    ex.close()


def _device_batch(G, ex, c):
    """ONE device-kind batch of one image -> its device buffers"""
    img, _, cam = HC.oracle_run(c)["inputs"]
    h, w = img.shape
    cap, ds = ex.cap, c["params"]["descSize"]
    b = dict(img=G.DevBuf(img), nkp=G.DevBuf(np.zeros(1, np.int32)), kps=G.DevBuf(np.zeros((1, cap), G.mcs.KP_DTYPE)), desc=G.DevBuf(np.zeros((1, cap, ds), np.uint8)),
             mask=G.DevBuf(np.zeros((1, cap, ds), np.uint8)), rays=G.DevBuf(np.zeros((1, cap, 3))))
    ex.extract_device(1, b["img"].ptr.value, w * h, w, 0, w * h, w, [G.mcs.make_ocam(cam)], b["nkp"].ptr.value, b["kps"].ptr.value, b["desc"].ptr.value,
                      b["mask"].ptr.value, b["rays"].ptr.value)
    G.ctx().synchronize()
    return b


def _device_rows(b):
    n = int(b["nkp"].read()[0])
    return b["kps"].read()[0, :n], b["desc"].read()[0, :n], b["mask"].read()[0, :n], b["rays"].read()[0, :n]


@pytest.mark.parametrize("geom", GEOMS)
def test_ties_pipelined_capture_and_window_miss(G, geom):
    """(c) device-kind batches patched from the capture ring (mcs_extractor_patch_ties): the rows are scribbled over first, so every row that is right afterwards is
    the host code's; (d) a sample outside the window cannot be refetched — the pyramid may hold a later batch —, so patch_ties reports MCS_ERR_UNSUPPORTED, patches
    nothing, and the extractor goes on: mcs_extractor_fix_ties still serves that batch while it is the latest, and a following Lafida batch is patched as usual"""
    cap_ = G.mcs._capi
    small = HC.small_cases(geom)
    ex = extractor_for(G, small[:1], max_batch=1)
    ex.set_describe(exact_only=True)
    ex.set_tie_band(0.5)
    ex.set_tie_capture(2, 128)
    patched = refused = 0
    for c in small + [HC.case(geom, "lafida0", None, nfeatures=HC.SMALL_NFEATURES)]:
        cl = HC.classify_case(c)
        b = _device_batch(G, ex, c)
        ex.status()
        nk = int(b["nkp"].read()[0])
        assert 0 < nk == len(HC.oracle_run(c)["kps"]) <= 128
        nbytes = b["desc"].arr.nbytes
        assert G.hip().hipMemset(b["desc"].ptr, 0xA5, nbytes) == 0 and G.hip().hipMemset(b["mask"].ptr, 0x5A, nbytes) == 0
        a, r = C.c_int(), C.c_int()
        rc = G.mcs.lib().mcs_extractor_patch_ties(ex.h, 0, a, r)
        if cl["beyond_40"].any():
            assert rc == cap_.MCS_ERR_UNSUPPORTED and a.value == nk and r.value == 0, (HC.tag_of(c), rc, a.value, r.value)
            assert (b["desc"].read() == 0xA5).all() and (b["mask"].read() == 0x5A).all()     # nothing patched
            assert ex.fix_ties() == nk                                                     # the synchronous form still serves the batch
            refused += 1
        else:
            assert rc == cap_.MCS_OK and a.value == r.value == nk, (HC.tag_of(c), rc, a.value, r.value, nk)
            assert ex.patch_ties(0) == (nk, 0)
            patched += 1
        check_outputs(G, _device_rows(b), c, "pipelined")
    assert refused >= 2 and patched >= 3 and c["camera"] == "lafida0", (refused, patched)    # (the Lafida batch came after the refusals)
    ex.close()
