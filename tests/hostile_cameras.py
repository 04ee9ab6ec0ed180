"""Hostile camera models for the descriptor stage (csrc/mcs_describe.hip, mcs_tiecap.h, mcs_tiefix.hip): the table of cameras and cases that
tests/test_oracle_hostile_cameras_cpu.py (oracle == the definition / the reference's own code, and the floors that keep a case from passing vacuously) and
tests/test_gpu_hostile_cameras.py (device == oracle, bit for bit) both walk.  Plain module: numpy and the CPU oracle only, nothing of the device.

The Lafida calibrations have affine terms c ~ 1, d ~ e ~ 0 and the principal point at the image centre: the distorted pattern never moves a sample more than 20 px
from its keypoint, so every sample is read from the 43 x 43 patch the kernels stage around it.  The camera model accepts any c, d, e, u0, v0; the cameras below
stretch and shear the pattern and push the principal point into an image corner, so that samples land
  outside the patch but inside the level (the blurred level, read from global memory),
  in the 25-px frame (the reflect-101 continuation of the UNBLURRED level),
  beyond the frame (clamped to the framed buffer: deviation (2) of DESIGN.md section 2; the reference reads outside its buffer there),
  more than 40 px from the keypoint (outside the 81 x 81 window of the rounding-tie capture),
and, without a mirror mask, keypoints near 90 degrees of incidence put pattern points outside the fast pass's G(s) table (s = x^2 + y^2 >= 2^24).

describe_by_definition states what a descriptor IS in vectorised numpy float64 — one array expression over all keypoints and pattern points,
none of the oracle's loops or helpers; classify reports which of the regimes above each keypoint reaches."""
import ctypes as C
import importlib

import numpy as np

import hostile_inputs as H
import oracle_lib as O

synth = importlib.import_module("multicol-slam_amd.synth")

PATCH_R = 21          # the kernels' staged patch: rows / columns -21 .. +21 around the keypoint
FRAME = 25            # EDGE_THRESHOLD: the border of a level's buffer
WINDOW_R = 40         # the rounding-tie capture: rows / columns -40 .. +40
TIE_EXCLUSION = 1e-9  # px: numpy's cos / sin / arctan need not equal glibc's in the last place; that moves a coordinate by ~1e-13 px at most
S_TABLE = (2.0 ** -10, 2.0 ** 24)   # the fast pass's G(s) table covers s in [2^-10, 2^24)

# (width, height, pyramid, nfeatures).  g400: levels 400 / 333 / 278 / 231 px wide — none a multiple of the device's row alignment, so the rows are padded
GEOMS = {"g160": (160, 120, dict(nlevels=3, scaleFactor=1.2), 500),
         "g400": (400, 300, dict(nlevels=4, scaleFactor=1.2), 500)}
MODES = {"dbrief": dict(do_dBrief=1, learnMasks=0), "mdbrief": dict(do_dBrief=1, learnMasks=1), "orb": dict(do_dBrief=0, learnMasks=0)}
DESC_SIZES = (16, 32, 64)
MASKS = (None, "mirror")
SMALL_NFEATURES = 40  # the "few keypoints" cases: at most 64 keypoints in all, so a host-kind call recomputes its listed keypoints from the capture slot


def _affine(c, d, e, u0=None, v0=None):
    def make(cam, w, h):
        out = dict(cam, c=c, d=d, e=e)
        if u0 is not None:
            out["u0"], out["v0"] = (u0(w), v0(h))
        return out
    return make


def _flipped(cam, w, h):
    """the mirror camera: p0 > 0, invP(-theta) — the other sign of p0"""
    out = dict(cam)
    out["p"] = [-v for v in cam["p"]]
    out["invP"] = [v * (-1) ** i for i, v in enumerate(cam["invP"])]
    return out


def _short(cam, w, h):
    """a degree-6 backward polynomial"""
    return dict(cam, invP=list(cam["invP"])[:6])


def _beyond_band(cam, w, h):
    """a backward polynomial with a pair of alternating coefficients on top (the construction of test_camera_beyond_the_band_runs_exact_only, stretched like s160):
    the fast pass's error bound grows with them by 2.65e-7 px per unit, so at 1.0 it is 4.4 times the default guard band (2^-24 px) and every keypoint is listed for
    the exact pass before the fast pass runs.  (That test adds 4e8: rho then reaches 7e10 px and the pattern coordinates leave the range of an int, where cvRound
    has no defined value — nothing to compare.  At 1.0 rho gains up to 180 px: samples in every regime.)"""
    out = _affine(1.6, 0.2, -0.15)(cam, w, h)
    inv = list(out["invP"])
    inv[10] += 1.0
    inv[11] -= 1.0 / (np.pi / 2) * 0.999
    out["invP"] = inv
    return out


# name -> (index of the Lafida calibration it starts from, what is done to it after scaling to the test size)
CAMERAS = {
    "lafida0": (0, None), "lafida1": (1, None), "lafida2": (2, None),                      # the controls
    "s115": (0, _affine(1.15, 0.0, 0.0)),
    "shear": (0, _affine(1.0, 0.5, -0.4)),
    "s160": (0, _affine(1.6, 0.2, -0.15)),
    "corner160": (0, _affine(1.6, 0.0, 0.8, lambda w: 28.0, lambda h: 27.0)),
    "corner_br": (0, _affine(2.0, -0.5, 1.0, lambda w: w - 27.5, lambda h: h - 26.5)),
    "s320": (0, _affine(3.2, 0.0, 0.0)),
    "corner320": (0, _affine(3.2, 0.0, 1.5, lambda w: 28.0, lambda h: 27.0)),
    "shrink": (0, _affine(0.5, 0.0, 0.0)),
    "flipped": (0, _flipped),
    "short": (2, _short),
    "band160": (0, _beyond_band),
}
CONTROLS = ("lafida0", "lafida1", "lafida2")
STRETCHED = tuple(n for n in CAMERAS if n not in CONTROLS)


def camera(name, w, h):
    base, change = CAMERAS[name]
    cam = synth.scaled_camera(synth.lafida_cameras()[base], w, h)
    return change(cam, w, h) if change else cam


def mirror_mask(cam):
    return O.mirror_mask(O.make_ocam(cam))


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------------------------------
def case(geom, cam, mask=None, mode="mdbrief", descSize=32, nfeatures=None):
    w, h, pyr, nf = GEOMS[geom]
    return dict(geom=geom, camera=cam, mask=mask, mode=mode, params=dict(H.BASE, **pyr, **H.DETECTORS["fast9_16"], **MODES[mode], descSize=descSize,
                                                                         nfeatures=nfeatures or nf))


def cases(geom, mode="mdbrief", descSize=32, cams=None, masks=MASKS, nfeatures=None):
    """every camera of the table, without a mask and with the camera's mirror mask"""
    return [case(geom, c, m, mode, descSize, nfeatures) for c in (cams or CAMERAS) for m in masks]


def small_cases(geom, mode="mdbrief", descSize=32):
    """few keypoints (<= 64) on the cameras that send samples beyond 40 px, and into frame and clamp next to a border keypoint"""
    return [case(geom, c, None, mode, descSize, SMALL_NFEATURES) for c in ("s320", "corner320", "corner160", "corner_br")]


def key_of(c):
    return (c["geom"], c["camera"], c["mask"], tuple(sorted(c["params"].items())))


def tag_of(c):
    return "%s/%s/%s %s%d n=%d" % (c["geom"], c["camera"], c["mask"], c["mode"], c["params"]["descSize"], c["params"]["nfeatures"])


def inputs(c):
    """-> image, mask (or None), camera of a case"""
    w, h = GEOMS[c["geom"]][:2]
    cam = camera(c["camera"], w, h)
    return H.image("noise", h, w), (mirror_mask(cam) if c["mask"] == "mirror" else None), cam


_RUNS = {}


def oracle_run(c, keep=True):
    """the oracle's run of a case, computed once and left unchanged: dict(inputs, oex, kps, desc, dmask, rays, keys, levels)"""
    k = key_of(c)
    if not keep and k not in _RUNS:
        saved = dict(_RUNS)
        try:
            return oracle_run(c)
        finally:
            _RUNS.clear()
            _RUNS.update(saved)
    if k not in _RUNS:
        img, msk, cam = inputs(c)
        oex, kps, d, dm = H.run_oracle(img, msk, cam, **c["params"])
        rays = np.zeros((len(kps), 3))
        if len(kps):
            O.lib().orc_rays(O.make_ocam(cam), O.ptr(kps), len(kps), O.ptr(rays))
        nl = c["params"]["nlevels"]
        _RUNS[k] = dict(inputs=(img, msk, cam), oex=oex, kps=kps, desc=d, dmask=dm, rays=rays, keys=keys_of(oex, kps, nl), levels=level_images(oex, nl))
    return _RUNS[k]


def keys_of(oex, kps, nlevels):
    """what a descriptor is computed from, per keypoint in output order: level, integer position in the level (row, col), image coordinates (u, v), angle (degrees)"""
    sel = [oex.selected(l) for l in range(nlevels)]
    lev = np.concatenate([np.full(len(s), l, np.int64) for l, s in enumerate(sel)]) if sel else np.zeros(0, np.int64)
    sel = np.concatenate(sel)
    assert len(sel) == len(kps) and np.array_equal(lev, kps["octave"]) and np.array_equal(sel["angle"].view(np.uint32), kps["angle"].view(np.uint32))
    row, col = np.rint(sel["y"]).astype(np.int64), np.rint(sel["x"]).astype(np.int64)
    assert np.array_equal(row, sel["y"]) and np.array_equal(col, sel["x"])      # (level positions are whole pixels)
    return dict(level=lev, row=row, col=col, u=kps["x"].astype(np.float64), v=kps["y"].astype(np.float64), angle=kps["angle"].astype(np.float32))


def level_images(oex, nlevels):
    """[(unblurred, blurred)] per level from the oracle's taps (a level without keypoints is never blurred, and never sampled)"""
    return [(oex.level_image(l), oex.level_image(l, blurred=True)) for l in range(nlevels)]


def pattern(descSize):
    xy = np.zeros(2 * 16 * descSize, np.int32)
    assert O.lib().orc_pattern(descSize, O.ptr(xy)) == 16 * descSize
    return xy.astype(np.float64).reshape(-1, 2)


# ---- the definition ----------------------------------------------------------------------------------------------------------------------------------------------------
def _poly(coeffs, x):
    r = np.zeros_like(x)
    for c in reversed(list(coeffs)):
        r = r * x + c
    return r


def pattern_angles(angle_deg, mode):
    """[patterns][keypoints] radians: the keypoint's orientation, and for mdBRIEF the same +- 20 degrees (float32 degrees -> radians as the reference converts them)"""
    a = np.asarray(angle_deg, np.float32)
    if mode == "dbrief":
        return [(a * (np.float32(np.pi) / np.float32(180.0))).astype(np.float64)]
    a = (a / (np.float32(180.0) / np.float32(np.pi))).astype(np.float64)
    rot = 20.0 / (180.0 / np.pi)
    return [a, a + rot, a - rot]


def distorted_patterns(keys, cam, descSize, mode):
    """-> (coords [patterns][keypoints, points, 2]: pattern coordinates minus their mean, BEFORE rounding; s [patterns][keypoints, points] = x^2 + y^2 of the points
    handed to WorldToImg)"""
    c, d, e, u0, v0, p, inv = cam["c"], cam["d"], cam["e"], cam["u0"], cam["v0"], cam["p"], cam["invP"]
    # ImgToWorld of the keypoint, then (-x / z, -y / z) * p0: the keypoint on the plane z = -p0
    ut, vt = keys["u"] - u0, keys["v"] - v0
    det = c - d * e
    x, y = (ut - d * vt) / det, (-e * ut + c * vt) / det
    z = -_poly(p, np.sqrt(x * x + y * y))
    n = np.sqrt(x * x + y * y + z * z)
    x, y, z = x / n, y / n, z / n
    kx, ky = (-x / z * p[0])[:, None], (-y / z * p[0])[:, None]
    pat = pattern(descSize)
    px, py = pat[None, :, 0], pat[None, :, 1]
    coords, ss = [], []
    for ang in pattern_angles(keys["angle"], mode):
        ca, sa = np.cos(ang)[:, None], np.sin(ang)[:, None]
        xr, yr = px * ca - py * sa + kx, px * sa + py * ca + ky
        # WorldToImg(xr, yr, -p0)
        nrm = np.sqrt(xr * xr + yr * yr)
        nrm = np.where(nrm == 0.0, 1e-14, nrm)
        rho = _poly(inv, np.arctan(p[0] / nrm))
        uu, vv = xr / nrm * rho, yr / nrm * rho
        iu, iv = uu * c + vv * d + u0, uu * e + vv + v0
        npts = float(pat.shape[0])
        # the mean is the SEQUENTIAL sum in point order (np.sum adds pairwise)
        mu, mv = np.cumsum(iu, axis=1)[:, -1:] / npts, np.cumsum(iv, axis=1)[:, -1:] / npts
        coords.append(np.stack([iu - mu, iv - mv], axis=2))
        ss.append(xr * xr + yr * yr)
    return coords, ss


def framed(raw, blurred):
    """a level as the descriptors see it: blurred inside, around it 25 px of the reflect-101 continuation of the UNBLURRED level"""
    buf = np.pad(raw, FRAME, mode="reflect")
    buf[FRAME:-FRAME, FRAME:-FRAME] = blurred
    return buf


def describe_by_definition(levels, keys, cam, descSize, mode):
    """levels: [(unblurred, blurred)] per level; keys: keys_of(); mode "dbrief" / "mdbrief".
    -> (descriptors, masks, left_out): left_out[k] = some coordinate of keypoint k lies within TIE_EXCLUSION of k + 1/2 (not comparable through another libm)"""
    nk = len(keys["level"])
    coords, _ = distorted_patterns(keys, cam, descSize, mode)
    left_out = np.zeros(nk, bool)
    bufs = {int(l): framed(*levels[int(l)]) for l in np.unique(keys["level"])}
    bits = []
    for xy in coords:
        assert np.isfinite(xy).all() and np.abs(xy).max(initial=0) < 2.0 ** 30
        left_out |= (np.abs(np.abs(xy - np.floor(xy)) - 0.5) < TIE_EXCLUSION).any(axis=(1, 2))
        off = np.rint(xy).astype(np.int64)                                   # cvRound: half to even
        val = np.zeros(off.shape[:2], np.uint8)
        for l, buf in bufs.items():
            sel = keys["level"] == l
            r = np.clip(keys["row"][sel, None] + off[sel, :, 1] + FRAME, 0, buf.shape[0] - 1)   # beyond the frame: clamped to the framed buffer
            c_ = np.clip(keys["col"][sel, None] + off[sel, :, 0] + FRAME, 0, buf.shape[1] - 1)
            val[sel] = buf[r, c_]
        bits.append(np.packbits(val[:, 0::2] < val[:, 1::2], axis=1, bitorder="little"))
    desc = bits[0].reshape(nk, descSize)
    if mode == "mdbrief":
        dmask = (~((bits[0] ^ bits[1]) | (bits[0] ^ bits[2]))).astype(np.uint8).reshape(nk, descSize)
    else:
        dmask = np.zeros_like(desc)
    return desc, dmask, left_out


REGIMES = ("outside_patch", "in_level_outside_patch", "in_frame", "beyond_frame", "beyond_40", "s_above_table", "s_below_table", "non_finite")


def classify(level_sizes, keys, cam, descSize, mode):
    """per keypoint, over all patterns of the mode: bool arrays by REGIMES.  level_sizes: [(w, h)] per level"""
    coords, ss = distorted_patterns(keys, cam, descSize, mode)
    nk = len(keys["level"])
    out = {r: np.zeros(nk, bool) for r in REGIMES}
    lw = np.array([s[0] for s in level_sizes], np.int64)[keys["level"]][:, None]
    lh = np.array([s[1] for s in level_sizes], np.int64)[keys["level"]][:, None]
    for xy, s in zip(coords, ss):
        fin = np.isfinite(xy).all(axis=2)
        out["non_finite"] |= ~fin.all(axis=1) | ~np.isfinite(s).all(axis=1)
        off = np.rint(np.where(np.isfinite(xy), xy, 0.0)).astype(np.int64)
        far = np.abs(off).max(axis=2)
        r, c_ = keys["row"][:, None] + off[:, :, 1], keys["col"][:, None] + off[:, :, 0]
        in_level = (r >= 0) & (r < lh) & (c_ >= 0) & (c_ < lw)
        in_buffer = (r >= -FRAME) & (r < lh + FRAME) & (c_ >= -FRAME) & (c_ < lw + FRAME)
        out["outside_patch"] |= (far > PATCH_R).any(axis=1)
        out["in_level_outside_patch"] |= ((far > PATCH_R) & in_level).any(axis=1)
        out["in_frame"] |= (in_buffer & ~in_level).any(axis=1)
        out["beyond_frame"] |= (~in_buffer).any(axis=1)
        out["beyond_40"] |= (far > WINDOW_R).any(axis=1)
        out["s_above_table"] |= (s >= S_TABLE[1]).any(axis=1)
        out["s_below_table"] |= (s < S_TABLE[0]).any(axis=1)
    return out


_CLASSES = {}


def classify_case(c):
    """classify() of a case's oracle run, computed once (ORB has no distorted pattern: nothing to classify)"""
    k = key_of(c)
    if k not in _CLASSES:
        r = oracle_run(c)
        nl = c["params"]["nlevels"]
        _CLASSES[k] = classify([r["oex"].level_size(l) for l in range(nl)], r["keys"], r["inputs"][2], c["params"]["descSize"], c["mode"])
    return _CLASSES[k]


def counts(cl):
    return {k: int(v.sum()) for k, v in cl.items()}
