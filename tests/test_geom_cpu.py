"""CPU: csrc/mcs_geom.h, the one statement of the rig geometry the map-side kernels share, compiled for the host alone (tests/cpp/geom_driver.cpp, no HIP call)
and held BIT FOR BIT to the reference's compiled code (oracle/_ref: ref_cayley2hom, ref_world_to_cam): cayley2hom, inv_mat(matx44_mul(M_t, M_c[c])) against the
MtMc_inv the reference's cMultiCamSys_ forms, world_to_cam_hom_fast + in_mirror_mask against WorldToCamHom_fast + isPointInMirrorMask.  The host's atan is on both
sides, so equality is exact.  dot3 / norm3 / mat3_vec3 are held to plain left-to-right Python float arithmetic (no fused multiply-add, IEEE doubles)."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_io_formats import CAYLEY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
have_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")
synth = importlib.import_module("multicol-slam_amd.synth")
NVEC = 300


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """the library's floating-point flags (csrc/Makefile), host only"""
    exe = tmp_path_factory.mktemp("geom") / "geom_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-I" + CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "geom_driver.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def vectors():
    rng = np.random.default_rng(11)
    a, b = rng.normal(0, 3.0, (NVEC, 3)), rng.normal(0, 3.0, (NVEC, 3))
    a[0], b[0] = [1e308, 1e308, -1e308], [1.0, 1.0, 1.0]        # the order of the additions decides: (1e308 + 1e308) - 1e308 = inf, not 1e308
    a[1], b[1] = [1.0, 1e-17, -1.0], [1.0, 1.0, 1.0]            # (1 + 1e-17) - 1 = 0, not 1e-17
    a[2] = [np.nan, 1.0, 2.0]
    return a, b, rng.normal(0, 1.0, (NVEC, 9)), rng.normal(0, 1.0, (NVEC, 16))


def run(driver, tmp_path, pose, mc_min, cams, masks, pts, pcam, vec):
    nr, n = len(cams), len(pts)
    a, b, M3, M4 = vec
    oc = (O.Ocam * nr)(*[O.make_ocam(c) for c in cams])
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([nr, n, len(a), C.sizeof(O.Ocam), 1 if masks else 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(pose, np.float64).tobytes() + np.ascontiguousarray(mc_min, np.float64).tobytes() + bytes(oc))
        for m in masks or []:
            f.write(np.ascontiguousarray(m, np.uint8).tobytes())
        f.write(np.ascontiguousarray(pts, np.float64).tobytes() + np.ascontiguousarray(pcam, np.int32).tobytes())
        for v in (a, b, M3, M4):
            f.write(np.ascontiguousarray(v, np.float64).tobytes())
    subprocess.check_call([str(driver), str(src), str(dst)])
    raw, at, out = open(dst, "rb").read(), 0, {}
    for name, shape, dt in (("Mt", (4, 4), np.float64), ("Mc", (nr, 4, 4), np.float64), ("inv", (nr, 4, 4), np.float64), ("uv", (n, 2), np.float64),
                            ("flags", (n,), np.uint8), ("dot", (len(a),), np.float64), ("norm", (len(a),), np.float64), ("mv3", (len(a), 3), np.float64),
                            ("mv4", (len(a), 3), np.float64)):
        size = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = np.frombuffer(raw[at:at + size], dt).reshape(shape)
        at += size
    assert at == len(raw)
    return out


def reference(pose, mc_min, cams, masks, pts, pcam):
    ref = C.CDLL(REF_SO)
    ref.ref_cayley2hom.argtypes = [C.c_void_p, C.c_void_p]
    ref.ref_world_to_cam.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(O.Ocam), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]

    def hom(c6):
        c6, M = np.ascontiguousarray(c6, np.float64), np.zeros((4, 4))
        ref.ref_cayley2hom(c6.ctypes.data, M.ctypes.data)
        return M
    nr, n = len(cams), len(pts)
    Mt, Mc = hom(pose), np.stack([hom(m) for m in mc_min])
    uv, fl, inv = np.zeros((n, 2)), np.zeros(n, np.uint8), np.zeros((nr, 4, 4))
    oc = (O.Ocam * nr)(*[O.make_ocam(c) for c in cams])
    mp = (C.c_void_p * nr)(*[m.ctypes.data for m in masks]) if masks else None
    pts, pcam = np.ascontiguousarray(pts, np.float64), np.ascontiguousarray(pcam, np.int32)
    assert ref.ref_world_to_cam(Mt.ctypes.data, Mc.ctypes.data, oc, mp, nr, pts.ctypes.data, pcam.ctypes.data, n, uv.ctypes.data, fl.ctypes.data, inv.ctypes.data) == 0
    return dict(Mt=Mt, Mc=Mc, inv=inv, uv=uv, flags=fl)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, ref):
    """bit for bit; a NaN equals a NaN (the sign and payload of a NaN are the compiler's choice of operand order, in the reference's build as in ours)"""
    for k in ("Mt", "Mc", "inv", "uv"):
        nan = np.isnan(ref[k])
        assert np.array_equal(np.isnan(got[k]), nan), k
        assert np.array_equal(bits(got[k])[~nan], bits(ref[k])[~nan]), k
    assert np.array_equal(got["flags"], ref["flags"])


def point_for_pixel(cam, u, v):
    """a camera-frame point that WorldToImg sends close to (u, v): the affine part inverted, rho(theta) = |(uu, vv)| by bisection (rho is monotonic for these cameras)"""
    A = np.array([[cam["c"], cam["d"]], [cam["e"], 1.0]])
    uu, vv = np.linalg.solve(A, [u - cam["u0"], v - cam["v0"]])
    want, lo, hi = math.hypot(uu, vv), -1.55, 1.55
    rho = lambda t: float(np.polyval(cam["invP"][::-1], t))
    assert rho(lo) < want < rho(hi)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if rho(mid) < want else (lo, mid)
    return [uu / want, vv / want, -math.tan(lo)]


@have_ref
def test_lafida_rig_equals_the_reference_code(driver, tmp_path, vectors):
    """the three cameras of calib/lafida.json on their rig (the Cayley parameters of the LaFiDa calibration), at three poses, with their mirror masks"""
    cams = synth.lafida_cameras()
    masks = [np.ascontiguousarray(synth.mirror_mask(c)) for c in cams]
    rng = np.random.default_rng(5)
    seen = np.zeros(4, int)
    for pose in (np.zeros(6), np.array([0.02, -0.3, 0.11, 0.4, -0.2, 0.1]), rng.normal(0, 1.0, 6)):
        pts, pcam = rng.normal(0, 3.0, (400, 3)), rng.integers(0, 3, 400).astype(np.int32)
        ref = reference(pose, CAYLEY, cams, masks, pts, pcam)
        same(run(driver, tmp_path, pose, CAYLEY, cams, masks, pts, pcam, vectors), ref)
        seen += np.bincount(ref["flags"], minlength=4)[:4]
    # among the seeded points: out of the mask, in it, behind the camera (a point behind the camera falls outside these mirrors: the branches test has one in bounds)
    assert (seen[:3] > 20).all(), seen


@have_ref
def test_branches_equal_the_reference_code(driver, tmp_path, vectors):
    """the cases the statements branch on, written out by hand on a rig of identities (zero Cayley parameters: the camera-frame point IS the world point).
    Each is asserted to occur from the REFERENCE's outputs, so none is vacuous."""
    cams = synth.lafida_cameras()
    masks = [np.ascontiguousarray(synth.mirror_mask(c)) for c in cams]
    cam, W, H = cams[0], cams[0]["width"], cams[0]["height"]
    mid_u, mid_v = 380.0, 240.0
    named = {
        "axis": [0.0, 0.0, 2.0], "axis_behind": [0.0, 0.0, -2.0],                                           # x = y = 0: norm -> 1e-14
        "z+0": [1.0, 1.0, 0.0], "z-0": [1.0, 1.0, -0.0], "z+tiny": [1.0, 1.0, 5e-324], "z-tiny": [1.0, 1.0, -5e-324],   # ptRot.z <= 0
        "u->0": point_for_pixel(cam, 0.4, mid_v), "u->1": point_for_pixel(cam, 0.6, mid_v),                  # cvRound and the open bounds
        "u->W-1": point_for_pixel(cam, W - 1.4, mid_v), "u->W": point_for_pixel(cam, W - 0.4, mid_v),
        "v->0": point_for_pixel(cam, mid_u, 0.4), "v->1": point_for_pixel(cam, mid_u, 0.6),
        "v->H-1": point_for_pixel(cam, mid_u, H - 1.4), "v->H": point_for_pixel(cam, mid_u, H - 0.4),
        "masked": point_for_pixel(cam, 60.0, mid_v), "unmasked": point_for_pixel(cam, 300.0, mid_v),
        "nan": [np.nan, 1.0, 1.0], "nan_z": [1.0, 1.0, np.nan], "inf": [np.inf, 1.0, 1.0],
    }
    names = list(named)
    pts, pcam = np.array([named[k] for k in names]), np.zeros(len(names), np.int32)
    zero = np.zeros(6)
    out = {}
    for label, m in (("masks", masks), ("bounds", None)):
        ref = reference(zero, [zero] * 3, cams, m, pts, pcam)
        same(run(driver, tmp_path, zero, [zero] * 3, cams, m, pts, pcam, vectors), ref)
        out[label] = ref
    assert np.array_equal(out["masks"]["inv"], np.stack([np.eye(4)] * 3))
    uv, fl = out["bounds"]["uv"], dict(zip(names, out["bounds"]["flags"]))
    at = lambda k: uv[names.index(k)]
    assert tuple(at("axis")) == (cam["u0"], cam["v0"]) == tuple(at("axis_behind")) and fl["axis"] == 1 and fl["axis_behind"] == 3
    assert fl["z+0"] & 2 and fl["z-0"] & 2 and fl["z-tiny"] & 2 and not fl["z+tiny"] & 2
    for k, col, r, inside in (("u->0", 0, 0, 0), ("u->1", 0, 1, 1), ("u->W-1", 0, W - 1, 1), ("u->W", 0, W, 0),
                              ("v->0", 1, 0, 0), ("v->1", 1, 1, 1), ("v->H-1", 1, H - 1, 1), ("v->H", 1, H, 0)):
        assert np.rint(at(k)[col]) == r and (fl[k] & 1) == inside, (k, at(k), fl[k])
    flm = dict(zip(names, out["masks"]["flags"]))
    assert flm["masked"] & 1 == 0 and fl["masked"] & 1 == 1 and flm["unmasked"] & 1 == 1   # in bounds, and the mask decides
    assert masks[0][int(np.rint(at("masked")[1])), int(np.rint(at("masked")[0]))] == 0
    assert np.isnan(at("nan")).all() and np.isnan(at("nan_z")).all() and fl["nan"] & 1 == 0 and fl["nan_z"] == 0


def test_vec3_arithmetic_is_left_to_right(driver, tmp_path, vectors):
    """dot3 / norm3 / mat3_vec3 against "s = 0; s += a * b" in increasing k, in Python floats"""
    a, b, M3, M4 = vectors
    cams = synth.lafida_cameras()[:1]
    got = run(driver, tmp_path, np.zeros(6), [np.zeros(6)], cams, None, np.zeros((1, 3)) + 1.0, np.zeros(1, np.int32), vectors)

    def dot(x, y):
        s = 0.0
        for k in range(3):
            s += float(x[k]) * float(y[k])
        return s
    exp_dot = np.array([dot(a[i], b[i]) for i in range(NVEC)])
    exp_norm = np.array([math.sqrt(dot(a[i], a[i])) if not math.isnan(dot(a[i], a[i])) else math.nan for i in range(NVEC)])
    exp_mv3 = np.array([[dot(M3[i, 3 * r:3 * r + 3], a[i]) for r in range(3)] for i in range(NVEC)])
    exp_mv4 = np.array([[dot(M4[i, 4 * r:4 * r + 3], a[i]) for r in range(3)] for i in range(NVEC)])
    for g, e in ((got["dot"], exp_dot), (got["norm"], exp_norm), (got["mv3"], exp_mv3), (got["mv4"], exp_mv4)):
        nan = np.isnan(e)
        assert np.array_equal(np.isnan(g), nan) and np.array_equal(bits(g)[~nan], bits(e)[~nan])
    assert np.isinf(exp_dot[0]) and exp_dot[1] == 0.0 and np.isnan(exp_dot[2]) and np.isinf(exp_norm[0])   # the order-sensitive cases are what they claim
