"""CPU: csrc/mcs_sim3g.h, the one statement of g2o::Sim3's arithmetic the Sim3 optimisation stands on, compiled for the host alone (tests/cpp/sim3g_driver.cpp,
no HIP call) with the library's floating-point flags and held BIT FOR BIT to tests/sim3opt_model.py.  Both sides call the host's libm (sin, cos, exp, sqrt), so
equality is exact: every function, a few thousand random inputs, and the edges: theta and |sigma| on either side of 1e-5 (all four branches of the
exponential map), the 1e-9 steps of the numeric Jacobian, traces on either side of 0 and each of the three cases behind a non-positive trace."""
import os
import subprocess

import numpy as np
import pytest

import sim3opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
N = 1500


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sim3g") / "sim3g_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-I" + CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "sim3g_driver.cpp"), "-o", str(exe)])
    return exe


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def inputs():
    rng = np.random.default_rng(5)
    u = rng.normal(0, 0.3, (N, 7))
    k = 0
    for th in (0.0, 1e-9, 9.9e-6, 0.99999e-5, 1e-5, 1.00001e-5, 1.1e-5, 1e-3, 3.0):          # theta across its threshold ...
        for sg in (0.0, 1e-9, -1e-9, 9.9e-6, -9.9e-6, 1e-5, -1e-5, 1.00001e-5, 1.1e-5, -1.1e-5, 0.2, -0.7):   # ... times sigma across its own
            d = rng.normal(0, 1, 3)
            u[k, :3] = d / np.linalg.norm(d) * th
            u[k, 6] = sg
            k += 1
    for d in range(7):                                    # the steps of the numeric Jacobian
        for s in (1e-9, -1e-9):
            u[k] = 0.0
            u[k, d] = s
            k += 1
    rts = np.zeros((N, 13))
    for i in range(N):
        ang = rng.uniform(0, np.pi) if i % 3 else np.pi - rng.uniform(0, 0.3)     # every third one near a half turn: trace <= 0
        R = rot(rng.normal(0, 1, 3), ang)
        if i % 7 == 0:
            R = R + rng.normal(0, 1e-3, (3, 3))           # not a rotation: the conversion does not care
        rts[i, :9], rts[i, 9:12], rts[i, 12] = R.reshape(9), rng.normal(0, 2, 3), np.exp(rng.normal(0, 0.3))
    for j, ax in enumerate(([1, 0, 0], [0, 1, 0], [0, 0, 1])):                    # exactly a half turn about each axis: trace = -1, case i = j
        rts[j, :9] = rot(ax, np.pi).reshape(9)
    rts[3, :9] = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64).reshape(9)   # trace exactly 0: the else branch
    S = rng.normal(0, 1, (N, 8))
    S[:, 7] = np.exp(rng.normal(0, 0.4, N))
    S[: N // 2, :4] /= np.linalg.norm(S[: N // 2, :4], axis=1)[:, None]           # half of them unit quaternions, half not
    ab = np.concatenate([S, np.roll(S, 7, 0)], 1)
    sx = np.concatenate([S, rng.normal(0, 3, (N, 3))], 1)
    return u, rts, ab, S.copy(), sx, S[:, :4].copy()


def run(driver, tmp_path, parts):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([len(p) for p in parts], np.int32).tobytes())
        for p in parts:
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    subprocess.check_call([str(driver), str(src), str(dst)])
    raw = np.fromfile(dst, np.float64)
    out, at = [], 0
    for n, wdt in ((len(parts[0]), 9), (len(parts[1]), 8), (len(parts[2]), 8), (len(parts[3]), 8), (len(parts[4]), 3), (len(parts[4]), 3), (len(parts[5]), 9),
                   (len(parts[5]), 4)):
        out.append(raw[at:at + n * wdt].reshape(n, wdt))
        at += n * wdt
    assert at == len(raw)
    return out


def tup(v):
    return ([float(c) for c in v[:4]], [float(c) for c in v[4:7]], float(v[7]))


def same(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def test_header_equals_the_model_bit_for_bit(driver, tmp_path):
    u, rts, ab, S, sx, q = parts = inputs()
    ex, fr, mu, inv, mp, ro, mat, cj = run(driver, tmp_path, parts)
    branches = set()
    for i in range(N):
        info = []
        assert same(ex[i, :8], M.sim3_vec(M.sim3_exp(u[i], info=info))), ("exp", i, u[i])
        assert ex[i, 8] == info[0]
        branches.add(info[0])
        assert same(fr[i], M.sim3_vec(M.sim3_from_rts(rts[i, :9], rts[i, 9:12], rts[i, 12]))), ("from_rts", i)
        assert same(mu[i], M.sim3_vec(M.sim3_mul(tup(ab[i, :8]), tup(ab[i, 8:])))), ("mul", i)
        assert same(inv[i], M.sim3_vec(M.sim3_inverse(tup(S[i])))), ("inverse", i)
        assert same(mp[i], M.sim3_map(tup(sx[i, :8]), [float(c) for c in sx[i, 8:]])), ("map", i)
        assert same(ro[i], M.quat_rotate([float(c) for c in sx[i, :4]], [float(c) for c in sx[i, 8:]])), ("rotate", i)
        assert same(mat[i], M.quat_to_mat([float(c) for c in q[i]])), ("to_mat", i)
        assert same(cj[i], M.quat_conj([float(c) for c in q[i]])), ("conj", i)
    assert branches == {0, 1, 2, 3}
    tr = rts[:, 0] + rts[:, 4] + rts[:, 8]
    assert (tr > 0).sum() > 100 and (tr <= 0).sum() > 100
    neg = rts[tr <= 0]
    which = {int(np.argmax([r[0], r[4], r[8]])) for r in neg}
    assert which == {0, 1, 2}                             # each case of the non-positive trace ran


def test_model_equals_recorded_g2o_sim3():
    """tests/golden/sim3g_g2o.npz holds data only: 300 inputs per function (made by inputs() above, stored with the results) and what g2o::Sim3 of the reference tree (ThirdParty/g2o/g2o/types/sim3.h over
    the vendored Eigen 3.2.10, compiled once outside the repository with g++ -O2 -ffp-contract=off -DEIGEN_DONT_VECTORIZE on x86-64) returned for them:
    Sim3(Vector7d), Sim3(R, t, s), operator*, inverse(), map() and rotation().toRotationMatrix().  No program text of the reference is in the file or in the
    repository.  The functions without a transcendental must agree bit for bit on any machine; the exponential map goes through libm's sin / cos / exp, so it
    is held to 1e-13 of the result's largest component (equal to the bit where the libm is the recording's)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "sim3g_g2o.npz"))
    u, rts, ab, S, sx = (g[k] for k in ("u", "rts", "ab", "S", "sx"))
    for i in range(len(u)):
        assert same(g["out_from_rts"][i], M.sim3_vec(M.sim3_from_rts(rts[i, :9], rts[i, 9:12], rts[i, 12]))), ("from_rts", i)
        assert same(g["out_mul"][i], M.sim3_vec(M.sim3_mul(tup(ab[i, :8]), tup(ab[i, 8:])))), ("mul", i)
        assert same(g["out_inverse"][i], M.sim3_vec(M.sim3_inverse(tup(S[i])))), ("inverse", i)
        assert same(g["out_map"][i], M.sim3_map(tup(sx[i, :8]), [float(c) for c in sx[i, 8:]])), ("map", i)
        assert same(g["out_to_mat"][i], M.quat_to_mat([float(c) for c in S[i, :4]])), ("to_mat", i)
        e = M.sim3_vec(M.sim3_exp(u[i]))
        assert np.abs(e - g["out_exp"][i]).max() <= 1e-13 * np.abs(e).max(), ("exp", i)
