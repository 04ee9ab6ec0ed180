"""CPU: Sim3::log, the 3x3 partial-pivot LU behind it and the essential graph's edge error in csrc/mcs_sim3g.h, compiled for the host alone
(tests/cpp/sim3g_log_driver.cpp, no HIP call) with the library's floating-point flags and held BIT FOR BIT to tests/essgraph_model.py.  Both sides call the
host's libm (log, acos, sin, cos, sqrt), so equality is exact.  1500 inputs per branch of log (|sigma| < 1e-5 or not, d > 1 - 1e-5 or not), with d and sigma on
either side of their thresholds, rotations near a half turn (where the LU swaps rows), quaternions that are not unit; 1500 edges; 1500 raw 3x3 systems whose
pivot rows are compared as well; and log(exp(v)) ~= v."""
import os
import subprocess

import numpy as np
import pytest

import essgraph_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
N = 1500


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sim3g_log") / "sim3g_log_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O3", "-std=c++17", "-ffp-contract=off",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-I" + CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "sim3g_log_driver.cpp"), "-o", str(exe)])
    return exe


def run(driver, tmp_path, S, ed, wb):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([len(S), len(ed), len(wb)], np.int32).tobytes())
        for p in (S, ed, wb):
            f.write(np.ascontiguousarray(p, np.float64).tobytes())
    subprocess.check_call([str(driver), str(src), str(dst)])
    raw = np.fromfile(dst, np.float64)
    a, b = 10 * len(S), 10 * len(S) + 7 * len(ed)
    assert len(raw) == b + 5 * len(wb)
    return raw[:a].reshape(-1, 10), raw[a:b].reshape(-1, 7), raw[b:].reshape(-1, 5)


def quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a, axis=-1, keepdims=True)
    return np.concatenate([a * np.sin(angle / 2)[..., None], np.cos(angle / 2)[..., None]], -1)


TH0 = float(np.sqrt(2e-5))   # d = cos(theta) crosses 1 - 1e-5 here


def branch_inputs(rng, br):
    """N Sim3 for branch br = 2 * (|sigma| >= eps) + (d <= 1 - eps); the first ones sit at the thresholds, on the side the branch needs or on both"""
    big_s, big_t = br >> 1, br & 1
    th = rng.uniform(0.01, np.pi, N) if big_t else rng.uniform(0.0, 0.9 * TH0, N)
    sg = rng.normal(0, 0.3, N) if big_s else rng.uniform(-0.9e-5, 0.9e-5, N)
    if big_t:
        th[:200] = np.pi - rng.uniform(0, 0.4, 200)           # near a half turn: the LU swaps rows
    edge_t = TH0 * (1 + np.array([-1e-3, -1e-6, -1e-9, 0.0, 1e-9, 1e-6, 1e-3]))
    edge_s = 1e-5 * (1 + np.array([-1e-3, -1e-9, 0.0, 1e-9, 1e-3]))
    k = 200
    for t in edge_t:                                              # both thresholds crossed: whatever branch results is compared, not assumed
        for s in edge_s:
            for sign in (1.0, -1.0):
                th[k], sg[k] = t, sign * s
                k += 1
    S = np.zeros((N, 8))
    S[:, :4] = quat(rng.normal(0, 1, (N, 3)), th)
    S[:, 4:7] = rng.normal(0, 2, (N, 3))
    S[:, 7] = np.exp(sg)
    S[N - 100:, :4] *= rng.uniform(0.999, 1.001, (100, 1))        # not unit: log() does not care
    return S


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)   # bit for bit; a NaN equals a NaN whatever its sign (d < -1 behind a non-unit quaternion)
    nan = np.isnan(a)
    return a.shape == b.shape and (nan == np.isnan(b)).all() and np.where(nan, 0.0, a).tobytes() == np.where(nan, 0.0, b).tobytes()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(11)
    S = np.concatenate([branch_inputs(rng, br) for br in range(4)])
    pool = np.concatenate([branch_inputs(rng, br) for br in (1, 3, 3)])[rng.permutation(3 * N)]
    ed = np.concatenate([pool[:N], pool[N:2 * N], M.sim3_vec(M.sim3_inverse(M.sim3_of(pool[2 * N:])))], 1)
    ed[: N // 2, :8] = M.sim3_vec(M.sim3_mul(M.sim3_of(pool[2 * N:2 * N + N // 2]), M.sim3_inverse(M.sim3_of(pool[N:N + N // 2]))))   # a near-zero residual
    W = rng.normal(0, 1, (N, 9))
    W[:300] += np.array([3.0, 0, 0, 0, 3.0, 0, 0, 0, 3.0])       # diagonally dominant: no swap
    W[300:320, 0] = 0.0                                           # a zero on the diagonal: a forced swap
    W[320:330, [0, 3, 6]] = [[1.0, -1.0, 0.5]]                    # a tie: the first one is kept
    wb = np.concatenate([W, rng.normal(0, 1, (N, 3))], 1)
    return S, ed, wb


def test_log_lu_and_edge_equal_the_model_bit_for_bit(driver, tmp_path, data):
    S, ed, wb = data
    lg, ee, lu = run(driver, tmp_path, S, ed, wb)
    info = []
    want = M.sim3_log(M.sim3_of(S), info=info)
    assert same(lg[:, :7], want), np.nonzero((lg[:, :7] != want).any(1))[0][:10]
    assert (lg[:, 7] == info[0]).all() and (lg[:, 8:] == info[1]).all()
    for br in range(4):                                           # every branch got its 1500, give or take the threshold inputs that fell across
        assert (lg[:, 7] == br).sum() >= N - 80, br
    assert ((lg[:, 8] != 0) | (lg[:, 9] != 1)).sum() > 50         # the LU swapped rows
    assert ((lg[:, 8] == 0) & (lg[:, 9] == 1)).sum() > 50
    assert same(ee, M.edge_error(M.sim3_of(ed[:, :8]), M.sim3_of(ed[:, 8:16]), M.sim3_of(ed[:, 16:])))
    info = []
    assert same(lu[:, :3], M.lu3_solve(wb[:, :9], wb[:, 9:], info=info))
    assert (lu[:, 3:] == info[0]).all()
    assert set(map(tuple, lu[:, 3:].astype(int))) == {(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2)}
    assert (lu[320:330, 3] == 0).all()


def test_lu3_solves_the_system(data):
    wb = data[2]
    x = M.lu3_solve(wb[:, :9], wb[:, 9:])
    A = wb[:, :9].reshape(-1, 3, 3)
    cond = np.linalg.cond(A)
    r = np.einsum("nij,nj->ni", A, x) - wb[:, 9:]
    assert (np.abs(r).max(1) <= 1e-13 * cond * np.abs(wb[:, 9:]).max(1))[cond < 1e6].all()


def test_log_inverts_exp():
    rng = np.random.default_rng(3)
    v = rng.normal(0, 0.5, (N, 7))
    w = rng.normal(0, 1, (N, 3))
    v[:, :3] = w / np.linalg.norm(w, axis=1)[:, None] * rng.uniform(0.01, 3.0, N)[:, None]
    back = M.sim3_log(M.sim3_exp(v))
    assert np.abs(back - v).max() <= 1e-9                        # Rodrigues both ways: rounding only (acos near a half turn costs the most)
    v[:, :3] *= (rng.uniform(0, 0.9 * TH0, N) / np.linalg.norm(v[:, :3], axis=1))[:, None]
    v[: N // 2, 6] = rng.uniform(-0.9e-5, 0.9e-5, N // 2)
    back = M.sim3_log(M.sim3_exp(v))
    # below the threshold log() takes omega = deltaR / 2 = sin(theta) * axis for theta * axis: off by theta^3 / 6 <= 1.5e-8, and A, B as constants
    err = np.abs(back - v)
    assert err[:, [0, 1, 2, 6]].max() <= 1e-7 and err[: N // 2].max() <= 1e-7
    # A quirk kept: with d > 1 - eps and |sigma| >= eps, sim3.h:199 (and :126 of the exponential) has B = (sigma^2 / 2 - sigma + 1) s / sigma^3 where the
    # limit of the general formula is ((sigma^2 / 2 - sigma + 1) s - 1) / sigma^3.  B is of the order 1 / sigma^3 then, and upsilon is NOT the inverse of
    # the exponential's for rotations between 1e-5 (where the exponential leaves its own series) and 4.5e-3.  A "repaired" B fails here.
    big = np.linalg.norm(v[N // 2:, :3], axis=1) > 1e-3
    assert err[N // 2:][big][:, 3:6].max() > 1e-3
