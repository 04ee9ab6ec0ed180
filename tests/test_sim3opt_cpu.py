"""CPU: tests/sim3opt_model.py, the restatement of cOptimizer::OptimizeSim3 the device is held to, pinned on its own; the tolerance of the GPU tests derived
from it; the argument checks of mcs_sim3_optimize without a device; the entry point's presence in library, binding and header.

The tolerance.  For every scene of tests/sim3opt_scenes.py the model runs with its edge sums reversed and under eight seeds that move every libm result by up
to +-k ulp (sim3opt_model.ULP: the OpenCL full-profile bounds, no document at hand states ocml's own).  The largest relative spread of S12 is the model's own
uncertainty (SPREAD below, measured on x86-64 and asserted), the device may differ by twice the largest (BOUND), and every scene keeps each decision further
from its edge than that and takes the same decisions in all ten runs, so the GPU tests compare decisions exactly."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import poseopt_model as PM
import sim3opt_model as M
import sim3opt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")

# the model's own uncertainty per scene, as measured (rounded up to two digits); 0: no transcendental and no sum decides anything (the return-0 paths)
SPREAD = {"n0": 0.0, "n2": 0.0, "n3": 2.2e-6, "n63": 1.2e-7, "n64": 6.8e-7, "n65": 9.3e-8, "n255": 1.3e-7, "n256": 9.0e-8, "n257": 2.6e-8, "n513": 4.9e-8,
          "nbad0": 3.0e-7, "nbad": 4.0e-7, "return0": 0.0, "dead_round_two": 8.4e-8, "far_start": 9.4e-8, "tiny_step": 2.2e-11, "negative_trace": 1.8e-7}
BOUND = 4.4e-6


@pytest.fixture(scope="module")
def pkg():
    import importlib
    return importlib.import_module("multicol-slam_amd")


# ---------------------------------------------------------------------------------------------- the Sim3 arithmetic
def expm_series(G):
    """matrix exponential by scaling and squaring around a Taylor series, independent of the closed form under test"""
    k = max(0, int(math.ceil(math.log2(max(np.abs(G).sum(1).max(), 1e-300)))) + 4)
    A = G / 2.0 ** k
    E, term = np.eye(4), np.eye(4)
    for i in range(1, 30):
        term = term @ A / i
        E = E + term
    for _ in range(k):
        E = E @ E
    return E


def test_exponential_map_in_all_four_branches():
    """Sim3(v) against exp of the generator [[Omega + sigma I, upsilon], [0, 0]] = [[s R, t], [0, 1]].  Where theta < 1e-5 the reference uses R = I + Omega +
    Omega^2 (true: Omega^2 / 2) and A = 1/2, B = 1/6: errors of theta^2 / 2 <= 5e-11 in R and of theta in W; where |sigma| < 1e-5 it uses C = 1 (true:
    1 + sigma / 2 + ...): an error of sigma / 2 <= 5e-6 relative in t.  The full branch is exact to rounding."""
    rng = np.random.default_rng(3)
    seen = set()
    for th, sg in ((1e-7, 1e-7), (1e-6, 0.0), (0.7, 1e-6), (2.5, -9e-6), (1e-6, 0.3), (9e-6, -0.8), (0.4, 0.2), (3.0, -0.6), (1.2e-5, 1.2e-5)):
        for _ in range(20):
            d = rng.normal(0, 1, 3)
            v = np.concatenate([d / np.linalg.norm(d) * th, rng.normal(0, 1, 3), [sg]])
            info = []
            q, t, s = M.sim3_exp(v, info=info)
            seen.add(info[0])
            G = np.zeros((4, 4))
            G[:3, :3] = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]) + sg * np.eye(3)
            G[:3, 3] = v[3:6]
            E = expm_series(G)
            tol_R = 1e-12 + (th * th if th < M.EPS else 0.0)
            tol_t = (1e-12 + (th if th < M.EPS else 0.0) + (abs(sg) if abs(sg) < M.EPS else 0.0)) * (1.0 + np.abs(v[3:6]).max())
            assert s == math.exp(sg)
            assert np.abs(s * M.quat_to_mat(q) - E[:3, :3]).max() <= tol_R * 4, (th, sg)
            assert np.abs(np.array(t) - E[:3, 3]).max() <= tol_t * 4, (th, sg)
    assert seen == {0, 1, 2, 3}


def test_inverse_and_product_identities():
    rng = np.random.default_rng(4)
    for _ in range(200):
        S1 = M.sim3_exp(rng.normal(0, 0.8, 7))
        I = M.sim3_mul(S1, M.sim3_inverse(S1))
        assert np.abs(M.sim3_vec(I) - [0, 0, 0, 1, 0, 0, 0, 1]).max() < 1e-13
        x = [float(v) for v in rng.normal(0, 3, 3)]
        back = M.sim3_map(M.sim3_inverse(S1), M.sim3_map(S1, x))
        assert np.abs(np.array(back) - x).max() < 1e-12
        S2 = M.sim3_exp(rng.normal(0, 0.8, 7))
        assert np.abs(np.array(M.sim3_map(M.sim3_mul(S1, S2), x)) - M.sim3_map(S1, M.sim3_map(S2, x))).max() < 1e-12


def test_quaternion_from_matrix_every_case():
    """trace > 0 and the three cases behind a non-positive trace give the rotation back"""
    for ax, ang in (([1, 2, 3], 0.4), ([1, 0.1, 0.1], 3.0), ([0.1, 1, 0.1], 3.0), ([0.1, 0.1, 1], 3.0), ([1, 0, 0], math.pi), ([0, 0, 1], math.pi)):
        R = S.rot(ax, ang)
        q = M.quat_from_mat(R)
        assert (np.trace(R) > 0) == (ang < 2.0)
        assert abs(sum(c * c for c in q) - 1.0) < 1e-14 and np.abs(M.quat_to_mat(q) - R).max() < 1e-14


def analytic_jacobian(pr, Sx):
    """d e / d xi of both edges at xi = 0, estimate Sim3(xi) * S: for e12, Y = S.map(P2) and d Y / d (omega, upsilon, sigma) = [-[Y]x, I, Y]; for e21,
    (Sim3(xi) S)^-1 = S^-1 Sim3(-xi), so d / d xi = (1 / s) R^T (-[-[P1]x, I, P1]).  Then e = obs - WorldToImg(invMat(M_c) (., 1)): [n][2][2][7]"""
    idx = pr.pairs()
    P1, P2 = M.rig_points(pr, idx)
    q, t, s = Sx
    Rs = M.quat_to_mat(q)
    Sinv = M.sim3_inverse(Sx)
    J = np.zeros((len(idx), 2, 2, 7))
    skew = lambda y: np.array([[0, -y[2], y[1]], [y[2], 0, -y[0]], [-y[1], y[0], 0]])
    for k in range(len(idx)):
        for g in range(2):
            if g == 0:
                Y = np.array(M.sim3_map(Sx, [float(P2[a][k]) for a in range(3)]))
                dY = np.concatenate([-skew(Y), np.eye(3), Y[:, None]], 1)
            else:
                P = np.array([float(P1[a][k]) for a in range(3)])
                Y = np.array(M.sim3_map(Sinv, list(P)))
                dY = (Rs.T / s) @ -np.concatenate([-skew(P), np.eye(3), P[:, None]], 1)
            c = pr.cam[idx[k], g]
            inv = PM.inv_mat(pr.Mc[c])
            p = inv[:3, :3] @ Y + inv[:3, 3]
            D = PM.d_world_to_img(pr.cams[c], p[0:1], p[1:2], p[2:3])[0]      # [2][3]
            J[k, g] = -D @ inv[:3, :3] @ dY
    return J


def test_numeric_jacobian_against_the_analytic_derivative():
    """Central differences with a step of 1e-9 carry the rounding of the two projections, eps |uv| / 2e-9 with |uv| <= 1e3 px: about 1e-4 per entry of the
    image-plane derivative times the lever of the parameter (the point's distance for a rotation or the scale).  Their truncation term, 1e-18 |e'''|, is nil.
    Held to 2e-3 absolute + 1e-5 relative: the Jacobian entries are of the order 1e2 .. 1e3."""
    pr = S.build("nbad0")
    Sx = M.sim3_from_rts(pr.R12, pr.t12, pr.s12)
    idx = pr.pairs()
    P1, P2 = M.rig_points(pr, idx)
    Jn = M.numeric_jacobian(pr, Sx, idx, P1, P2, [PM.inv_mat(m) for m in pr.Mc])
    Ja = analytic_jacobian(pr, Sx)
    assert np.abs(Ja).max() > 50.0
    assert np.all(np.abs(Jn - Ja) <= 2e-3 + 1e-5 * np.abs(Ja)), float(np.abs(Jn - Ja).max())


def test_ldlt_of_seven():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(7, 7))
    A = A @ A.T + 0.1 * np.eye(7)
    b = rng.normal(size=7)
    ok, x = M.ldlt6(A, b)
    assert ok and np.abs(A @ x - b).max() < 1e-10
    A[3, 3] = -1.0
    assert not M.ldlt6(A, b)[0]


# ---------------------------------------------------------------------------------------------- the tolerance and the margins
@pytest.mark.parametrize("name", list(S.ALL))
def test_scene_spread_and_margins(name):
    m = S.model(name)
    sp = S.spread(name)
    print("sim3opt %-16s spread %.2e margin %.2e" % (name, sp, m.margin))
    assert sp <= SPREAD[name], (name, sp)
    assert m.margin > S.bound() and S.stable(name), (name, m.margin)     # else: re-seed the scene (tools/sim3opt_seed_search.py)


def test_the_bound():
    assert 0.0 < S.bound() <= BOUND and S.bound() == 2.0 * max(S.spread(n) for n in S.ALL)
    assert S.bound("chi2") <= 2.4e-6 and S.bound("lam") <= 2.5e-3


def test_scenes_show_their_paths():
    g = S.model
    assert g("n0").n_corr == 0 and g("n0").iters == [0, 0] and g("n2").iters == [5, 0] and g("n2").n_inliers == 0
    assert g("n3").n_inliers == 3 and g("n3").iters[1] >= 1
    for n in ("n63", "n64", "n65", "n255", "n256", "n257", "n513"):
        assert g(n).n_bad1 > 0 and g(n).iters[0] == 5 and g(n).iters[1] >= 1, n
    assert [S.build(n).n for n in S.SIZES] == [0, 2, 3, 63, 64, 65, S.T - 1, S.T, S.T + 1, 2 * S.T + 1]
    assert {len(S.build(n).Mc) for n in S.SIZES} == {1, 3, 32}
    assert g("nbad0").n_bad1 == 0 and 1 <= g("nbad0").iters[1] <= 5
    assert g("nbad").n_bad1 > 0 and g("nbad").iters[1] > 5
    assert 0 < g("return0").n_corr - g("return0").n_bad1 < 3 and g("return0").n_inliers == 0
    assert g("dead_round_two").stop == [M.STOP_GAIN, M.STOP_NOT_RUN]
    assert g("far_start").trials[0, :3].max() > 1
    assert g("tiny_step").branches[0] == 0 and g("nbad").branches[0] == 3      # |sigma| and theta of the first step below / above 1e-5
    pr = S.build("negative_trace")
    assert np.trace(pr.R12) < 0 and np.trace(S.build("nbad").R12) > 0


# ---------------------------------------------------------------------------------------------- the quirks: each scene fails when the quirk is "repaired"
def test_get_sigma2_weight():
    """:188: the information of e21 is GetSigma2(octave2), not its inverse"""
    m, f = S.model("nbad0"), S.model("nbad0", fix=("inverse_w2",))
    assert M.rel_spread(m.S12, f.S12) > 100 * S.bound()
    pr = S.build("nbad0")
    assert np.array_equal(pr.w[:, 1], pr.sigma2[pr.octave[:, 1]]) and np.array_equal(pr.w[:, 0], 1.0 / pr.sigma2[pr.octave[:, 0]])


def test_either_edge_rejects_a_correspondence():
    """:215-216: chi2 of e12 OR of e21 above the bound"""
    m, f = S.model("dead_round_two"), S.model("dead_round_two", fix=("both_edges",))
    assert m.n_bad1 > f.n_bad1 and m.keep.sum() < f.keep.sum()


def test_ten_iterations_against_five():
    """:228-232"""
    m, f = S.model("nbad"), S.model("nbad", fix=("always_5",))
    assert m.n_bad1 > 0 and m.iters[1] > 5 and f.iters[1] == 5 and M.rel_spread(m.S12, f.S12) > S.bound()
    assert S.model("nbad0").n_bad1 == 0 and S.model("nbad0").iters[1] <= 5


def test_return_zero_leaves_the_estimate_but_nulls_the_matches():
    """:234-235: return 0 before g2oS12 is written; the matches of :219 stay nulled"""
    pr, m, f = S.build("return0"), S.model("return0"), S.model("return0", fix=("write_back",))
    assert m.n_inliers == 0 and m.iters[0] == 5 and m.keep.sum() == m.n_corr - m.n_bad1 < 3
    assert np.array_equal(m.S12, M.sim3_vec(M.sim3_from_rts(pr.R12, pr.t12, pr.s12))) and not np.array_equal(f.S12, m.S12)


def test_dead_second_round():
    """round one ends on the gain test; the terminate action's stop flag is only cleared by a call with iteration -1, which this g2o never makes
    (sparse_optimizer.cpp:376-413 calls postIteration(i) with i >= 0 only), so the second optimize() runs no iteration"""
    m, f = S.model("dead_round_two"), S.model("dead_round_two", fix=("clear_stop",))
    assert m.stop == [M.STOP_GAIN, M.STOP_NOT_RUN] and m.iters[1] == 0 and m.n_bad1 > 0
    assert f.iters[1] >= 1 and not np.array_equal(f.S12, m.S12)


def test_quaternion_is_never_normalised():
    """R = I + Omega + Omega^2 of the small-angle branches is no rotation, Quaterniond(R) of it no unit quaternion, and nothing normalises the product"""
    q = M.sim3_exp([3e-6, -2e-6, 1e-6, 0, 0, 0, 0])[0]
    assert abs(sum(c * c for c in q) - 1.0) > 1e-13
    m, f = S.model("nbad"), S.model("nbad", fix=("normalize",))
    assert not np.array_equal(m.S12, f.S12)
    assert abs(np.sum(f.S12[:4] ** 2) - 1.0) < 1e-14 or abs(np.sum(m.S12[:4] ** 2) - 1.0) != abs(np.sum(f.S12[:4] ** 2) - 1.0)


def test_cameras_are_looked_up_crossed():
    """e12 projects with keypoint_to_cam1[i2], e21 with keypoint_to_cam2[i] (the point vertex an edge holds carries the other side's index)"""
    pr = S.build("nbad")
    kp = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])

    class Rig:
        def __init__(self, Mt):
            self.Mt = Mt

        def Get_M_t(self):
            return self.Mt
    kf1, kf2, matches, at, drop = S.keyframes(pr, Rig, kp)
    got, at2 = M.keyframe_problem(kf1, kf2, matches, pr.R12, pr.t12, pr.s12, pr.Mc, pr.cams, pr.std_sim)
    assert at2 == at and np.array_equal(got.cam, pr.cam) and np.array_equal(got.w, pr.w) and np.array_equal(got.Xw, pr.Xw) and np.array_equal(got.obs, pr.obs)
    assert np.array_equal(M.optimize(got).S12, S.model("nbad").S12)
    straight, _ = M.keyframe_problem(kf1, kf2, matches, pr.R12, pr.t12, pr.s12, pr.Mc, pr.cams, pr.std_sim, fix=("straight_cams",))
    assert not np.array_equal(straight.cam, pr.cam)


def test_nonfinite_input_is_not_optimised():
    pr = S.build("nbad")
    pr.Xw[1, 0, 0] = np.nan
    m = M.optimize(pr)
    assert m.status == M.SIM3_NONFINITE and m.n_inliers == 6 and m.keep.all() and m.iters == [0, 0]
    assert np.array_equal(m.S12, M.sim3_vec(M.sim3_from_rts(pr.R12, pr.t12, pr.s12)))


def test_device_kind_guards_drop_the_pair():
    pr = S.build("nbad0")
    pr.cam[4, 1] = 3
    m = M.optimize(pr)
    assert m.n_corr == 39 and m.keep[4] == 1 and m.status == 0


# ---------------------------------------------------------------------------------------------- the entry point without a device
def test_library_exports_the_entry_point(pkg):
    L = pkg.lib()
    assert hasattr(L, "mcs_sim3_optimize") and "mcs_sim3_optimize" in pkg._capi.EXPORTS
    txt = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    assert "int mcs_sim3_optimize(" in txt and "#define MCS_ABI_VERSION 10" in txt and L.mcs_abi_version() == 10


def test_empty_batch_and_null_arguments(pkg):
    cap, L = pkg._capi, pkg.lib()
    assert L.mcs_sim3_optimize(None, 0, None, None, None, 0, None, None, None, None, None, 0, None, None, None, None, None) == 0
    assert L.mcs_sim3_optimize(None, 1, None, None, None, 1, None, None, None, None, None, 0, None, None, None, None, None) == cap.MCS_ERR_INVALID
    assert b"null" in L.mcs_last_error()


def test_struct_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "mcs_c.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(mcs_sim3opt_problem), offsetof(mcs_sim3opt_problem, w), offsetof(mcs_sim3opt_problem, n), sizeof(mcs_sim3opt_diag), '
                   'offsetof(mcs_sim3opt_diag, iters), offsetof(mcs_sim3opt_diag, stop), offsetof(mcs_sim3opt_diag, trials), offsetof(mcs_sim3opt_diag, lambda), '
                   'offsetof(mcs_sim3opt_diag, chi2)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    F, dt = pkg._capi.Sim3OptProblem, pkg._capi.SIM3OPT_DIAG_DTYPE
    assert got == [C.sizeof(F), F.w.offset, F.n.offset, dt.itemsize, dt.fields["iters"][1], dt.fields["stop"][1], dt.fields["trials"][1], dt.fields["lam"][1],
                   dt.fields["chi2"][1]]


def test_argument_checks_without_a_device(tmp_path):
    """csrc/mcs_sim3opt_guard.hip alone, through tests/cpp/sim3opt_guard_driver.cpp, compiled by hipcc in host-only mode"""
    exe = tmp_path / "sim3opt_guard_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "sim3opt_guard_driver.cpp"),
                           os.path.join(CSRC, "mcs_sim3opt_guard.hip"), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, rc, text = line.split("\t")
        out[name] = (int(rc), text)
    ok = [n for n, (rc, _) in out.items() if rc == 0]
    assert sorted(ok) == sorted(["valid", "empty", "null_keep_of_empty", "camera.device"])
    for n in ("negative", "null_ctx", "null_keep", "null_Xw", "null_w", "null_S12", "null_Mt", "cams_0", "cams_33", "correspondences",
              "correspondences.negative", "camera", "camera.second", "camera.negative", "polynomial"):
        assert out[n][0] == -1, n
    assert out["deferred"][0] == -4 and out["deferred+camera"][0] == -4          # refused before the contents are looked at
    assert "camera" in out["camera"][1] and "65536" in out["correspondences"][1] and "null" in out["null_keep"][1]


def test_facade_driver_compiles_and_links(pkg, tmp_path):
    exe = tmp_path / "facade_driver_sim3opt"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_sim3opt.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 2       # no arguments: the usage exit, before anything touches a device
