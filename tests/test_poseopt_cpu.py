"""CPU: the model of cOptimizer::PoseOptimization (tests/poseopt_model.py) pinned to the reference's own code where that is possible without g2o (the
residual), its hand-derived Jacobian against a central difference, every reproduced quirk and project choice of DESIGN 7 on a scene found by a seed search
over the model (tools/poseopt_seed_search.py), and the boundary of mcs_pose_optimization that needs no device (exports, struct layouts, the argument checks).

Quirk 1 of the issue ("stale errors") is not in the sources: SparseOptimizerTerminateAction::operator() calls computeActiveErrors() itself (core/
sparse_optimizer_terminate_action.cpp:29) in every post-iteration call, and optimize() makes that call after every iteration (core/sparse_optimizer.cpp:413).
So the gain test and both outlier passes read the errors of the CURRENT estimate.  test_errors_are_those_of_the_current_estimate holds the model to that and
says why no scene tells the two readings apart.

Jacobian agreement, measured on the scenes below (65 edges, rigs of 2 and 3 cameras): largest |analytic - central difference| 8.7e-08 where the entries reach
3e+03 pixels per unit of pose, with h = 1e-6, against an estimate of 2.2e-07; the bound asserted is 10 x the truncation + rounding estimate of that difference (see the test)."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import poseopt_model as PM
import poseopt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")
REF_SO = os.path.join(ROOT, "oracle", "_ref", "libmcs_ref.so")
have_ref = pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


# ---------------------------------------------------------------------------------------------- residual and Jacobian
@have_ref
def test_residual_equals_the_reference_code_bit_for_bit():
    """cayley2hom through the reference's template, then cMultiCamSys_(M_t, M_c) -> invMat(M_t * M_c[c]) * (X, 1) -> WorldToImg, all compiled from the
    reference's sources (oracle/_ref): what EdgeProjectXYZ2MCS::computeError evaluates."""
    import oracle_lib as O
    ref = C.CDLL(REF_SO)
    ref.ref_cayley2hom.argtypes = [C.c_void_p, C.c_void_p]
    ref.ref_world_to_cam.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(O.Ocam), C.POINTER(C.c_void_p), C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    for nr, seed in ((3, 0), (2, 1), (3, 2)):
        pr = S.scene(seed, 400, nr, start=0.5)
        idx = pr.edges()
        rng = np.random.default_rng(seed)
        for pose in (pr.pose0, pr.pose0 + rng.normal(0, 0.2, 6), rng.normal(0, 1.0, 6)):
            hom = lambda c6: (lambda M: (ref.ref_cayley2hom(np.ascontiguousarray(c6, np.float64).ctypes.data, M.ctypes.data), M)[1])(np.zeros((4, 4)))
            M_t, M_c = hom(pose), np.stack([hom(m) for m in pr.Mc_min])
            assert np.array_equal(M_t, PM.cayley2hom(pose))
            n = len(idx)
            uv, fl, inv = np.zeros((n, 2)), np.zeros(n, np.uint8), np.zeros((nr, 4, 4))
            oc = (O.Ocam * nr)(*[O.make_ocam(c) for c in pr.cams])
            pts, pc = np.ascontiguousarray(pr.pos[pr.points[idx]]), np.ascontiguousarray(pr.cam[idx])
            assert ref.ref_world_to_cam(M_t.ctypes.data, M_c.ctypes.data, oc, None, nr, pts.ctypes.data, pc.ctypes.data, n, uv.ctypes.data, fl.ctypes.data,
                                        inv.ctypes.data) == 0
            assert np.array_equal(inv, PM.rig_from_min(pose, pr.Mc_min)[1])
            e = PM.residual(pr, pose, idx)
            z = pr.xy[idx].astype(np.float64)
            assert np.array_equal(e[:, 0], z[:, 0] - uv[:, 0]) and np.array_equal(e[:, 1], z[:, 1] - uv[:, 1])


def test_residual_equals_the_oracle_bit_for_bit(oracle):
    """the same through the oracle's orc_world_to_cam, which tests/test_oracle_vs_ref.py pins to the reference: runs where oracle/_ref is absent too"""
    pr = S.scene(3, 300, 3, start=0.5)
    idx = pr.edges()
    for pose in (pr.pose0, pr.pose0 * 3.0):
        uv, _ = oracle.world_to_cam(PM.rig_from_min(pose, pr.Mc_min)[1], pr.cams, None, pr.pos[pr.points[idx]], pr.cam[idx])
        u, v = PM.project(pr, pose, idx)
        assert np.array_equal(u, uv[:, 0]) and np.array_equal(v, uv[:, 1])


def test_jacobian_against_a_central_difference():
    """J = d e / d pose by the chain rule against (e(p + h) - e(p - h)) / 2h.  The difference of the two is bounded by the truncation term h^2/6 |e'''| plus the
    rounding term eps |e| / h.  |e'''| is estimated from third differences of the residual itself (step 1e-3), |e| <= the image size (1e3 px), eps = 2.2e-16.
    The test prints the measured agreement and asserts it with a 10x margin over that estimate."""
    h, worst, bound = 1e-6, 0.0, 0.0
    for nr, seed in ((3, 0), (2, 5), (3, 14)):
        pr = S.scene(seed, 65, nr, start=0.3)
        idx = pr.edges()
        pose = pr.pose0
        J = PM.jacobian(pr, pose, idx)
        for k in range(6):
            d = np.zeros(6)
            d[k] = 1.0
            num = (PM.residual(pr, pose + h * d, idx) - PM.residual(pr, pose - h * d, idx)) / (2 * h)
            g = 1e-3
            third = (PM.residual(pr, pose + 2 * g * d, idx) - 2 * PM.residual(pr, pose + g * d, idx) + 2 * PM.residual(pr, pose - g * d, idx)
                     - PM.residual(pr, pose - 2 * g * d, idx)) / (2 * g ** 3)
            est = h * h / 6 * np.abs(third).max() + 2.2e-16 * 1e3 / h
            worst, bound = max(worst, float(np.abs(J[:, :, k] - num).max())), max(bound, float(est))
            assert np.abs(J[:, :, k] - num).max() <= 10 * est, (nr, seed, k, np.abs(J[:, :, k] - num).max(), est)
        assert np.abs(J).max() > 100.0   # pixels per unit of pose: a Jacobian of zeros would pass the bound above
    print("jacobian: worst |analytic - numeric| %.3g, estimate %.3g" % (worst, bound))


def test_jacobian_constant_norm_branch():
    """a point on the camera axis: norm == 0 is replaced by 1e-14 (src/cam_model_omni.cpp:149), a constant; the derivative stays finite"""
    cams, _ = S.rig(1)
    D = PM.d_world_to_img(cams[0], np.array([0.0]), np.array([0.0]), np.array([2.0]))
    assert np.isfinite(D).all()


def test_ldlt_positivity_and_solution():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(6, 6))
    A = A @ A.T + 1e-3 * np.eye(6)
    b = rng.normal(size=6)
    ok, x = PM.ldlt6(A, b)
    assert ok and np.allclose(A @ x, b, rtol=1e-9, atol=1e-9)
    assert PM.ldlt6(np.zeros((6, 6)), b)[0] is False          # the zero matrix is "not positive" here
    A[2, 2] = -1.0
    assert PM.ldlt6(A, b)[0] is False
    A[2, 2] = np.nan
    assert PM.ldlt6(A, b)[0] is False


# ---------------------------------------------------------------------------------------------- the quirks, each on a scene that shows it
def _same(a, b):
    return np.array_equal(a.pose, b.pose) and np.array_equal(a.outlier, b.outlier) and a.n_inliers == b.n_inliers and a.share == b.share and a.chi2 == b.chi2


@pytest.mark.parametrize("name", sorted({**S.SIZES, **S.QUIRKS}))
def test_scene_decisions_are_off_their_edges(name):
    """what lets the GPU tests compare decisions exactly; e1 (one edge: a perfect fit, chi2 -> 0, every late decision is rounding noise) is the one scene that
    cannot have it, and its GPU test compares no decision"""
    m = S.model(name)
    assert m.status == PM.POSE_OK and m.nInitial == len(S.build(name).edges())
    if name == "e1":
        assert m.margin < PM.MARGIN and m.n_inliers == 1
    else:
        assert m.margin >= PM.MARGIN, m.margin


def test_errors_are_those_of_the_current_estimate():
    """Quirk 1 as the sources have it: the terminate action recomputes the active errors (:29), so the chi2 it judges and the errors both outlier passes read
    are those of the returned pose.  Held on the suite's scenes and on a scene polished until an iteration rejects trial after trial (started at a converged
    pose, 7-9 rejections by rounding noise, then rho == 0 and Terminate).
    The other reading (fix "stale_errors": the action reads what the last trial left) gives the SAME result on every one of them, and this is why the kernel
    keeps no per-edge error: the trial loop (optimization_algorithm_levenberg.cpp:102-149) only ends behind an accepted trial, whose errors are the current
    estimate's, or behind rho == 0, a trial that did not move chi2.  Ten rejections in a row would be the exception; lambda grows by 2^45 over them, the step
    underflows against the pose long before, and rho == 0 ends the loop first.  So no scene can make a test fail with this quirk "fixed"."""
    pr = S.build("dead_round_two")
    r = PM.optimize(pr)
    polished = None
    for it in range(8):
        pr.pose0 = r.pose
        r = PM.optimize(pr)
        if r.trials[0].max() >= 5 and r.stop[0] == PM.STOP_TRIALS:
            polished = (S.build("dead_round_two"), r)
            polished[0].pose0 = pr.pose0.copy()
            break
    assert polished is not None
    cases = [(S.build(n), S.model(n)) for n in ("e3", "e65", "dead_round_two", "round_two_runs")] + [polished]
    for pr, m in cases:
        idx = pr.edges()
        idx = idx[m.outlier[idx] == 0] if m.iters[1] > 0 else idx      # the action last ran over the edges that were active then
        e = PM.residual(pr, m.pose, idx)
        w = pr.inv_sigma2[pr.octave[idx]]
        c2 = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        d = 1.345 * pr.huber
        if m.iters[1] == 0:
            assert m.chi2 == np.cumsum(np.where(c2 <= d * d, c2, 2 * np.sqrt(c2) * d - d * d))[-1]   # the action's chi2 IS the returned pose's
        assert ((c2 > d * d) == False).all() or m.iters[1] == 0        # round two's survivors were judged at the returned pose
        assert _same(m, PM.optimize(pr, fix={"stale_errors"}))


def test_dead_second_round():
    """Quirk 2: round one ends on the gain test, the stop flag is never cleared, the second optimize(10) runs no iteration."""
    m = S.model("dead_round_two")
    assert m.stop[0] == PM.STOP_GAIN and m.iters[0] < 10 and m.iters[1] == 0 and m.stop[1] == PM.STOP_NOT_RUN
    fixed = S.model("dead_round_two", fix=("clear_stop",))
    assert fixed.iters[1] > 0 and not _same(m, fixed)


def test_bad_points_and_repeated_points_are_used():
    """Quirk 3: only `if (pMP)`; a bad point gives an edge, a point held at two features gives two."""
    pr = S.build("dead_round_two")
    pr.points[1] = pr.points[0]          # feature 1 holds feature 0's point (its key no longer fits: an outlier edge)
    pr.bad = np.zeros(len(pr.pos), bool)
    pr.bad[pr.points[5]] = True
    pr.xy[5] += 40.0                     # the bad point's observation is wrong, and it still pulls
    m = PM.optimize(pr)
    assert m.nInitial == 65 and m.margin >= PM.MARGIN
    fixed = PM.optimize(pr, fix={"skip_bad"})
    assert fixed.nInitial == 63 and not _same(m, fixed) and m.outlier[5] == 1 and fixed.outlier[5] == 0


def test_second_round_when_it_runs():
    """Quirk 4: level-0 edges only, nBad carries over, a first-pass flag is never cleared."""
    m = S.model("round_two_runs")
    assert m.iters[0] == 10 and m.stop[0] == PM.STOP_ITERATIONS and m.iters[1] > 0 and m.outlier.any() and m.margin >= PM.MARGIN
    for fix in ("second_all_levels", "reset_nbad", "second_clears"):
        assert not _same(m, S.model("round_two_runs", fix=(fix,))), fix
    # the flags of the first pass survive: evaluate them at the pose where round one ended
    pr = S.build("round_two_runs")
    one = PM.optimize(pr, fix={"clear_stop"})   # same first round
    assert (m.outlier >= 0).all() and m.n_inliers == m.nInitial - int(m.outlier.sum())
    assert one.iters[0] == m.iters[0]


def test_inliers_is_the_outlier_share():
    """Quirk 5"""
    m = S.model("dead_round_two")
    nbad = int(m.outlier.sum())
    assert nbad > 0 and m.n_inliers == m.nInitial - nbad and m.share == nbad / m.nInitial
    assert S.model("dead_round_two", fix=("share_is_inliers",)).share == (m.nInitial - nbad) / m.nInitial != m.share


def test_no_correspondence():
    """Quirk 6: nothing is optimised; pose unchanged, count 0, share 0"""
    pr = S.scene(3, 0, 2, n_null=7)
    m = PM.optimize(pr)
    assert m.nInitial == 0 and np.array_equal(m.pose, pr.pose0) and m.n_inliers == 0 and m.share == 0.0 and not m.outlier.any() and m.iters == [0, 0]
    assert np.array_equal(m.MtMc_inv, PM.rig_from_min(pr.pose0, pr.Mc_min)[1])


def test_nonfinite_input_is_not_optimised():
    pr = S.build("e8")
    pr.pos[pr.points[3]] = np.nan
    m = PM.optimize(pr)
    assert m.status == PM.POSE_NONFINITE and np.array_equal(m.pose, pr.pose0) and not m.outlier.any() and m.n_inliers == 8 and m.share == 0.0


def test_device_kind_guards_drop_the_edge():
    pr = S.build("e65")
    full = PM.optimize(pr)
    a, b, c = pr.edges()[[0, 2, 4]]
    pr.points[a], pr.cam[b], pr.octave[c] = len(pr.pos), 7, -1
    m = PM.optimize(pr)
    assert m.nInitial == full.nInitial - 3 and not m.outlier[[a, b, c]].any()


def test_sum_order_spread_is_small():
    """what the GPU tests' tolerance is made of: index order against reversed order"""
    for name in ("e3", "e65", "round_two_runs"):
        assert S.spread(name) < 1e-8


# ---------------------------------------------------------------------------------------------- the library's surface, without a device
def test_library_exports_the_entry_point(pkg):
    L = pkg.lib()
    assert hasattr(L, "mcs_pose_optimization") and "mcs_pose_optimization" in pkg._capi.EXPORTS
    txt = open(os.path.join(ROOT, "include", "mcs_c.h")).read()
    assert re.search(r"\bint mcs_pose_optimization\(", txt)
    assert L.mcs_abi_version() == int(re.search(r"#define MCS_ABI_VERSION (\d+)", txt).group(1))   # additive: a host finds the call with dlsym


def test_empty_batch_and_null_arguments(pkg):
    cap, L = pkg._capi, pkg.lib()
    none = [None] * 7
    assert L.mcs_pose_optimization(None, 0, None, None, None, None, 0, None, 0, None, 0, *none) == cap.MCS_OK          # nproblems = 0: nothing is read
    assert L.mcs_pose_optimization(None, -1, None, None, None, None, 0, None, 0, None, 0, *none) == cap.MCS_ERR_INVALID
    assert L.mcs_pose_optimization(None, 1, None, None, None, None, 0, None, 0, None, 0, *none) == cap.MCS_ERR_INVALID
    assert b"null" in L.mcs_last_error()
    with pytest.raises(pkg.McsError):
        pkg.check(L.mcs_pose_optimization(None, 2, None, None, None, None, 2, None, 3, None, 1, *none))


def test_struct_layouts_match_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "mcs_c.h"\n#include <stdio.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mcs_pose_frame), '
                   'offsetof(mcs_pose_frame, points), offsetof(mcs_pose_frame, n), sizeof(mcs_pose_diag), offsetof(mcs_pose_diag, iters), offsetof(mcs_pose_diag, stop), '
                   'offsetof(mcs_pose_diag, trials), offsetof(mcs_pose_diag, lambda), offsetof(mcs_pose_diag, chi2)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    F, D, dt = pkg._capi.PoseFrame, pkg._capi.PoseDiag, pkg._capi.POSE_DIAG_DTYPE
    assert got == [C.sizeof(F), F.points.offset, F.n.offset, C.sizeof(D), D.iters.offset, D.stop.offset, D.trials.offset, D.lam.offset, D.chi2.offset]
    assert dt.itemsize == C.sizeof(D) and [dt.fields[k][1] for k in ("iters", "stop", "trials", "lam", "chi2")] == got[4:]


INVALID, UNSUPPORTED = -1, -4
GUARDS = {
    "valid": (0, ""), "empty": (0, ""), "negative": (INVALID, "nproblems"), "null_ctx": (INVALID, "null argument"), "null_outlier": (INVALID, "null argument"),
    "null_keys": (INVALID, "null argument"), "null_pos": (INVALID, "null argument"), "cams_0": (INVALID, "bad sizes"), "cams_33": (INVALID, "bad sizes"),
    "levels_0": (INVALID, "bad sizes"), "features": (INVALID, "65536"), "deferred": (UNSUPPORTED, "deferred searches"),
    "deferred+point": (UNSUPPORTED, "deferred searches"), "point": (INVALID, "map point id"), "point.device": (0, ""), "camera": (INVALID, "camera index"),
    "camera.negative": (INVALID, "camera index"), "camera.null_point": (0, ""), "octave": (INVALID, "octave"), "octave.device": (0, ""),
    "polynomial": (INVALID, "polynomial"),
}


def test_argument_checks_without_a_device(tmp_path):
    """csrc/mcs_poseopt_guard.hip alone, through tests/cpp/poseopt_guard_driver.cpp, compiled by hipcc in host-only mode (as tests/test_window_guards_cpu.py does)"""
    exe = tmp_path / "poseopt_guard_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "poseopt_guard_driver.cpp"),
                           os.path.join(CSRC, "mcs_poseopt_guard.hip"), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, rc, text = line.split("\t")
        out[name] = (int(rc), text)
    assert sorted(out) == sorted(GUARDS)
    for name, (rc, text) in GUARDS.items():
        assert out[name][0] == rc and text in out[name][1], (name, out[name])


def test_facade_driver_compiles_and_links(pkg, tmp_path):
    exe = tmp_path / "facade_driver_poseopt"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_poseopt.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 2       # no arguments: the usage exit, before anything touches a device
