"""No GPU: tests/lba_model.py (cOptimizer::LocalBundleAdjustment restated, src/cOptimizer.cpp:461-874) on its own terms — the Jacobians against a central
difference, the Schur solve against numpy.linalg.solve on the full system, every quirk of DESIGN 7 on a scene that fails when the model "repairs" it, the
list-building of the model and of the frontend on stand-in objects, the struct layout, and the argument checks of mcs_local_bundle_adjustment through
tests/cpp/lba_guard_driver.cpp (host logic only).

Jacobian agreement, measured on the scenes below: largest |analytic - central difference| 3.2e-05 (poses, where entries reach 1e5 pixels per unit of
Cayley parameter) and 3.8e-07 (points) with h = 1e-6; the bound asserted is 10 x the truncation + rounding estimate (see the test)."""
import ctypes as C
import importlib
import os
import subprocess

import numpy as np
import pytest

import lba_model as LM
import lba_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multicol-slam_amd", "csrc")


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("multicol-slam_amd")


def test_jacobians_against_a_central_difference():
    """d e / d pose and d e / d point by the chain rule against (e(x + h) - e(x - h)) / 2h; the difference is bounded by h^2/6 |e'''| + eps |e| / h, |e'''|
    estimated from third differences (step 1e-3), |e| <= 1e3 px.  Asserted with a 10x margin over that estimate."""
    h, g = 1e-6, 1e-3
    worst = [0.0, 0.0]
    for name in ("window", "twice"):
        pr = S.build(name)
        ept, ok = pr.edge_point()
        idx = np.nonzero(ok)[0]
        _, Jp, Jl = LM.evaluate(pr, pr.kf_pose, pr.pos, idx, ept)

        def res(dpose, dpos):
            return LM.evaluate(pr, pr.kf_pose + dpose, pr.pos + dpos, idx, ept, jac=False)

        for which, J, width in ((0, Jp, 6), (1, Jl, 3)):
            for k in range(width):
                d = np.zeros((1, width))
                d[0, k] = 1.0
                step = (lambda s: (s * d, 0.0)) if which == 0 else (lambda s: (0.0, s * d))      # every keyframe (every point) moves: an edge sees its own
                num = (res(*step(h)) - res(*step(-h))) / (2 * h)
                third = (res(*step(2 * g)) - 2 * res(*step(g)) + 2 * res(*step(-g)) - res(*step(-2 * g))) / (2 * g ** 3)
                est = h * h / 6 * np.abs(third).max() + 2.2e-16 * 1e3 / h
                diff = float(np.abs(J[:, :, k] - num).max())
                worst[which] = max(worst[which], diff)
                assert diff <= 10 * est, (name, which, k, diff, est)
        assert np.abs(Jp).max() > 100.0 and np.abs(Jl).max() > 10.0
        assert np.array_equal(Jp[:, :, 3:6], -Jl)        # dp/dt = -dp/dX
    print("jacobians: worst |analytic - numeric| pose %.3g point %.3g" % tuple(worst))


def _system(name):
    pr = S.build(name)
    ept, ok = pr.edge_point()
    idx = np.nonzero(ok)[0]
    e, Jp, Jl = LM.evaluate(pr, pr.kf_pose, pr.pos, idx, ept)
    fidx = np.full(pr.n_kfs, -1, np.int32)
    free = np.nonzero(pr.kf_fixed == 0)[0]
    fidx[free] = np.arange(len(free))
    w = pr.inv_sigma2[pr.octave[idx]]
    return LM.build_system(pr, fidx, ept, idx, e, Jp, Jl, w)


@pytest.mark.parametrize("name", ["window", "twice", "split", "hub"])
def test_schur_solve_equals_the_full_system(name):
    """an identity: marginalising the points and back-substituting solves the (6F + 3P) system"""
    s = _system(name)
    for lam in (1e-3, 10.0):
        ok, xp, xl = LM.schur_solve(s, lam)
        H, b = LM.full_system(s, lam)
        x = np.linalg.solve(H, b)
        got = np.concatenate([xp.reshape(-1), xl.reshape(-1)])
        assert ok and np.abs(got - x).max() <= 1e-9 * np.abs(x).max(), (name, lam, np.abs(got - x).max() / np.abs(x).max())
        okr, xpr, xlr = LM.schur_solve(s, lam, reverse=True)
        assert okr and np.abs(xpr - xp).max() <= 1e-9 * np.abs(x).max()


def test_eigen_inverse_and_ldlt():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(5, 3, 3))
    A = A @ np.transpose(A, (0, 2, 1)) + 0.1 * np.eye(3)
    assert np.abs(LM.eigen_inv3(A) @ A - np.eye(3)).max() < 1e-12
    B = rng.normal(size=(12, 12))
    B = B @ B.T + 1e-3 * np.eye(12)
    b = rng.normal(size=12)
    ok, x = LM.ldlt(B, b)
    assert ok and np.allclose(B @ x, b, rtol=1e-9, atol=1e-9)
    B[3, 3] = -1.0                                        # LDL^T, not Cholesky: a negative pivot is no failure
    assert LM.ldlt(B, b)[0] and np.allclose(B @ LM.ldlt(B, b)[1], b, rtol=1e-7, atol=1e-7)
    assert LM.ldlt(np.zeros((6, 6)), np.ones(6))[0] is False
    B[0, 0] = np.nan
    assert LM.ldlt(B, b)[0] is False


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_decisions_are_off_their_edges(name):
    """what lets the GPU tests compare decisions exactly, in index order and in reversed order"""
    m, r = S.model(name), S.model(name, reverse=True)
    assert m.margin >= LM.MARGIN and r.margin >= LM.MARGIN and m.status == 0 and m.failed_solves == 0
    assert m.iters == r.iters and m.stop == r.stop and np.array_equal(m.trials, r.trials) and np.array_equal(m.edge_state, r.edge_state)
    assert 0.0 < 100 * S.spread(name) <= 1e-6


# ---------------------------------------------------------------------------------------------- the quirks, each on a scene that shows it
def test_quirk1_the_callers_flag_is_written_and_nothing_is_written_back():
    pr = S.build("split")
    flag = [False]
    m = LM.optimize(pr, stop_flag=flag)
    assert m.status == LM.LBA_STOPPED and flag == [True] and m.stop[0] == LM.STOP_GAIN and m.iters[1] == 0
    assert np.array_equal(m.kf_pose, pr.kf_pose) and np.array_equal(m.pos, pr.pos) and not m.edge_state.any() and (m.pt_state == LM.PT_KEPT).all()
    flag = [False]
    fixed = LM.optimize(pr, stop_flag=flag, fix={"own_flag"})              # repaired: the action keeps to its own flag
    assert fixed.status == LM.LBA_OK and flag == [False] and not np.array_equal(fixed.kf_pose, pr.kf_pose)
    null = LM.optimize(pr)                                                 # NULL: the call that optimises; round two is dead (4l quirk 2)
    assert null.status == LM.LBA_OK and null.stop == [LM.STOP_GAIN, LM.STOP_NOT_RUN] and np.array_equal(null.kf_pose, fixed.kf_pose)
    assert LM.optimize(pr, stop_flag=[True]).status == LM.LBA_STOPPED      # :739


class KF:
    def __init__(self, mnId, bad=False):
        self.mnId, self.bad, self.neigh, self.matches = mnId, bad, [], []
        self.pose_min = np.full(6, 0.01 * mnId)
        self.keypoint_to_cam, self.keys = [], []

    def isBad(self):
        return self.bad

    def GetVectorCovisibleKeyFrames(self):
        return self.neigh

    def GetMapPointMatches(self):
        return self.matches

    def GetKeyPoint(self, i):
        return self.keys[i]


class MP:
    def __init__(self, mnId, bad=False):
        self.mnId, self.bad, self.obs, self.pos = mnId, bad, {}, np.array([1.0, 2.0, 3.0 + mnId])

    def isBad(self):
        return self.bad

    def GetObservations(self):
        return self.obs

    def GetWorldPos(self):
        return self.pos


def observe(kf, mp, cam=0, octave=1):
    kf.matches.append(mp)
    kf.keys.append(dict(x=10.0 + len(kf.keys), y=20.0, octave=octave))
    kf.keypoint_to_cam.append(cam)
    mp.obs.setdefault(kf, []).append(len(kf.matches) - 1)


def little_map(ids, current, neighbours, extra=()):
    kfs = {i: KF(i) for i in list(ids) + list(extra)}
    kfs[current].neigh = [kfs[i] for i in neighbours]
    return kfs


def test_quirk2_one_fixed_reflects_the_last_local_keyframe(pkg):
    cams, Mc = S.rig(2)
    fe = importlib.import_module("multicol-slam_amd.frontend")
    sig = np.ones(8)
    # keyframe 0 in the middle of the local list, no fixed camera: 0 is fixed where it stands AND the fallback fixes the first local keyframe
    kfs = little_map([5, 0, 3], 5, [0, 3])
    mp = MP(0)
    for k in (5, 0, 3):
        observe(kfs[k], mp)
    pr, local, fixed, pts, feat = LM.build_problem(kfs[5], Mc, cams, sig)
    assert [k.mnId for k in local] == [5, 0, 3] and not fixed and pr.kf_fixed.tolist() == [1, 1, 0]
    assert pr.edge_kf.tolist() == [1, 2, 0]               # the edges of a point: keyframes in ascending mnId (0, 3, 5)
    # keyframe 0 last: oneFixed is true at the end, no fallback
    kfs = little_map([5, 3, 0], 5, [3, 0])
    mp = MP(0)
    for k in (5, 3, 0):
        observe(kfs[k], mp)
    assert LM.build_problem(kfs[5], Mc, cams, sig)[0].kf_fixed.tolist() == [0, 0, 1]
    # a fixed camera exists: no fallback; a bad neighbour is marked local (:484), so it is neither local nor fixed, and its observation gives no edge
    kfs = little_map([5, 3, 4], 5, [3, 4], extra=[7, 8])
    kfs[4].bad = True
    kfs[8].bad = True
    mp, mq = MP(0), MP(1, bad=True)
    for k in (5, 3, 4, 7, 8):
        observe(kfs[k], mp)
    observe(kfs[5], mq)
    observe(kfs[5], mp, cam=1)                            # the point at a second feature of keyframe 5
    pr, local, fixed, pts, feat = LM.build_problem(kfs[5], Mc, cams, sig)
    assert [k.mnId for k in local] == [5, 3] and [k.mnId for k in fixed] == [7] and pts == [mp] and pr.kf_fixed.tolist() == [0, 0, 1]
    assert pr.edge_kf.tolist() == [1, 0, 0, 2] and feat.tolist() == [0, 0, 2, 0] and pr.edge_cam.tolist() == [0, 0, 1, 0]
    assert pr.total_obs.tolist() == [6] and pr.bad_obs.tolist() == [2]
    # the frontend builds the same lists
    l2, p2, f2, fx = fe._lba_lists(kfs[5])
    assert l2 == local and p2 == pts and f2 == fixed and fx.tolist() == pr.kf_fixed.tolist()
    kfs = little_map([5], 5, [])
    assert LM.optimize(LM.build_problem(kfs[5], Mc, cams, sig)[0]).status == LM.LBA_TOO_FEW      # quirk 6 (:489)


def _shield_scene():
    """point 0 has three edges and three observations; its first two keys, at the fixed keyframes, are gross outliers that no position reconciles"""
    pr = S.make(3, [0, 0, 1, 1], 2, [[2, 3, 0]] + [[0, 1, 2, 3]] * 12, nr=2)
    pr.xy[0] += (300.0, -200.0)
    pr.xy[1] += (-250.0, 300.0)
    return pr


def test_quirk3_an_erasure_shields_the_edges_behind_it():
    pr = _shield_scene()
    m = LM.optimize(pr)
    assert m.status == 0 and m.edge_state[:3].tolist() == [1, 1, 0] and m.pt_state[0] == LM.PT_BAD and m.margin >= LM.MARGIN
    pr.xy[2] += 300.0                                     # the third key is a gross outlier too, but it lies behind the erasure that made the point bad
    m = LM.optimize(pr)
    assert m.edge_state[:3].tolist() == [1, 1, 0] and m.pt_state[0] == LM.PT_BAD
    fixed = LM.optimize(pr, fix={"no_shield"})
    assert fixed.edge_state[:3].tolist() == [1, 1, 1]
    pr.total_obs = np.diff(pr.pt_first).astype(np.int32)
    pr.total_obs[0] += 2                                  # two more observations at bad keyframes: they count in EraseObservation, the point stays good
    m = LM.optimize(pr)
    assert m.edge_state[:3].tolist() == [1, 1, 1] and m.pt_state[0] == LM.PT_WRITTEN   # quirk 4: erased edges still count among the vertex's edges
    pr.bad_obs = np.zeros(pr.n_points, np.int32)
    pr.bad_obs[0] = 2                                     # ... but TotalNrObservations() skips those two: nothing is left, the point is not written
    assert LM.optimize(pr).pt_state[0] == LM.PT_KEPT


def test_quirk4_write_back_conditions():
    m = S.model("twice")
    assert m.pt_state[2] == LM.PT_KEPT and m.pt_state[3] == LM.PT_WRITTEN       # one edge: kept; seen only by fixed keyframes: optimised and written
    pr = S.build("twice")
    assert np.array_equal(m.pos[2], pr.pos[2]) and not np.array_equal(m.pos[3], pr.pos[3])
    assert LM.optimize(pr, fix={"write_all"}).pt_state[2] == LM.PT_WRITTEN
    pr.total_obs = np.diff(pr.pt_first).astype(np.int32)
    pr.bad_obs = np.zeros(pr.n_points, np.int32)
    pr.total_obs[4], pr.bad_obs[4] = 5, 4                 # TotalNrObservations() skips the observations at bad keyframes: 1 is left
    assert LM.optimize(pr).pt_state[4] == LM.PT_KEPT
    assert np.array_equal(m.kf_pose[pr.n_local:], pr.kf_pose[pr.n_local:])      # fixed cameras are not written


def test_quirk5_fail_means_no_active_edge():
    pr = S.build("pair")
    pr.pt_first[:] = 0
    m = LM.optimize(pr)
    assert m.status == LM.LBA_FAILED and np.array_equal(m.kf_pose, pr.kf_pose)
    pr = S.build("pair")
    pr.xy[:] = 1e6                                        # keys no estimate can reach: the omni model's image is bounded
    pr.total_obs = np.full(pr.n_points, 10, np.int32)     # no point goes bad, so nothing is shielded: pass one erases every edge and round two fails
    m = LM.optimize(pr)
    assert m.status == LM.LBA_FAILED and (m.edge_state == 1).all() and (m.pt_state == LM.PT_KEPT).all() and m.iters[1] == 0
    assert np.array_equal(m.pos, pr.pos) and np.array_equal(m.kf_pose, pr.kf_pose)       # the erasures stay, no pose and no position is written
    assert LM.optimize(pr, fix={"fail_goes_on"}).status == LM.LBA_OK


# ---------------------------------------------------------------------------------------------- the binding and the argument checks
def test_struct_layout_matches_the_header(pkg, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include "mcs_c.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mcs_lba_diag), '
                   'offsetof(mcs_lba_diag, iters), offsetof(mcs_lba_diag, stop), offsetof(mcs_lba_diag, trials), offsetof(mcs_lba_diag, n_free), '
                   'offsetof(mcs_lba_diag, n_edges1), offsetof(mcs_lba_diag, n_erased), offsetof(mcs_lba_diag, lambda), offsetof(mcs_lba_diag, chi2)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    D, dt = pkg._capi.LbaDiag, pkg._capi.LBA_DIAG_DTYPE
    assert got == [C.sizeof(D), D.iters.offset, D.stop.offset, D.trials.offset, D.n_free.offset, D.n_edges1.offset, D.n_erased.offset, D.lam.offset, D.chi2.offset]
    assert dt.itemsize == C.sizeof(D) and [dt.fields[k][1] for k in ("iters", "stop", "trials", "n_free", "n_edges1", "n_erased", "lam", "chi2")] == got[1:]
    assert pkg.lib().mcs_abi_version() == 10              # the entry point is additive


INVALID, CAPACITY, UNSUPPORTED = -1, -3, -4
GUARDS = {
    "valid": (0, ""), "null_ctx": (INVALID, "null"), "kind": (INVALID, "memory kind"), "negative": (INVALID, "bad sizes"), "local>kfs": (INVALID, "bad sizes"),
    "cams_0": (INVALID, "bad sizes"), "cams_33": (CAPACITY, "32 cameras"), "levels_0": (INVALID, "bad sizes"), "kfs_4097": (CAPACITY, "4096 keyframes"),
    "points": (CAPACITY, "2^20 points"), "edges": (CAPACITY, "2^22 edges"), "free_64": (0, ""), "free_65": (CAPACITY, "64 free"),
    "free_65.device": (CAPACITY, "64 free"), "deferred": (UNSUPPORTED, "deferred"), "deferred+kf": (UNSUPPORTED, "deferred"),
    "first.negative": (INVALID, "pt_first"), "first.backwards": (INVALID, "pt_first"), "first.beyond": (INVALID, "pt_first"), "first.device": (0, ""),
    "kf": (INVALID, "keyframe index"), "kf.negative": (INVALID, "keyframe index"), "kf.device": (0, ""), "camera": (INVALID, "camera index"),
    "octave": (INVALID, "octave"), "octave.device": (0, ""), "polynomial": (INVALID, "polynomial"),
}


def test_argument_checks_without_a_device(tmp_path):
    """csrc/mcs_lba_guard.hip alone, through tests/cpp/lba_guard_driver.cpp, compiled by hipcc in host-only mode (as tests/test_poseopt_cpu.py does)"""
    exe = tmp_path / "lba_guard_driver"
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-Wno-unused-function", "-I" + CSRC, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "lba_guard_driver.cpp"),
                           os.path.join(CSRC, "mcs_lba_guard.hip"), "-o", str(exe)])
    out = {}
    for line in subprocess.check_output([str(exe)]).decode().splitlines():
        name, rc, text = line.split("\t")
        out[name] = (int(rc), text)
    assert sorted(out) == sorted(GUARDS)
    for name, (rc, text) in GUARDS.items():
        assert out[name][0] == rc and text in out[name][1], (name, out[name])


def test_facade_driver_compiles_and_links(pkg, tmp_path):
    exe = tmp_path / "facade_driver_lba"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_lba.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    assert subprocess.call([str(exe)]) == 2       # no arguments: the usage exit, before anything touches a device
