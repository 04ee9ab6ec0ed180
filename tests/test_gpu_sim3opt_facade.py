"""-m gpu: cOptimizer::OptimizeSim3 through the two surfaces above the C ABI — frontend.OptimizeSim3 / OptimizeSim3Batch (host and device kind) and
MultiColSLAM::cOptimizer::OptimizeSim3 of include/mcs/mcs_facade.hpp (tests/cpp/facade_driver_sim3opt.cpp) — on keyframe stand-ins, against the raw call (bit
for bit: the same device arithmetic) and against the model (tests/sim3opt_model.py; decisions exact, S12 to the bound of tests/test_gpu_sim3opt.py).  The
stand-ins hold entries every pointer test of the reference drops, a permuted keyframe 2, and cameras stored so that only the reference's crossed lookups and
its GetSigma2 weight reproduce the problem; vpMatches1 is nulled in place."""
import importlib
import os
import signal
import subprocess

import numpy as np
import pytest

import sim3opt_scenes as S
import test_gpu_sim3opt as TS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


@pytest.fixture(autouse=True)
def _time_limit():
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(180)
    yield
    signal.alarm(0)


def stand_ins(pkg, pr):
    FE = importlib.import_module("multicol-slam_amd.frontend")
    make_rig = lambda Mt: FE.cMultiCamSys_([FE.cCamModelGeneral_.from_dict(c) for c in pr.cams], list(pr.Mc), Mt)
    return S.keyframes(pr, make_rig, pkg._capi.KP_DTYPE)


def nulled(matches, at, drop, keep):
    """vpMatches1 afterwards is what it was, minus the correspondences whose keep byte is 0"""
    want = [True] * len(matches)
    for i in drop[:1]:
        want[i] = False                                    # the entry that was NULL to begin with
    for k, i in zip(keep, at):
        want[i] = bool(k)
    return [m is not None for m in matches] == want


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["nbad", "n65", "return0", "dead_round_two"])
def test_frontend_equals_the_raw_call_and_the_model(env, name, device):
    FE = importlib.import_module("multicol-slam_amd.frontend")
    pr, m = S.build(name), S.model(name)
    kf1, kf2, matches, at, drop = stand_ins(env["pkg"], pr)
    g = FE.Sim3(pr.R12, pr.t12, pr.s12)
    ret = FE.OptimizeSim3(kf1, kf2, matches, g, pr.std_sim, device=device, ctx=env["ctx"])
    raw = S.run_library(env["pkg"], env["ctx"], [pr], device)[0]
    assert ret == raw["n_inliers"] == m.n_inliers and nulled(matches, at, drop, raw["keep"]) and np.array_equal(raw["keep"], m.keep)
    if name == "return0":
        assert g.q is None and np.array_equal(g.R, pr.R12) and np.array_equal(g.t, pr.t12) and g.s == pr.s12 and raw["keep"].sum() < 3   # not written back
    else:
        assert np.array_equal(np.concatenate([g.q, g.t, [g.s]]), raw["S12"]) and np.array_equal(g.R, raw["R12"])
        assert TS.rel(raw["S12"], m.S12, 1.0) <= S.bound()


def test_frontend_batch(env):
    FE = importlib.import_module("multicol-slam_amd.frontend")
    names = ["nbad", "return0", "n63"]                     # three cameras each
    prs = [S.build(n) for n in names]
    rigsys = stand_ins(env["pkg"], prs[0])[0].camSystem
    problems = [dict(Xw=p.Xw, cam=p.cam, obs=p.obs, w=p.w, Mt_inv=p.Mt_inv, R12=p.R12, t12=p.t12, s12=p.s12, std_sim=p.std_sim) for p in prs]
    res, diag = FE.OptimizeSim3Batch(problems, rigsys, device=True, ctx=env["ctx"], diag=True)
    raw = S.run_library(env["pkg"], env["ctx"], prs, True)
    for i, n in enumerate(names):
        m = S.model(n)
        assert res[i]["n_inliers"] == m.n_inliers and np.array_equal(res[i]["keep"], m.keep) and diag[i]["iters"].tolist() == m.iters, n
        assert np.array_equal(res[i]["S12"], raw[i]["S12"]) and np.array_equal(res[i]["R12"], raw[i]["R12"]), n
    assert FE.OptimizeSim3Batch([], rigsys, ctx=env["ctx"]) == []


@pytest.mark.parametrize("name", ["nbad", "n63", "return0"])
def test_cpp_facade_equals_the_raw_call(env, name, tmp_path):
    import test_io_formats as T
    pkg = env["pkg"]
    exe = tmp_path / "facade_driver_sim3opt"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_sim3opt.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    pr = S.build(name)
    kf1, kf2, matches, at, drop = stand_ins(pkg, pr)
    calib = tmp_path / "calib"
    calib.mkdir()
    T.write_lafida_dir(str(calib), pr.cams, T.CAYLEY)
    num = lambda a: " ".join(repr(float(v)) for v in np.asarray(a, np.float64).reshape(-1))
    lines = [num(pr.Mt[0]), num(pr.Mt[1]), num(pr.R12) + " " + num(pr.t12) + " %r %r" % (pr.s12, pr.std_sim), str(len(pr.sigma2)), num(kf1.mvLevelSigma2),
             num(kf1.mvInvLevelSigma2)]
    for kf in (kf1, kf2):
        lines.append(str(len(kf.mvKeys)))
        lines += ["%r %r %d %d" % (float(k["x"]), float(k["y"]), k["octave"], c) for k, c in zip(kf.mvKeys, kf.keypoint_to_cam)]
    for mp1, mp2 in zip(kf1.mvpMapPoints, matches):
        lines.append("%s %d %d %s %d" % (num(np.zeros(3) if mp1 is None else mp1.X), 2 if mp1 is None else mp1.bad, -2 if mp2 is None else mp2.idx, num(np.zeros(3) if mp2 is None else mp2.X), 0 if mp2 is None else mp2.bad))
    (tmp_path / "scene.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(calib), str(tmp_path / "scene.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.splitlines()
    raw = S.run_library(pkg, env["ctx"], [pr], False)[0]
    assert int(rows[0]) == raw["n_inliers"] == S.model(name).n_inliers
    vals = np.array([float.fromhex(v) for v in rows[1].split()])
    if name == "return0":
        assert np.array_equal(vals[4:7], pr.t12) and vals[7] == pr.s12 and np.array_equal(vals[8:].reshape(3, 3), pr.R12)
    else:
        assert np.array_equal(vals[:8], raw["S12"]) and np.array_equal(vals[8:].reshape(3, 3), raw["R12"])
    assert nulled([None if c == "0" else 1 for c in rows[2]], at, drop, raw["keep"])
