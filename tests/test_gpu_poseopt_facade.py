"""-m gpu: cOptimizer::PoseOptimization through the two surfaces above the C ABI — frontend.PoseOptimization / PoseOptimizationBatch (host and device kind)
and MultiColSLAM::cOptimizer::PoseOptimization of include/mcs/mcs_facade.hpp (tests/cpp/facade_driver_poseopt.cpp) — against the raw call (bit for bit: the
same device arithmetic) and against the model (tests/poseopt_model.py; decisions exact, pose to the tolerance of tests/test_gpu_poseopt.py)."""
import importlib
import os
import signal
import subprocess

import numpy as np
import pytest

import poseopt_model as PM
import poseopt_scenes as S
import test_gpu_poseopt as TP

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


class Frame:
    """what frontend.PoseOptimization reads of a cMultiFrame"""

    def __init__(self, pkg, pr):
        FE = importlib.import_module("multicol-slam_amd.frontend")
        io = importlib.import_module("multicol-slam_amd.io")
        self.mvKeys = S.keys_of(pr, pkg._capi)
        self.keypoint_to_cam = pr.cam.astype(np.int32)
        self.mvpMapPoints = [None if p < 0 else int(p) for p in pr.points]
        self.mvbOutlier = [True] * pr.n
        self.mvInvLevelSigma2 = list(pr.inv_sigma2)
        self.camSystem = FE.cMultiCamSys_([FE.cCamModelGeneral_.from_dict(c) for c in pr.cams], [io.cayley2hom(m) for m in pr.Mc_min])
        self.camSystem.M_c_min = [np.array(m) for m in pr.Mc_min]
        self.camSystem.Set_M_t_from_min(pr.pose0)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", ["e65", "round_two_runs", "e1025"])
def test_frontend_equals_the_raw_call_and_the_model(env, name, device):
    FE = importlib.import_module("multicol-slam_amd.frontend")
    pr, m = S.build(name), S.model(name)
    F = Frame(env["pkg"], pr)
    assert np.array_equal(F.camSystem.MtMc_inv, PM.rig_from_min(pr.pose0, pr.Mc_min)[1])      # Set_M_t_from_min on the host, as the model builds it
    nin, share = FE.PoseOptimization(F, dict(pos=pr.pos), pr.huber, device=device, ctx=env["ctx"])
    raw = S.run_library(env["pkg"], env["ctx"], [pr], device)[0]
    assert nin == raw["n_inliers"] == m.n_inliers and share == raw["share"] == m.share
    assert np.array_equal(np.array(F.mvbOutlier, np.uint8), raw["outlier"]) and np.array_equal(raw["outlier"], m.outlier)
    assert np.array_equal(F.camSystem.GetPoseMin(), raw["pose"]) and np.array_equal(np.stack(F.camSystem.MtMc_inv), raw["MtMc_inv"])
    assert np.array_equal(np.stack(F.camSystem.MtMc), raw["MtMc"])
    assert np.abs(F.camSystem.GetPoseMin() - m.pose).max() <= TP.tol()


def test_frontend_batch(env):
    FE = importlib.import_module("multicol-slam_amd.frontend")
    names = ["e64", "e8", "dead_round_two"]       # three cameras each
    prs = [S.build(n) for n in names]
    frames = [Frame(env["pkg"], p) for p in prs]
    base = np.cumsum([0] + [len(p.pos) for p in prs])
    for F, b in zip(frames, base):
        F.mvpMapPoints = [None if p is None else p + int(b) for p in F.mvpMapPoints]
    res, diag = FE.PoseOptimizationBatch(frames, dict(pos=np.concatenate([p.pos for p in prs])), [p.huber for p in prs], device=True, ctx=env["ctx"], diag=True)
    for i, n in enumerate(names):
        m = S.model(n)
        assert res[i] == (m.n_inliers, m.share) and diag[i]["iters"].tolist() == m.iters and np.array_equal(np.array(frames[i].mvbOutlier, np.uint8), m.outlier), n
        assert np.abs(frames[i].camSystem.GetPoseMin() - m.pose).max() <= TP.tol()
    assert FE.PoseOptimizationBatch([], dict(pos=np.zeros((0, 3))), ctx=env["ctx"]) == []


def test_cpp_facade_equals_the_raw_call(env, tmp_path):
    import test_io_formats as T
    pkg = env["pkg"]
    exe = tmp_path / "facade_driver_poseopt"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_poseopt.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    names = ["e64", "e8", "round_two_runs"]
    prs = [S.build(n) for n in names]
    calib = tmp_path / "calib"
    calib.mkdir()
    T.write_lafida_dir(str(calib), prs[0].cams, T.CAYLEY)
    base = np.cumsum([0] + [len(p.pos) for p in prs])
    lines = [str(len(prs))]
    for p, b in zip(prs, base):
        lines.append(" ".join(repr(float(v)) for v in p.pose0))
        lines.append("%r %d" % (p.huber, p.n))
        for i in range(p.n):
            lines.append("%r %r %d %d %d" % (float(p.xy[i, 0]), float(p.xy[i, 1]), p.octave[i], p.cam[i], -1 if p.points[i] < 0 else p.points[i] + b))
    pos = np.concatenate([p.pos for p in prs])
    lines.append(str(len(pos)))
    lines += [" ".join(repr(float(v)) for v in x) for x in pos]
    lines.append(str(len(prs[0].inv_sigma2)))
    lines.append(" ".join(repr(float(v)) for v in prs[0].inv_sigma2))
    (tmp_path / "scene.txt").write_text("\n".join(lines) + "\n")
    out = subprocess.run([str(exe), str(calib), str(tmp_path / "scene.txt")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.splitlines()
    assert len(rows) == 6 * len(prs)
    raw = S.run_library(pkg, env["ctx"], prs, False)
    for half in range(2):                      # one call per frame, then the batched call
        for i, p in enumerate(prs):
            a, b, c = rows[3 * (half * len(prs) + i):3 * (half * len(prs) + i) + 3]
            head = a.split()
            assert int(head[0]) == raw[i]["n_inliers"] == S.model(names[i]).n_inliers and float.fromhex(head[1]) == raw[i]["share"]
            assert np.array_equal(np.array([float.fromhex(v) for v in head[2:]]), raw[i]["pose"]), (half, i)
            assert b == "".join(str(int(v)) for v in raw[i]["outlier"])
            assert np.array_equal(np.array([float.fromhex(v) for v in c.split()]).reshape(3, 4, 4), raw[i]["MtMc_inv"])
