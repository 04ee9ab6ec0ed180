"""-m gpu: mcs_pose_optimization on the hostile frames of tests/hostile_poseopt.py against tests/poseopt_model.py, both memory kinds.

Exact (test_gpu_poseopt.exact): status, iters, stop, trials, the outlier flags, n_inliers and the share, on every scene that hostile_poseopt.EXCUSED does not
name.  Of an excused scene: status, n_inliers, flags, share, and the fit (the residuals at the returned pose against those at the model's).

To a tolerance computed from the model at run time: pose, MtMc, MtMc_inv, lambda, chi2, each relative to max(1, |component|).  Per scene it is 100 x the
scene's own spread (the model with its edge sums in index order against reversed order, hostile_poseopt.spread), floored at the tolerance of
tests/test_gpu_poseopt.py (7.5e-11) and capped at 1e-6: a scene whose spread breaks the cap is re-seeded or excused, never given a looser bound
(tests/test_poseopt_hostile_cpu.py asserts the cap without a device).  NaN and infinities must sit in the same places with the same sign.

Host kind against device kind and a batch against each of its problems alone: bit for bit, the device's own runs.  A frame of 65 536 features against
the 65-edge frame it was made from: the same decisions and flags, the pose to the tolerance (its threads add the edges in another order).

Measured on an MI355X (largest relative difference device - model | the scene's spread):
  A.absorb           1.1e-16 | 5.2e-15    B.huber_nan        0.0e+00 | 0.0e+00    E.cayley50         6.6e-13 | 2.6e-12
  A.far10            4.2e-13 | 1.1e-13    C.levels_1         1.9e-15 | 1.3e-15    E.point_1e154      1.4e-16 | 1.9e-16
  A.far3             7.5e-13 | 8.4e-13    C.levels_max       4.9e-15 | 1.2e-15    E.point_1e200      3.9e-16 | 7.6e-16
  A.far30            3.3e-12 | 1.1e-12    C.weight_1e-300    3.8e-16 | 2.9e-16    E.point_overflow   0.0e+00 | 0.0e+00
  A.weight_negative  2.1e-11 | 5.1e-12    C.weight_1e300     1.1e-14 | 5.9e-15    E.scale_1e-6       2.5e-14 | 1.3e-14
  A.weights_zero     0.0e+00 | 0.0e+00    C.weight_1e308     0.0e+00 | 0.0e+00    E.scale_1e4        2.0e-14 | 4.3e-16
  B.huber_-1         1.4e-15 | 4.9e-16    C.weight_inf       0.0e+00 | 0.0e+00    E.scale_1e8        5.3e-16 | 7.0e-16
  B.huber_0          0.0e+00 | 0.0e+00    C.weight_nan       0.0e+00 | 0.0e+00    E.three_cameras    8.0e-16 | 1.2e-15
  B.huber_1e-3       1.7e-16 | 3.3e-16    D.axis_behind      8.1e-16 | 0.0e+00    F.late_trial       9.4e-12 | 1.6e-13
  B.huber_1e-300     1.1e-16 | 0.0e+00    D.axis_front       5.7e-23 | 4.6e-16    G.cameras32        1.8e-16 | 2.2e-16
  B.huber_1e200      0.0e+00 | 0.0e+00    D.centre           8.1e-16 | 0.0e+00    G.cap_stride       1.8e-16 | 7.3e-16
  B.huber_1e6        4.3e-16 | 2.1e-16    D.grazing          9.0e-16 | 7.2e-16    G.cap_tail         2.4e-16 | 7.3e-16
  B.huber_inf        0.0e+00 | 0.0e+00    D.stretched        8.4e-16 | 8.4e-16    G.one_camera       1.9e-15 | 5.1e-16
  A.accepted_failure 3.5e-11 | 3.2e-11
The largest are the two negative-weight scenes' 3.5e-11 and 2.1e-11, one and four times their spreads; a scene at 0.0e+00 returned its start pose and zeros.
"""
import importlib
import os
import signal
import subprocess

import numpy as np
import pytest

import hostile_poseopt as H
import poseopt_model as PM
import poseopt_scenes as S
import test_gpu_poseopt as TP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = ("pose", "MtMc", "MtMc_inv", "outlier", "diag")


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


@pytest.fixture(autouse=True)
def _time_limit():
    """every test under its own limit: a hung kernel ends the run instead of holding the machine"""
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    signal.alarm(120)
    yield
    signal.alarm(0)


def run(env, prs, device):
    got = S.run_library(env["pkg"], env["ctx"], prs, device)
    assert not isinstance(got, int), (got, env["pkg"].lib().mcs_last_error())
    return got


def tol_of(name):
    t = max(TP.tol(), 100.0 * H.spread(name))
    assert t <= 1e-6, (name, t)       # a condition, not a measurement
    return t


def difference(got, m, lam_chi=True):
    d = got["diag"]
    out = [H.rel(got["pose"], m.pose), H.rel(got["MtMc"], m.MtMc), H.rel(got["MtMc_inv"], m.MtMc_inv)]
    if lam_chi:
        out += [H.rel(d["lam"], m.lam), H.rel(d["chi2"], m.chi2)]
    return max(out)


def same_bits(a, b, what):
    for k in BITS:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)
    assert a["n_inliers"] == b["n_inliers"] and a["share"] == b["share"], what


_alone = {}


def alone(env, name, pr, device):
    """one problem in a call of its own, computed once per scene and memory kind"""
    if (name, device) not in _alone:
        _alone[name, device] = run(env, [pr], device)[0]
    return _alone[name, device]


def held_to_the_model(got, name, pr, m):
    t = tol_of(name)
    if name in H.EXCUSED:
        assert got["diag"]["status"] == m.status and got["n_inliers"] == m.n_inliers and got["share"] == m.share and np.array_equal(got["outlier"], m.outlier), name
        idx = pr.edges()
        fit = np.abs(PM.residual(pr, got["pose"], idx) - PM.residual(pr, m.pose, idx))[m.outlier[idx] == 0].max()
        assert fit <= 1e-6, (name, fit)                       # pixels: the same fit
        diff = difference(got, m, lam_chi=False)
    else:
        TP.exact(got, m, name)
        diff = difference(got, m)
    print("MEASURED %-18s %.1e | %.1e" % (name, diff, H.spread(name)))
    assert diff <= t, (name, diff, t)
    if m.status == PM.POSE_NONFINITE or name in ("A.weights_zero", "B.huber_0", "D.axis_behind", "D.centre"):
        assert got["pose"].tobytes() == pr.pose0.tobytes(), name            # not a bit of the pose moved


@pytest.mark.parametrize("name", sorted(H.SCENES))
def test_scene_equals_the_model_in_both_kinds(env, name):
    pr, m = H.build(name), H.model(name)
    if name not in H.EXCUSED:
        assert m.margin >= PM.MARGIN
    dev = alone(env, name, pr, True)
    held_to_the_model(dev, name, pr, m)
    same_bits(alone(env, name, pr, False), dev, name)         # the host-kind guards admit every scene of the table


def test_every_matrix_of_the_32_camera_rig(env):
    pr, m = H.build("G.cameras32"), H.model("G.cameras32")
    t = tol_of("G.cameras32")
    for device in (False, True):
        got = alone(env, "G.cameras32", pr, device)
        assert got["MtMc"].shape == got["MtMc_inv"].shape == (32, 4, 4)
        for c in range(32):
            assert H.rel(got["MtMc"][c], m.MtMc[c]) <= t and H.rel(got["MtMc_inv"][c], m.MtMc_inv[c]) <= t, c
            assert np.array_equal(got["MtMc"][c][3], [0, 0, 0, 1]) and np.abs(got["MtMc"][c][:3, :3]).max() > 0.1


def test_frames_at_the_feature_cap(env):
    """65 536 features, 65 edges: in the last 512 indices, and at multiples of 512 (one thread owns every edge, so the sums are added in another order than the
    source frame's: held to the model like any scene above, and the flags land on the features that hold the edges)"""
    src = S.scene(0, 65, 2, n_outliers=5)
    ref = run(env, [src], True)[0]
    for name in ("G.cap_tail", "G.cap_stride"):
        pr = H.build(name)
        got = alone(env, name, pr, True)
        at = pr.edges()
        assert len(got["outlier"]) == H.MAX_FEATURES and np.array_equal(got["outlier"][at], ref["outlier"]) and got["outlier"].sum() == ref["outlier"].sum()
        assert got["n_inliers"] == ref["n_inliers"] and got["diag"]["iters"].tolist() == ref["diag"]["iters"].tolist()
        assert H.rel(got["pose"], ref["pose"]) <= tol_of(name)


@pytest.mark.parametrize("device", [False, True])
def test_every_huber_multiplier_in_one_call(env, device):
    """one value per problem beside two controls at 1: each problem is its own single-problem run, bit for bit, and the model's"""
    batch = H.huber_batch()
    got = run(env, [p for _, p in batch], device)
    control = alone(env, "control1", H.base(1), device)
    for (name, p), g in zip(batch, got):
        if name == "control":
            same_bits(g, control, name)
            TP.exact(g, S.model("e65"), name)                 # hostile_poseopt.base(1) is poseopt_scenes' e65
        else:
            same_bits(g, alone(env, name, p, device), name)
            TP.exact(g, H.model(name), name)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("n", H.BATCH_SIZES)
def test_a_hostile_workgroup_does_not_disturb_its_neighbours(env, n, device):
    """calls of 64, 65, 128 and 129 problems (one launch, one and a problem, two, two and a problem) that interleave hostile scenes with controls: every
    problem equals its own single-problem run bit for bit"""
    batch = H.interleaved(n)
    got = run(env, [p for _, p in batch], device)
    assert len(got) == n
    statuses = set()
    for k, ((name, p), g) in enumerate(zip(batch, got)):
        key = name or "control%d" % (1 if (k // 2) % 2 == 0 else 4)
        same_bits(g, alone(env, key, p, device), (n, k, key))
        statuses.add(int(g["diag"]["status"]))
        if name is None:
            assert g["diag"]["status"] == 0 and g["n_inliers"] > 50, (n, k)
    assert statuses == {0, 1}


@pytest.mark.parametrize("device", [False, True])
def test_hostile_level_weights_beside_controls_in_one_call(env, device):
    """129 problems under one level table that holds a negative, a 1e-300 and a 1e300 weight; the controls' edges avoid those levels.  Every problem equals
    its own single-problem run bit for bit, and the model's (test_poseopt_hostile_cpu.py asserts the margins of the six distinct problems)"""
    batch = H.weight_interleaved(129)
    got = run(env, [p for _, p in batch], device)
    for k, ((kind, p), g) in enumerate(zip(batch, got)):
        same_bits(g, alone(env, "weights." + kind, p, device), (k, kind))
        if kind not in _weight_models:
            _weight_models[kind] = PM.optimize(p)
        TP.exact(g, _weight_models[kind], kind)
    assert sum(kind.startswith("control") for kind, _ in batch) == 65 and len(_weight_models) == 6


_weight_models = {}


# ---------------------------------------------------------------------------------------------- the layers above the C ABI clean nothing up
LAYERS = ("A.weight_negative", "B.huber_0")


@pytest.mark.parametrize("name", LAYERS)
def test_frontend_passes_the_hostile_frame_through(env, name):
    import test_gpu_poseopt_facade as TF
    FE = importlib.import_module("multicol-slam_amd.frontend")
    pr = H.build(name)
    for device in (False, True):
        raw = alone(env, name, pr, device)
        F = TF.Frame(env["pkg"], pr)
        res, diag = FE.PoseOptimizationBatch([F], dict(pos=pr.pos), [pr.huber], device=device, ctx=env["ctx"], diag=True)
        assert res[0] == (raw["n_inliers"], raw["share"]) and diag[0].tobytes() == raw["diag"].tobytes()
        assert np.array_equal(np.array(F.mvbOutlier, np.uint8), raw["outlier"])
        assert F.camSystem.GetPoseMin().tobytes() == raw["pose"].tobytes()
        assert np.stack(F.camSystem.MtMc).tobytes() == raw["MtMc"].tobytes() and np.stack(F.camSystem.MtMc_inv).tobytes() == raw["MtMc_inv"].tobytes()


def test_cpp_facade_passes_the_hostile_frames_through(env, tmp_path):
    """tests/cpp/facade_driver_poseopt.cpp over a scene file per frame (the level weights are the file's, so the negative weight needs its own)"""
    import test_io_formats as T
    exe = tmp_path / "facade_driver_poseopt"
    lib_dir = os.path.join(ROOT, "multicol-slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "facade_driver_poseopt.cpp"), "-o", str(exe), "-L" + lib_dir, "-lmcs_hip", "-Wl,-rpath," + lib_dir])
    for name in LAYERS:
        p = H.build(name)
        nr = len(p.Mc_min)
        calib = tmp_path / ("calib_" + name)
        calib.mkdir()
        T.write_lafida_dir(str(calib), p.cams, [list(map(float, m)) for m in p.Mc_min])
        lines = ["1", " ".join(repr(float(v)) for v in p.pose0), "%r %d" % (p.huber, p.n)]
        lines += ["%r %r %d %d %d" % (float(p.xy[i, 0]), float(p.xy[i, 1]), p.octave[i], p.cam[i], p.points[i]) for i in range(p.n)]
        lines.append(str(len(p.pos)))
        lines += [" ".join(repr(float(v)) for v in x) for x in p.pos]
        lines += [str(len(p.inv_sigma2)), " ".join(repr(float(v)) for v in p.inv_sigma2)]
        (tmp_path / (name + ".txt")).write_text("\n".join(lines) + "\n")
        out = subprocess.run([str(exe), str(calib), str(tmp_path / (name + ".txt"))], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        rows = out.stdout.splitlines()
        assert len(rows) == 6
        raw = alone(env, name, p, False)
        for half in range(2):                      # the call per frame, then the batched call
            a, b, c = rows[3 * half:3 * half + 3]
            head = a.split()
            assert int(head[0]) == raw["n_inliers"] == H.model(name).n_inliers and float.fromhex(head[1]) == raw["share"]
            assert np.array([float.fromhex(v) for v in head[2:]]).tobytes() == raw["pose"].tobytes(), (name, half)
            assert b == "".join(str(int(v)) for v in raw["outlier"])
            assert np.array([float.fromhex(v) for v in c.split()]).reshape(nr, 4, 4).tobytes() == raw["MtMc_inv"].tobytes()


def test_nan_weight_and_nan_multiplier_are_a_status(env):
    """DESIGN 7, the first evaluation's screen.  Before it covered the weight, the Huber pair and the sums, both ran twenty iterations to status 0 and the
    device's lambda (fmax drops a NaN) was not the model's."""
    for name in ("C.weight_nan", "B.huber_nan", "C.weight_inf", "B.huber_inf", "C.weight_1e308", "B.huber_1e200"):
        pr = H.build(name)
        for device in (False, True):
            got = alone(env, name, pr, device)
            d = got["diag"]
            assert d["status"] == PM.POSE_NONFINITE and d["iters"].tolist() == [0, 0] and d["lam"] == 0.0 and d["chi2"] == 0.0, name
            assert got["n_inliers"] == 65 and got["share"] == 0.0 and not got["outlier"].any() and got["pose"].tobytes() == pr.pose0.tobytes(), name
