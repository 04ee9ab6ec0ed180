"""-m gpu: mcs_pose_optimization (cOptimizer::PoseOptimization, src/cOptimizer.cpp:259-459) against tests/poseopt_model.py, both memory kinds, rigs of 2 and 3
Lafida cameras, the scenes of tests/poseopt_scenes.py.

Exact: status, iters, trials and stop of the diagnostics, the outlier flags, n_inliers and the share — on every scene whose model run keeps each decision at
least poseopt_model.MARGIN from its edge (asserted here again).  The one-edge scene cannot (a perfect fit: chi2 -> 0 and the late decisions are rounding
noise); of it only the status, the count, the flag and the fit itself are compared.

To a measured tolerance: pose, MtMc, MtMc_inv, lambda, chi2.  For each scene the model runs with its edge sums in index order and in reversed order; the
largest difference of the final pose is the scene's spread.  Measured (model, x86-64): 0 .. 2.3e-16 on the well-posed scenes, 7.5e-13 on "e3" (three edges on
one point: H has rank 2 and the pose drifts along the null space with whatever lambda * I lets through).  The device may differ from the model by TOL = 100 x
the largest spread = 7.5e-11 on a pose component or matrix entry, and relatively on lambda and chi2; the margin covers summation order, ocml's atan against
libm's and the pow of the lambda update.  Measured on an MI355X: 6.6e-12 on "e3", 4.6e-13 on "e2", 1.6e-13 on "e1", at most 2.1e-16 everywhere else.
TOL is computed from the model at run time and may never exceed 1e-6 (a condition, not a measurement).

A batch of 65 / 0 / 1025 edges against each problem alone, and 70 problems against the first launch's 64 + 6: bit for bit, both the device's own runs."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import poseopt_model as PM
import poseopt_scenes as S

pytestmark = pytest.mark.gpu
NAMES = list(S.SIZES) + list(S.QUIRKS)


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


_tol = []


def tol():
    if not _tol:
        t = 100.0 * max(S.spread(n) for n in NAMES)
        assert 0.0 < t <= 1e-6, t
        _tol.append(t)
    return _tol[0]


def close(got, m, name):
    t = tol()
    assert np.abs(got["pose"] - m.pose).max() <= t, (name, float(np.abs(got["pose"] - m.pose).max()), t)
    assert np.abs(got["MtMc"] - m.MtMc).max() <= t and np.abs(got["MtMc_inv"] - m.MtMc_inv).max() <= t, name
    d = got["diag"]
    assert abs(d["lam"] - m.lam) <= t * max(abs(m.lam), 1.0) and abs(d["chi2"] - m.chi2) <= t * max(abs(m.chi2), 1.0), (name, d["lam"], m.lam, d["chi2"], m.chi2)


def exact(got, m, name):
    d = got["diag"]
    assert d["status"] == m.status, name
    assert d["iters"].tolist() == m.iters and d["stop"].tolist() == m.stop and np.array_equal(d["trials"], m.trials), (name, d, m.iters, m.stop, m.trials)
    assert np.array_equal(got["outlier"], m.outlier) and got["n_inliers"] == m.n_inliers and got["share"] == m.share, name


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", [n for n in NAMES if n != "e1"])
def test_scene_equals_the_model(env, name, device):
    m = S.model(name)
    assert m.margin >= PM.MARGIN       # else: re-seed the scene (tools/poseopt_seed_search.py), never loosen this
    got = S.run_library(env["pkg"], env["ctx"], [S.build(name)], device)[0]
    exact(got, m, name)
    close(got, m, name)


@pytest.mark.parametrize("device", [False, True])
def test_one_edge(env, device):
    """rank 2 of 6 and a perfect fit: the key is reproduced, the edge is an inlier, the pose moved; no decision of the late iterations is compared"""
    pr, m = S.build("e1"), S.model("e1")
    got = S.run_library(env["pkg"], env["ctx"], [pr], device)[0]
    assert got["diag"]["status"] == 0 and got["n_inliers"] == 1 == m.n_inliers and got["outlier"].tolist() == [0] and got["share"] == 0.0
    assert np.isfinite(got["pose"]).all() and np.abs(got["pose"] - pr.pose0).max() > 1e-4
    assert np.abs(PM.residual(pr, got["pose"], pr.edges())).max() < 1e-6
    close(got, m, "e1")


@pytest.mark.parametrize("device", [False, True])
def test_batch_equals_each_problem_alone_bit_for_bit(env, device):
    prs = [S.build("e65"), S.scene(3, 0, 2, n_null=7), S.scene(0, 1025, 2, n_outliers=100, n_null=200)]
    both = S.run_library(env["pkg"], env["ctx"], prs, device)
    assert [len(p.edges()) for p in prs] == [65, 0, 1025]
    for i, p in enumerate(prs):
        alone = S.run_library(env["pkg"], env["ctx"], [p], device)[0]
        for k in ("pose", "MtMc", "MtMc_inv", "outlier", "diag"):
            assert np.asarray(both[i][k]).tobytes() == np.asarray(alone[k]).tobytes(), (i, k)
        assert both[i]["n_inliers"] == alone["n_inliers"] and both[i]["share"] == alone["share"]
    assert both[0]["n_inliers"] == S.model("e65").n_inliers


def test_more_problems_than_one_launch_takes(env):
    """70 problems: launches of 64 and 6; place and launch do not show"""
    base = [S.build("e8"), S.build("e2"), S.build("e64")]       # three cameras each
    prs = [base[i % 3] for i in range(70)]
    got = S.run_library(env["pkg"], env["ctx"], prs, True)
    alone = [S.run_library(env["pkg"], env["ctx"], [p], True)[0] for p in base]
    for i, g in enumerate(got):
        for k in ("pose", "MtMc_inv", "outlier", "diag"):
            assert np.asarray(g[k]).tobytes() == np.asarray(alone[i % 3][k]).tobytes(), (i, k)


@pytest.mark.parametrize("device", [False, True])
def test_no_correspondence(env, device):
    pr = S.scene(3, 0, 3, n_null=7)
    got = S.run_library(env["pkg"], env["ctx"], [pr], device)[0]
    m = PM.optimize(pr)
    assert got["n_inliers"] == 0 and got["share"] == 0.0 and not got["outlier"].any() and got["diag"]["status"] == 0
    assert np.array_equal(got["pose"], pr.pose0) and got["diag"]["iters"].tolist() == [0, 0] and got["diag"]["stop"].tolist() == [4, 4]
    assert np.abs(got["MtMc_inv"] - m.MtMc_inv).max() <= tol()
    empty = S.scene(3, 0, 3)           # not a single feature
    got = S.run_library(env["pkg"], env["ctx"], [empty], device)[0]
    assert got["n_inliers"] == 0 and np.array_equal(got["pose"], empty.pose0)


@pytest.mark.parametrize("device", [False, True])
def test_nonfinite_input_is_a_status(env, device):
    for what in ("point", "key", "pose"):
        pr = S.build("e65")
        i = pr.edges()[3]
        if what == "point":
            pr.pos[pr.points[i]] = np.nan
        elif what == "key":
            pr.xy[i, 0] = np.inf
        else:
            pr.pose0[4] = np.nan
        got = S.run_library(env["pkg"], env["ctx"], [pr], device)[0]
        assert got["diag"]["status"] == PM.POSE_NONFINITE and got["n_inliers"] == 65 and got["share"] == 0.0 and not got["outlier"].any(), what
        assert np.array_equal(got["pose"], pr.pose0, equal_nan=True) and got["diag"]["iters"].tolist() == [0, 0], what
        m = PM.optimize(pr)
        assert m.status == PM.POSE_NONFINITE and m.n_inliers == 65


def test_guards(env):
    """a point id >= table->n, a camera outside [0, nr_cams), an octave outside [0, nlevels): no edge in device kind, MCS_ERR_INVALID in host kind"""
    pkg, cap = env["pkg"], env["pkg"]._capi
    for k in range(4):
        pr = S.build("e65")
        a, b, c = pr.edges()[[0, 2, 4]]
        if k in (0, 3):
            pr.points[a] = len(pr.pos) + 3
        if k in (1, 3):
            pr.cam[b] = 2 if k == 1 else -1
        if k in (2, 3):
            pr.octave[c] = len(pr.inv_sigma2)
        m = PM.optimize(pr)
        assert m.margin >= PM.MARGIN
        got = S.run_library(pkg, env["ctx"], [pr], True)[0]
        assert got["n_inliers"] == m.n_inliers and np.array_equal(got["outlier"], m.outlier) and m.nInitial == 65 - (3 if k == 3 else 1)
        assert np.abs(got["pose"] - m.pose).max() <= tol()
        assert S.run_library(pkg, env["ctx"], [pr], False) == cap.MCS_ERR_INVALID
        assert (b"point id", b"camera", b"octave", b"point id")[k] in pkg.lib().mcs_last_error()


def test_refusals_and_optional_outputs(env):
    pkg, ctx = env["pkg"], env["ctx"]
    cap, L = pkg._capi, pkg.lib()
    pr = S.build("e8")
    pkg.check(L.mcs_ctx_set_async_search(ctx.h, 1))
    try:
        assert S.run_library(pkg, ctx, [pr], True) == cap.MCS_ERR_UNSUPPORTED
        assert S.run_library(pkg, ctx, [pr], False) == cap.MCS_ERR_UNSUPPORTED
    finally:
        pkg.check(L.mcs_ctx_set_async_search(ctx.h, 0))
    full = S.run_library(pkg, ctx, [pr], True)[0]
    for device in (False, True):
        bare = S.run_library(pkg, ctx, [pr], device, with_rig=False, with_diag=False)[0]
        assert np.array_equal(bare["pose"], full["pose"]) and np.array_equal(bare["outlier"], full["outlier"]) and bare["n_inliers"] == full["n_inliers"]
        assert not bare["MtMc_inv"].any() and bare["diag"]["iters"].tolist() == [0, 0]      # not written
    assert L.mcs_pose_optimization(ctx.h, 0, None, None, None, None, 0, None, 0, None, 1, *([None] * 7)) == 0


def test_huber_multiplier_per_problem(env):
    a, b = S.build("e65"), S.build("e65")
    b.huber = 4.0
    got = S.run_library(env["pkg"], env["ctx"], [a, b], True)
    mb = PM.optimize(b)
    assert mb.margin >= PM.MARGIN and not np.array_equal(mb.pose, S.model("e65").pose)
    exact(got[0], S.model("e65"), "huber 1")
    exact(got[1], mb, "huber 4")
    close(got[1], mb, "huber 4")


# ---------------------------------------------------------------------------------------------- the chain of a tracked frame on resident data
def test_search_pose_search_chain_without_a_host_visit(env):
    """mcs_search_last_frame -> mcs_pose_optimization -> mcs_search_local_points, every array in device memory: cur_points of the first call are the `points` of
    the second, whose MtMc / MtMc_inv are the rig view of the third, and nothing is read in between.  Equal, bit for bit, to the same chain with the matches and
    the pose taken through the host (host-kind optimisation, its matrices uploaded)."""
    import frustum_model as FM
    import frustum_pack as FP
    import lastframe_scene as LS
    import test_gpu_lastframe as TL
    pkg, G, ctx = env["pkg"], env["G"], env["ctx"]
    FE = importlib.import_module("multicol-slam_amd.frontend")
    cap, L = pkg._capi, pkg.lib()
    Sc = LS.make_pair(**LS.SCENES["3x401"])
    fsc = FM.make_scene(**FM.SCENES["2000"])
    cams, nr, n = Sc["rig"]["cams"], 3, Sc["cur"]["n"]
    # the rig of both scenes (frustum_model.make_rig at frame 1) in minimal form
    M_t = FM.small_motion(0.2, -0.3, 0.1, [0.01, 0.0, 0.02])
    Mc = []
    for c in range(nr):
        M = FM.rot_y(360.0 / nr * c)
        M[:3, 3] = [0.1 * np.cos(c * 2.1), 0.02 * c, 0.1 * np.sin(c * 2.1)]
        Mc.append(FE._hom2cayley(M))
    pose0, Mc = FE._hom2cayley(M_t), np.array(Mc)
    sig = 1.0 / LS.scales() ** 2
    ocs = np.frombuffer((cap.Ocam * nr)(*[cap.make_ocam(c) for c in cams]), np.uint8).copy()

    def optimise(points_ptr, device):
        mem = FE._DEVICE if device else FE._HOST
        g = {k: mem.put(v) for k, v in dict(keys=Sc["cur"]["keys"], cam=Sc["cur"]["cam"], pos=Sc["pts"]["pos"], Mc=Mc, ocs=ocs, sig=sig, hub=np.ones(1),
                                            pose=pose0.reshape(1, 6).copy(), MtMc=np.zeros((nr, 16)), inv=np.zeros((nr, 16)), out=np.zeros(n, np.uint8),
                                            nin=np.zeros(1, np.int32), share=np.zeros(1)).items()}
        fr = cap.PoseFrame(mem.ptr(g["keys"]), mem.ptr(g["cam"]), points_ptr, n)
        outs = (C.c_void_p * 1)(mem.ptr(g["out"]))
        tab = cap.PointTable(mem.ptr(g["pos"]), None, Sc["pts"]["n"])
        pkg.check(L.mcs_pose_optimization(ctx.h, 1, C.byref(fr), C.byref(tab), mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(sig), mem.ptr(g["hub"]),
                                          mem.kind, mem.ptr(g["pose"]), mem.ptr(g["MtMc"]), mem.ptr(g["inv"]), outs, mem.ptr(g["nin"]), mem.ptr(g["share"]), None))
        return g, mem

    def local_search(inv_ptr, fwd_ptr, keep):
        call = FP.Call(pkg, G, fsc, True)
        call.rig.MtMc_inv, call.rig.MtMc = inv_ptr, fwd_ptr
        call.reset()
        pkg.check(call.run(ctx, reset=False))
        return call

    # ---- resident: three calls enqueued, then the host looks
    first = TL.Call(env, Sc, True)
    pkg.check(first.run(1, ctx))
    g, mem = optimise(first.cur_points.ptr, True)
    third = local_search(g["inv"].ptr, g["MtMc"].ptr, g)
    got = third.read()
    got_pose, got_out, got_nin = mem.read(g["pose"]), mem.read(g["out"]), int(mem.read(g["nin"])[0])
    # ---- through the host
    again = TL.Call(env, Sc, True)
    pkg.check(again.run(1, ctx))
    points = again.cur_points.read()
    h, hmem = optimise(cap.np_ptr(points), False)
    up = [G.DevBuf(h["inv"]), G.DevBuf(h["MtMc"])]
    want = local_search(up[0].ptr, up[1].ptr, up).read()
    assert np.array_equal(got_pose, h["pose"]) and np.array_equal(got_out, h["out"]) and got_nin == int(h["nin"][0])
    assert got_nin >= 100 and got_out.sum() >= 5 and np.abs(got_pose - pose0).max() > 1e-7        # a real optimisation with inliers and outliers
    for k in ("match", "assigned", "visible_inc"):
        assert np.array_equal(got[k], want[k]), k
    assert got["nmatches"] == want["nmatches"] >= 100 and got["n_to_match"] == want["n_to_match"]
    for k in ("in_view", "proj_x", "proj_y", "level", "view_cos"):
        assert FP.same_doubles(got["state"][k], want["state"][k]), k
