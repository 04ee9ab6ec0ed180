"""-m gpu: mcs_local_bundle_adjustment (cOptimizer::LocalBundleAdjustment, src/cOptimizer.cpp:461-874) against tests/lba_model.py, both memory kinds, the scenes of
tests/lba_scenes.py: pair, window, slow, twice, split, hub (72 edges on one point), long_row (1025 edges at one keyframe), cap (64 free keyframes).

Exact: status, iterations, trials, stop reasons, the erasure counts, edge_state and pt_state — on every scene, each of which keeps every decision of its model
run at least lba_model.MARGIN from its edge (asserted here again).

To a measured tolerance: poses, points, kf_t, lambda, chi2.  For each scene the model runs with its sums in index order and in reversed order; the largest
difference of a final pose component or point coordinate is the scene's spread (model, x86-64: 8e-15 .. 7e-14 on the small scenes, 4.8e-13 on cap, 1.5e-11
on long_row).  The device may differ from the model by TOL = 100 x the largest spread on a pose component, point coordinate or kf_t entry, and relatively on
lambda and chi2.  TOL is computed from the model at run time (1.5e-9 with these seeds) and may never exceed 1e-6 (a condition, not a measurement).
Measured on an MI355X, the same in both kinds: pose 1.8e-14 (cap), 6.3e-15 (long_row), at most 2.6e-15 elsewhere; point 1.1e-11 (long_row), 4.0e-13 (cap), at
most 6.0e-14 elsewhere; lambda 2.7e-11 relative (split), 1.1e-11 (twice), at most 3.1e-15 elsewhere; chi2 at most 5.7e-13 relative.

The same call twice is bit-identical; 65 free keyframes are refused with nothing written; the caller's stop flag is written by the optimiser and then nothing
is written back; the device-kind outputs feed mcs_covis_set_keyframe_pose and mcs_covis_update_points where they lie."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import lba_model as LM
import lba_scenes as S

pytestmark = pytest.mark.gpu
NAMES = list(S.SCENES)


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


def exact(got, m, name):
    d = got["diag"]
    assert got["status"] == m.status, (name, got["status"], m.status)
    assert d["iters"].tolist() == m.iters and d["stop"].tolist() == m.stop and np.array_equal(d["trials"], m.trials), (name, d, m.iters, m.stop, m.trials)
    assert d["n_free"] == m.n_free and d["n_edges1"] == m.n_edges1 and d["n_erased"].tolist() == m.n_erased, (name, d, m.n_erased)
    assert np.array_equal(got["edge_state"], m.edge_state) and np.array_equal(got["pt_state"], m.pt_state), name


def close(got, m, name, n_local):
    t = tol()
    dp, dx = float(np.abs(got["kf_pose"] - m.kf_pose).max()), float(np.abs(got["pos"] - m.pos).max())
    d = got["diag"]
    print("%s: |pose| %.3g |pos| %.3g lambda %.3g chi2 %.3g (tol %.3g)" % (name, dp, dx, abs(d["lam"] - m.lam) / max(abs(m.lam), 1.0),
                                                                           abs(d["chi2"] - m.chi2) / max(abs(m.chi2), 1.0), t))
    assert dp <= t and dx <= t, (name, dp, dx, t)
    assert np.abs(got["kf_t"] - m.kf_pose[:n_local, 3:6]).max() <= t, name
    assert abs(d["lam"] - m.lam) <= t * max(abs(m.lam), 1.0) and abs(d["chi2"] - m.chi2) <= t * max(abs(m.chi2), 1.0), (name, d["lam"], m.lam, d["chi2"], m.chi2)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_scene_equals_the_model(env, name, device):
    m = S.model(name)
    assert m.margin >= LM.MARGIN and m.status == LM.LBA_OK       # else: re-seed the scene (tools/lba_seed_search.py), never loosen this
    pr = S.build(name)
    got = S.run_library(env["pkg"], env["ctx"], pr, device)
    exact(got, m, name)
    close(got, m, name, pr.n_local)
    assert np.array_equal(got["kf_pose"][pr.n_local:], pr.kf_pose[pr.n_local:])            # a fixed camera is never written
    kept = got["pt_state"] != LM.PT_WRITTEN
    assert np.array_equal(got["pos"][kept], pr.pos[kept])


def test_scene_shapes():
    """the shapes the scenes are there for"""
    hub, row, cap, tw = S.build("hub"), S.build("long_row"), S.build("cap"), S.build("twice")
    assert np.diff(hub.pt_first).max() == 72 and (row.edge_kf == 0).sum() == 1025 and (cap.kf_fixed == 0).sum() == 64
    assert np.diff(tw.pt_first)[2] == 1 and tw.kf_fixed[tw.edge_kf[tw.pt_first[3]:tw.pt_first[4]]].all()
    assert len(set(tw.edge_kf[tw.pt_first[0]:tw.pt_first[1]].tolist())) < np.diff(tw.pt_first)[0]
    assert S.model("slow").stop[0] == LM.STOP_ITERATIONS and S.model("slow").iters[1] >= 2 and S.model("window").n_erased[0] >= 6


@pytest.mark.parametrize("device", [False, True])
def test_the_same_call_twice_is_bit_identical(env, device):
    for name in ("window", "hub"):
        pr = S.build(name)
        a, b = S.run_library(env["pkg"], env["ctx"], pr, device), S.run_library(env["pkg"], env["ctx"], pr, device)
        for k in ("kf_pose", "kf_t", "pos", "edge_state", "pt_state"):
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert a["diag"].tobytes() == b["diag"].tobytes(), name


def test_host_and_device_kind_agree_bit_for_bit(env):
    pr = S.build("window")
    a, b = S.run_library(env["pkg"], env["ctx"], pr, False), S.run_library(env["pkg"], env["ctx"], pr, True)
    for k in ("kf_pose", "kf_t", "pos", "edge_state", "pt_state"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_65_free_keyframes_are_refused_with_nothing_written(env):
    pkg = env["pkg"]
    cap, L = pkg._capi, pkg.lib()
    pr = S.chain(65)
    for device in (False, True):
        assert S.run_library(pkg, env["ctx"], pr, device) == cap.MCS_ERR_CAPACITY
        assert b"64 free" in L.mcs_last_error()
    # host kind, straight through the C ABI, every output preset
    pose, pos = pr.kf_pose.copy(), pr.pos.copy()
    es, ps, t = np.full(pr.n_edges, 7, np.uint8), np.full(pr.n_points, 7, np.uint8), np.full((pr.n_local, 3), 7.0)
    dg = cap.LbaDiag()
    dg.status = 77
    ocs = (cap.Ocam * len(pr.cams))(*[cap.make_ocam(c) for c in pr.cams])
    p = cap.np_ptr
    keys = S.keys_of(pr, cap)
    rc = L.mcs_local_bundle_adjustment(env["ctx"].h, pr.n_kfs, pr.n_local, p(pose), p(pr.kf_fixed), p(t), pr.n_points, p(pos), p(pr.pt_first), pr.n_edges,
                                       p(pr.edge_kf), p(pr.edge_cam), p(keys), None, None, p(np.ascontiguousarray(pr.Mc_min)), ocs, len(pr.cams),
                                       p(pr.inv_sigma2), len(pr.inv_sigma2), 2.0, None, cap.MEM_HOST, p(es), p(ps), C.byref(dg))
    assert rc == cap.MCS_ERR_CAPACITY and dg.status == 77
    assert np.array_equal(pose, pr.kf_pose) and np.array_equal(pos, pr.pos) and (es == 7).all() and (ps == 7).all() and (t == 7.0).all()


@pytest.mark.parametrize("device", [False, True])
def test_the_callers_flag_is_written_and_then_nothing_is_written_back(env, device):
    """quirk 1: round one of "split" ends on the gain test; with a flag given the action writes it and the reference writes nothing back"""
    pr = S.build("split")
    m = S.model("split", flag=False)
    assert m.status == LM.LBA_STOPPED and m.flag_out and S.model("split").stop[0] == LM.STOP_GAIN and m.margin >= LM.MARGIN
    flag = [False]
    got = S.run_library(env["pkg"], env["ctx"], pr, device, flag=flag)
    assert got["status"] == LM.LBA_STOPPED and flag == [True] and got["stop_flag"] is True
    d = got["diag"]
    assert d["iters"].tolist() == m.iters and d["stop"].tolist() == m.stop and np.array_equal(d["trials"], m.trials)
    assert np.array_equal(got["kf_pose"], pr.kf_pose) and np.array_equal(got["pos"], pr.pos) and not got["edge_state"].any() and (got["pt_state"] == 1).all()
    assert not got["kf_t"].any()
    # the same scene without a flag optimises (the action's own flag; round two runs no iteration)
    free = S.run_library(env["pkg"], env["ctx"], pr, device)
    assert free["status"] == LM.LBA_OK and free["diag"]["iters"].tolist()[1] == 0 and np.abs(free["kf_pose"] - pr.kf_pose).max() > 1e-6
    # a flag that is set on entry: nothing runs (:739)
    got = S.run_library(env["pkg"], env["ctx"], pr, device, flag=[True])
    assert got["status"] == LM.LBA_STOPPED and got["diag"]["iters"].tolist() == [0, 0] and np.array_equal(got["pos"], pr.pos)
    # a flag on a scene whose first round uses its 10 iterations is never written; the result is the NULL call's
    slow = S.build("slow")
    flag = [False]
    got = S.run_library(env["pkg"], env["ctx"], slow, device, flag=flag)
    ms = S.model("slow", flag=False)
    exact(got, ms, "slow with a flag")
    assert got["stop_flag"] == ms.flag_out


@pytest.mark.parametrize("device", [False, True])
def test_statuses_that_write_nothing(env, device):
    pkg, ctx = env["pkg"], env["ctx"]
    pr = S.build("pair")
    pr.pos[3, 1] = np.nan
    got = S.run_library(pkg, ctx, pr, device)
    assert got["status"] == LM.LBA_NONFINITE == LM.optimize(pr).status and np.array_equal(got["pos"], pr.pos, equal_nan=True)
    assert np.array_equal(got["kf_pose"], pr.kf_pose) and not got["edge_state"].any()
    pr = S.build("pair")
    pr.kf_fixed[:] = 1
    assert S.run_library(pkg, ctx, pr, device)["status"] == LM.LBA_NO_FREE_POSE == LM.optimize(pr).status
    pr = S.build("pair")
    pr.n_local = 1
    assert S.run_library(pkg, ctx, pr, device)["status"] == LM.LBA_TOO_FEW == LM.optimize(pr).status
    pr = S.build("pair")
    pr.pt_first[:] = 0                                   # no edge at all: optimize() returns Fail (quirk 5)
    got = S.run_library(pkg, ctx, pr, device)
    assert got["status"] == LM.LBA_FAILED == LM.optimize(pr).status and np.array_equal(got["kf_pose"], pr.kf_pose)


@pytest.mark.parametrize("device", [False, True])
def test_round_two_fails_after_pass_one_erased_every_edge(env, device):
    """quirk 5: keys no estimate can reach and points that never go bad — pass one erases every edge, optimize() of round two returns Fail: the erasures are
    reported, no pose and no position is written"""
    pr = S.build("pair")
    pr.xy[:] = 1e6
    pr.total_obs = np.full(pr.n_points, 10, np.int32)
    m = LM.optimize(pr)
    assert m.status == LM.LBA_FAILED and (m.edge_state == 1).all()
    got = S.run_library(env["pkg"], env["ctx"], pr, device)
    exact(got, m, "fail")
    assert np.array_equal(got["kf_pose"], pr.kf_pose) and np.array_equal(got["pos"], pr.pos) and not got["kf_t"].any()
    pr.total_obs = None                                  # quirk 3 on the same keys: the first erasure makes each point bad and shields its second edge
    m = LM.optimize(pr)
    got = S.run_library(env["pkg"], env["ctx"], pr, device)
    assert m.status == LM.LBA_OK and m.edge_state.tolist() == [1, 0] * pr.n_points and (m.pt_state == LM.PT_BAD).all()
    assert got["status"] == m.status and np.array_equal(got["edge_state"], m.edge_state) and np.array_equal(got["pt_state"], m.pt_state)
    assert got["diag"]["n_erased"].tolist() == m.n_erased


def test_guards(env):
    """a keyframe index, camera or octave out of range: no edge in device kind, MCS_ERR_INVALID in host kind; a pt_first that runs backwards likewise"""
    pkg, cap = env["pkg"], env["pkg"]._capi
    for k in range(4):
        pr = S.build("window")
        if k == 0:
            pr.edge_kf[5] = pr.n_kfs
        elif k == 1:
            pr.edge_cam[17] = -1
        elif k == 2:
            pr.octave[40] = len(pr.inv_sigma2)
        else:
            pr.pt_first[-1] = pr.pt_first[-2] - 1        # the last point's range runs backwards: it has no edge
        m = LM.optimize(pr)
        got = S.run_library(pkg, env["ctx"], pr, True)
        assert got["status"] == m.status == 0 and got["diag"]["n_edges1"] == m.n_edges1 < pr.n_edges
        if m.margin >= LM.MARGIN:
            assert np.array_equal(got["edge_state"], m.edge_state) and np.abs(got["kf_pose"] - m.kf_pose).max() <= tol()
        assert S.run_library(pkg, env["ctx"], pr, False) == cap.MCS_ERR_INVALID
        assert (b"keyframe index", b"camera", b"octave", b"pt_first")[k] in pkg.lib().mcs_last_error()


def test_refused_while_deferred_searches_are_on(env):
    pkg, ctx = env["pkg"], env["ctx"]
    L = pkg.lib()
    pkg.check(L.mcs_ctx_set_async_search(ctx.h, 1))
    try:
        assert S.run_library(pkg, ctx, S.build("pair"), True) == pkg._capi.MCS_ERR_UNSUPPORTED
    finally:
        pkg.check(L.mcs_ctx_set_async_search(ctx.h, 0))


def test_outputs_feed_the_covisibility_store_where_they_lie(env):
    """the device-kind call's kf_t and pos go into mcs_covis_set_keyframe_pose and mcs_covis_update_points as device pointers, nothing copied to the host in
    between; equal, bit for bit, to the same two calls fed from the host-kind result"""
    pkg, ctx = env["pkg"], env["ctx"]
    FE = importlib.import_module("multicol-slam_amd.frontend")
    cap, L = pkg._capi, pkg.lib()
    pr = S.build("window")
    P, nl = pr.n_points, pr.n_local
    rows = [[int(p) for p in range(P) if k in pr.edge_kf[pr.pt_first[p]:pr.pt_first[p + 1]]] for k in range(pr.n_kfs)]
    sf = 1.2 ** np.arange(8)
    ids, ref = np.arange(P, dtype=np.int32), np.array([int(pr.edge_kf[pr.pt_first[p]]) for p in range(P)], np.int64)
    mn = np.arange(nl, dtype=np.int64)

    def refresh(t_ptr, pos_ptr, kind, mem):
        store = FE.cCovisibility(16, 128, P, ctx=ctx)
        for k in range(pr.n_kfs):
            store.SetKeyFrame(k, rows[k])
        o = {k: mem.put(np.zeros((P, 3)) if k == "normal" else np.zeros(P)) for k in ("normal", "min_dist", "max_dist")}
        o["status"] = mem.put(np.full(P, -1, np.int32))
        a = [mem.put(ids), mem.put(ref), mem.put(sf)]
        pkg.check(L.mcs_covis_set_keyframe_pose(store.h, nl, cap.np_ptr(mn), t_ptr, kind))
        pkg.check(L.mcs_covis_update_points(store.h, P, mem.ptr(a[0]), pos_ptr, mem.ptr(a[1]), mem.ptr(a[2]), len(sf), kind, mem.ptr(o["normal"]),
                                            mem.ptr(o["min_dist"]), mem.ptr(o["max_dist"]), None, None, None, None, None, None, None, mem.ptr(o["status"])))
        return {k: mem.read(v) for k, v in o.items()}

    dev = S.run_library(pkg, ctx, pr, True)
    got = refresh(dev["arrays"]["t"].ptr, dev["arrays"]["pos"].ptr, cap.MEM_DEVICE, FE._DEVICE)
    hst = S.run_library(pkg, ctx, pr, False)
    want = refresh(cap.np_ptr(np.ascontiguousarray(hst["kf_t"])), cap.np_ptr(np.ascontiguousarray(hst["pos"])), cap.MEM_HOST, FE._HOST)
    assert (got["status"] == 0).all()
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
