"""-m gpu: mcs_optimize_essential_graph (cOptimizer::OptimizeEssentialGraph, src/cOptimizerLoopStuff.cpp:267-513) against tests/essgraph_model.py, both memory
kinds, the scenes of tests/essgraph_scenes.py: chain6, dup (a pair with two edges), isolated (a vertex without an edge: its block is lambda I), fixed_mid
(the fixed vertex is not first), scale (s of 0.93 and 1.07, rotations beyond the small-angle branch: all four branches of log), panels (77 unknowns: two
full solver panels and one of 13), big (150 keyframes, two loops: 1043 unknowns), identity (nothing to correct, every residual exactly 0).

Exact: status, iterations, stop reason, trials and n_free — on every scene, each of which keeps every decision of its model run (the sign of rho, the gain
against 1e-6, every branch of exp and log, every quaternion-conversion case, every LU pivot choice) at least its essgraph_scenes.MARGIN from its edge in all ten
runs of the spread (asserted here again; identity decides on exact zeros instead).

To a DERIVED tolerance: Scw_out, pose, kf_t, pos, lambda, chi2.  The device differs from the model through ocml's acos / sin / cos / exp / log and through the
order of its sums, and the numeric Jacobian divides such differences by 2e-9.  For every scene the model also runs with its edge sums and the solve's inner
sums reversed and under eight seeds that move every transcendental by the OpenCL full-profile ulp bounds (no figure for ocml's own FP64 functions was at
hand); the largest relative spread over the scenes is the model's own uncertainty and the device may differ by TWICE that (DESIGN.md 4m's rule).  TOL is
computed from the model at run time and may never exceed 1e-4 (a condition, not a measurement).
Model, x86-64: spread 6.9e-6 (chain6), 5.4e-7 (dup), 3.1e-5 (isolated), 6.3e-8 (fixed_mid), 1.1e-5 (scale), 1.1e-7 (panels), 1.1e-5 (big): TOL = 6.2e-5.
Measured on an MI355X, the same in both kinds, largest relative difference of an output / lambda / chi2: chain6, isolated, identity 0 (equal to the bit),
dup 0 / 0 / 1.4e-16, fixed_mid 2.4e-8 / 0 / 3.0e-9, scale 1.9e-7 / 7.8e-6 / 5.8e-9, panels 1.1e-9 / 0 / 1.2e-10, big 1.2e-8 / 0 / 1.6e-8.

Also: the same call twice is bit-identical; host and device kind give the same bytes; 513 free vertices are refused with nothing written; every guard and
every status that writes nothing; the device-kind kf_t and pos feed mcs_covis_set_keyframe_pose and mcs_covis_update_points where they lie."""
import ctypes as C
import importlib
import signal

import numpy as np
import pytest

import essgraph_model as M
import essgraph_scenes as S

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
        t = 2.0 * max(S.spread(n)[0] for n in NAMES if n != "identity")   # identity decides on exact zeros: a moved exp(0) is another scene
        assert 0.0 < t <= 1e-4, t
        _tol.append(t)
    return _tol[0]


def exact(got, m, name):
    d = got["diag"]
    assert got["status"] == m.status, (name, got["status"], m.status)
    assert (int(d["iters"]), int(d["stop"]), d["trials"].tolist(), int(d["n_free"]), int(d["n_edges"])) == (m.iters, m.stop, m.trials, m.n_free, m.n_edges), (name, d, m.iters, m.stop, m.trials)


def close(got, m, name):
    t = tol()
    diff = {k: S.rel(got[k], getattr(m, k)) for k in S.FIELDS}
    d = got["diag"]
    diff["lam"] = abs(d["lam"] - m.lam) / max(abs(m.lam), 1e-300)
    diff["chi2"] = abs(d["chi2"] - m.chi2) / max(abs(m.chi2), 1e-300)
    print("%s: %s (tol %.3g)" % (name, " ".join("%s %.3g" % kv for kv in diff.items()), t))
    assert max(diff.values()) <= t, (name, diff, t)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_scene_equals_the_model(env, name, device):
    m = S.model(name)
    assert m.status == M.EG_OK
    pr = S.build(name)
    if name == "identity":
        assert m.chi2 == 0.0 and (m.iters, m.stop, m.trials[0]) == (1, M.STOP_TRIALS, 1)
    else:
        spread, margin, same = S.spread(name)
        assert same and margin >= 1.0 and spread <= S.MAX_SPREAD, (name, margin, spread)   # else: re-seed the scene (tools/essgraph_seed_search.py), never loosen this
    got = S.run_library(env["pkg"], env["ctx"], pr, device)
    exact(got, m, name)
    close(got, m, name)
    untouched = pr.pt_ref < 0
    assert untouched.any() and np.array_equal(got["pos"][untouched], pr.pos[untouched])
    if name == "identity":                                       # every output equals its input's conversion, to the bit
        assert np.array_equal(got["Scw_out"], pr.Scw) and np.array_equal(got["pose"], m.pose) and np.array_equal(got["kf_t"], -pr.Scw[:, 4:7])
        assert np.array_equal(got["pos"], m.pos) and np.abs(got["pos"] - pr.pos).max() <= 1e-14   # (X + t) - t: no transcendental, two roundings
    else:
        fx = pr.fixed != 0
        assert np.array_equal(got["Scw_out"][fx], pr.Scw[fx]) and np.abs(got["Scw_out"][~fx] - pr.Scw[~fx]).max() > 1e-6


def test_scene_shapes():
    """the shapes the scenes are there for"""
    d, iso, fm, pn, bg = (S.build(n) for n in ("dup", "isolated", "fixed_mid", "panels", "big"))
    pairs = list(zip(d.edge_i.tolist(), d.edge_j.tolist()))
    assert pairs.count((5, 0)) == 2 and sorted(d.edge_kind[[k for k, p in enumerate(pairs) if p == (5, 0)]].tolist()) == [0, 1]
    assert 3 not in iso.edge_i and 3 not in iso.edge_j and not iso.fixed[3]
    assert fm.fixed.tolist().index(1) == 3
    n = 7 * int((pn.fixed == 0).sum())
    assert n > 2 * M.PANEL and n % M.PANEL != 0
    assert len(bg.Scw) == 150 and (bg.edge_kind == 0).sum() == 3 and 7 * 149 > M.kExactSolve
    assert S.model("scale").branches == {0, 1, 2, 3} and len(S.model("scale").pivots | S.model("big").pivots) > 1
    assert S.model("isolated").stop == M.STOP_CAP and S.model("isolated").iters == 16


@pytest.mark.parametrize("device", [False, True])
def test_the_same_call_twice_is_bit_identical(env, device):
    for name in ("scale", "panels", "big"):
        pr = S.build(name)
        a, b = S.run_library(env["pkg"], env["ctx"], pr, device), S.run_library(env["pkg"], env["ctx"], pr, device)
        for k in S.FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert a["diag"].tobytes() == b["diag"].tobytes(), name


def test_host_and_device_kind_agree_bit_for_bit(env):
    for name in ("dup", "panels"):
        pr = S.build(name)
        a, b = S.run_library(env["pkg"], env["ctx"], pr, False), S.run_library(env["pkg"], env["ctx"], pr, True)
        for k in S.FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), (name, k)
        assert a["diag"].tobytes() == b["diag"].tobytes(), name


def star(n_free):
    """n_free free vertices, each tied to one fixed vertex by one edge"""
    K = n_free + 1
    Scw = np.zeros((K, 8))
    Scw[:, 3] = Scw[:, 7] = 1.0
    Scw[:, 4] = np.arange(K)
    fixed = np.zeros(K, np.uint8)
    fixed[0] = 1
    return M.Problem(Scw, Scw, np.zeros(K, np.uint8), fixed, np.arange(1, K), np.zeros(n_free, int), np.ones(n_free, np.uint8), np.ones((3, 3)), [0, 1, -1])


def test_513_free_vertices_are_refused_with_nothing_written(env):
    pkg = env["pkg"]
    cap, L = pkg._capi, pkg.lib()
    pr = star(513)
    for device in (False, True):
        assert S.run_library(pkg, env["ctx"], pr, device) == cap.MCS_ERR_CAPACITY
        assert b"512 free" in L.mcs_last_error()
    K = len(pr.Scw)
    out, pose, t, pos = np.full((K, 8), 7.0), np.full((K, 16), 7.0), np.full((K, 3), 7.0), pr.pos.copy()
    dg = cap.EgDiag()
    dg.status = 77
    p = cap.np_ptr
    rc = L.mcs_optimize_essential_graph(env["ctx"].h, K, p(pr.Scw), p(pr.Snc), p(pr.has_nc), p(pr.fixed), len(pr.edge_i), p(pr.edge_i), p(pr.edge_j),
                                        p(pr.edge_kind), len(pos), p(pos), p(pr.pt_ref), cap.MEM_HOST, p(out), p(pose), p(t), C.byref(dg))
    assert rc == cap.MCS_ERR_CAPACITY and dg.status == 77
    assert (out == 7.0).all() and (pose == 7.0).all() and (t == 7.0).all() and np.array_equal(pos, pr.pos)


@pytest.mark.parametrize("device", [False, True])
def test_statuses_that_write_nothing(env, device):
    pkg, ctx = env["pkg"], env["ctx"]

    def nothing(got, pr):
        return np.array_equal(got["pos"], pr.pos) and not got["Scw_out"].any() and not got["pose"].any() and not got["kf_t"].any()

    pr = S.build("chain6")
    pr.Scw[2, 5] = np.nan
    got = S.run_library(pkg, ctx, pr, device)
    assert got["status"] == M.EG_NONFINITE == M.optimize(pr).status and nothing(got, pr)
    pr = S.build("chain6")
    pr.fixed[:] = 1
    got = S.run_library(pkg, ctx, pr, device)
    assert got["status"] == M.EG_NO_FREE_VERTEX == M.optimize(pr).status and nothing(got, pr)
    pr = S.build("chain6")
    pr.edge_i, pr.edge_j, pr.edge_kind = pr.edge_i[:0], pr.edge_j[:0], pr.edge_kind[:0]
    got = S.run_library(pkg, ctx, pr, device)
    assert got["status"] == M.EG_FAILED == M.optimize(pr).status and nothing(got, pr) and got["diag"]["iters"] == 0


def test_guards(env):
    """an edge with an index out of range or with both ends at one vertex, a pt_ref out of range: nothing from it in device kind, MCS_ERR_INVALID in host kind"""
    pkg, cap = env["pkg"], env["pkg"]._capi
    for k in range(4):
        pr = S.build("fixed_mid")
        if k == 0:
            pr.edge_i[4] = len(pr.Scw)
        elif k == 1:
            pr.edge_j[9] = -1
        elif k == 2:
            pr.edge_j[6] = pr.edge_i[6]
        else:
            pr.pt_ref[5] = len(pr.Scw)
        m = M.optimize(pr)
        got = S.run_library(pkg, env["ctx"], pr, True)
        assert got["status"] == m.status == 0 and got["diag"]["n_edges"] == m.n_edges == len(pr.edge_i) - (k < 3)
        assert np.array_equal(got["pos"][pr.pt_ref == len(pr.Scw)], pr.pos[pr.pt_ref == len(pr.Scw)])
        if k == 3:                                               # the edges are the scene's: its decisions hold
            exact(got, m, "guard")
            close(got, m, "guard")
        assert S.run_library(pkg, env["ctx"], pr, False) == cap.MCS_ERR_INVALID
        assert (b"edge vertex", b"edge vertex", b"with itself", b"pt_ref")[k] in pkg.lib().mcs_last_error()
    # an edge that is refused in device kind leaves no edge at all: optimize() returns Fail
    pr = star(1)
    pr.edge_j[0] = 5
    assert S.run_library(pkg, env["ctx"], pr, True)["status"] == M.EG_FAILED == M.optimize(pr).status


def test_refused_while_deferred_searches_are_on(env):
    pkg, ctx = env["pkg"], env["ctx"]
    L = pkg.lib()
    pkg.check(L.mcs_ctx_set_async_search(ctx.h, 1))
    try:
        assert S.run_library(pkg, ctx, S.build("chain6"), True) == pkg._capi.MCS_ERR_UNSUPPORTED
    finally:
        pkg.check(L.mcs_ctx_set_async_search(ctx.h, 0))


def test_outputs_feed_the_covisibility_store_where_they_lie(env):
    """the device-kind call's kf_t and pos go into mcs_covis_set_keyframe_pose and mcs_covis_update_points as device pointers, nothing copied to the host in
    between; equal, bit for bit, to the same two calls fed from the host-kind result"""
    pkg, ctx = env["pkg"], env["ctx"]
    FE = importlib.import_module("multicol-slam_amd.frontend")
    cap, L = pkg._capi, pkg.lib()
    pr = S.build("fixed_mid")
    K, P = len(pr.Scw), len(pr.pos)
    ref = np.where(pr.pt_ref < 0, 0, pr.pt_ref).astype(np.int64)
    rows = [[int(p) for p in range(P) if ref[p] == k or (ref[p] + 1) % K == k] for k in range(K)]
    sf = 1.2 ** np.arange(8)
    ids, mn = np.arange(P, dtype=np.int32), np.arange(K, dtype=np.int64)

    def refresh(t_ptr, pos_ptr, kind, mem):
        store = FE.cCovisibility(16, 128, P, ctx=ctx)
        for k in range(K):
            store.SetKeyFrame(k, rows[k])
        o = {k: mem.put(np.zeros((P, 3)) if k == "normal" else np.zeros(P)) for k in ("normal", "min_dist", "max_dist")}
        o["status"] = mem.put(np.full(P, -1, np.int32))
        a = [mem.put(ids), mem.put(ref), mem.put(sf)]
        pkg.check(L.mcs_covis_set_keyframe_pose(store.h, K, cap.np_ptr(mn), t_ptr, kind))
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
