"""-m gpu: mcs_frustum / mcs_search_local_points (cMultiFrame::isInFrustum, src/cMultiFrame.cpp:218-270, and cTracking::SearchReferencePointsInFrustum from
src/cTracking.cpp:978 on) against tests/frustum_model.py.

in_view, level, view_cos, the untouched fields, visible_inc, n_to_match: bit-equal.  proj_x / proj_y: atol 1e-9 px, more than 95 % bit-equal, identical
finiteness (atan is ocml's on the device, glibc's in the model: the rule of test_world_to_cam_matches_oracle).  match per slot, nmatches and the final
`assigned`: equal to the model's AND to the oracle's search_by_projection run on the device's own fields."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import frustum_model as M
import frustum_pack as P

pytestmark = pytest.mark.gpu

_MODEL = {}


def scene(name, desc_masks=True):
    """(scene, model output) — cached: the model takes a second per scene"""
    key = (name, desc_masks)
    if key not in _MODEL:
        sc = M.make_scene(**M.SCENES[name])
        pts, rig, st, desc, mask, F, asg = sc
        _MODEL[key] = (sc, M.search_local_points(pts, rig, st, desc, mask if desc_masks else None, F, asg))
    return _MODEL[key]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


def run(env, sc, device, search=True, desc_masks=True, **kw):
    call = P.Call(env["pkg"], env["G"], sc, device, search=search, desc_masks=desc_masks, **kw)
    env["pkg"].check(call.run(env["ctx"]))
    if device:
        env["ctx"].synchronize()
    return call.read()


def check_chain(got, want, sc, desc_masks, where):
    pts, rig, st, desc, mask, F, asg = sc
    P.compare_fields(got, want, where)
    assert np.array_equal(got["match"], want["match"]), (where, int((got["match"] != want["match"]).sum()))
    assert got["nmatches"] == want["nmatches"] and np.array_equal(got["assigned"], want["assigned"]), where
    # ... and the oracle's search on the DEVICE's own fields: a last-place difference of uv can neither cause nor hide a mismatch
    a2 = np.ascontiguousarray(asg, np.uint8).copy()
    nm, m = (0, np.full(got["match"].shape, -1, np.int32)) if got["n_to_match"] == 0 else \
        M.search_on_state(pts, got["state"], desc, mask if desc_masks else None, F, a2, 3.0, 0.8)
    assert nm == got["nmatches"] and np.array_equal(m, got["match"]) and np.array_equal(a2, got["assigned"]), where


@pytest.mark.parametrize("name", ["2000", "8000", "2000_64"])
def test_frustum_fields_match_the_model(env, name):
    sc, want = scene(name)
    M.check_scene(sc[0], sc[1], want)      # every branch and level occurs, 10 .. 90 % in view: asserted on the model's output
    got_h = run(env, sc, False, search=False)
    got_d = run(env, sc, True, search=False)
    P.compare_fields(got_h, want, name)
    for k in got_h["state"]:
        assert got_h["state"][k].tobytes() == got_d["state"][k].tobytes(), k
    assert np.array_equal(got_h["visible_inc"], got_d["visible_inc"]) and got_h["n_to_match"] == got_d["n_to_match"]


@pytest.mark.parametrize("desc_masks", [True, False])
@pytest.mark.parametrize("name", ["2000", "8000", "2000_64", "8000_64"])
def test_chain_matches_the_model_both_memory_kinds(env, name, desc_masks):
    sc, want = scene(name, desc_masks)
    assert want["nmatches"] >= 200 and want["n_to_match"] >= 500
    got_h = run(env, sc, False, desc_masks=desc_masks)
    got_d = run(env, sc, True, desc_masks=desc_masks)
    check_chain(got_h, want, sc, desc_masks, (name, "host"))
    check_chain(got_d, want, sc, desc_masks, (name, "device"))
    for k in got_h["state"]:       # identical bytes from both kinds
        assert got_h["state"][k].tobytes() == got_d["state"][k].tobytes(), k
    for k in ("match", "assigned", "visible_inc"):
        assert got_h[k].tobytes() == got_d[k].tobytes(), k
    assert (got_h["nmatches"], got_h["n_to_match"]) == (got_d["nmatches"], got_d["n_to_match"])


def test_chain_without_stream_overlap_in_a_child_process(env):
    """MCS_NO_OVERLAP=1 (read when the context is created): same outputs"""
    e = dict(os.environ, MCS_NO_OVERLAP="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_device_calls_back_to_back_share_the_scratch(env):
    """three device-kind calls of different sizes enqueued without a wait in between reuse the context's scratch in stream order"""
    calls = []
    for name in ("8000", "2000", "8000_64"):
        sc, want = scene(name)
        c = P.Call(env["pkg"], env["G"], sc, True)
        env["pkg"].check(c.run(env["ctx"]))
        calls.append((name, c, sc, want))
    env["ctx"].synchronize()
    for name, c, sc, want in calls:
        check_chain(c.read(), want, sc, True, name)


# ---------------------------------------------------------------------------------------------- the quirks
def tiny_scene():
    """one camera; map point k on the bearing ray of feature idx[k] of the frame, carrying its descriptor; every slot holds a stale flag on that feature"""
    fr = M.oracle_frames(32, 1, 300)
    F = fr[1]
    synth = importlib.import_module("multicol-slam_amd.synth")
    rig = M.make_rig(F["cams"], 1, True, synth)
    idx = np.flatnonzero(F["keys"]["octave"] <= 1)[:6]
    n = len(idx)
    pos = np.array([(rig["MtMc"][0] @ np.append(F["rays"][j] * 3.0, 1.0))[:3] for j in idx])
    st = M.new_state(n, 1)
    for k, j in enumerate(idx):
        st["in_view"][k, 0], st["proj_x"][k, 0], st["proj_y"][k, 0] = 1, float(F["keys"]["x"][j]), float(F["keys"]["y"][j])
        st["level"][k, 0], st["view_cos"][k, 0] = int(F["keys"]["octave"][j]), 1.0
    return F, rig, idx, pos, st


def tiny_points(pos, minD, maxD, flags):
    n = len(pos)
    return dict(pos=np.ascontiguousarray(pos), normal=np.tile([0.0, 0.0, 1.0], (n, 1)), min_dist=np.full(n, minD), max_dist=np.full(n, maxD),
                flags=np.array(flags, np.uint8))


@pytest.mark.parametrize("device", [False, True])
def test_stale_flags_of_a_seen_point_are_searched(env, device):
    F, rig, idx, pos, st = tiny_scene()
    n = len(idx)
    pts = tiny_points(pos, 2.9, 10.0, [0] + [M.LP_SEEN] * (n - 1))
    got = run(env, (pts, rig, st, F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8)), device)
    assert got["n_to_match"] == 1 and got["visible_inc"].tolist() == [1] + [0] * (n - 1)
    assert got["match"][:, 0].tolist() == idx.tolist() and got["nmatches"] == n     # the frustum loop alone would give one match
    assert got["assigned"][idx].all() and got["assigned"].sum() == n


@pytest.mark.parametrize("device", [False, True])
def test_nothing_is_searched_when_no_slot_came_into_view(env, device):
    F, rig, idx, pos, st = tiny_scene()
    n = len(idx)
    pts = tiny_points(pos, 50.0, 100.0, [0] + [M.LP_SEEN] * (n - 1))               # the one projected point is too near: nToMatch = 0
    got = run(env, (pts, rig, st, F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8)), device)
    assert got["n_to_match"] == 0 and got["nmatches"] == 0 and (got["match"] == -1).all() and not got["assigned"].any()
    assert got["state"]["in_view"][:, 0].tolist() == [0] + [1] * (n - 1)           # the stale flags are still set


@pytest.mark.parametrize("device", [False, True])
def test_a_bad_point_with_a_stale_flag_is_not_searched(env, device):
    F, rig, idx, pos, st = tiny_scene()
    n = len(idx)
    pts = tiny_points(pos, 2.9, 10.0, [0, M.LP_BAD, M.LP_SEEN, M.LP_BAD | M.LP_SEEN] + [0] * (n - 4))
    got = run(env, (pts, rig, st, F["desc"][idx], F["mask"][idx], F, np.zeros(F["n"], np.uint8)), device)
    want = idx.copy()
    want[[1, 3]] = -1
    assert got["match"][:, 0].tolist() == want.tolist() and got["nmatches"] == n - 2
    assert got["state"]["in_view"][[1, 3], 0].tolist() == [1, 1] and got["visible_inc"].tolist() == [1, 0, 0, 0] + [1] * (n - 4)


def test_quirk_inputs_nan_zero_distance_and_behind_the_camera(env):
    """NaN position, dist == 0, minDistance == 0, a point behind the camera inside the bounds (no mask image): fields bit-equal to the model"""
    synth = importlib.import_module("multicol-slam_amd.synth")
    F = M.oracle_frames(32, 1, 300)[1]
    rig = M.make_rig(F["cams"], 1, False, synth)
    centre = rig["MtMc"][0][:3, 3]
    front = (rig["MtMc"][0] @ np.array([0.05, 0.02, 1.0, 1.0]))[:3]
    behind = (rig["MtMc"][0] @ np.array([1.0, 0.5, -0.05, 1.0]))[:3]
    pos = np.array([front, behind, centre, [np.nan, 0.0, 1.0], front, front])
    pts = dict(pos=pos, normal=np.tile([0.0, 0.0, 1.0], (6, 1)), min_dist=np.array([0.5, 0.5, -1.0, 1.0, 0.0, np.nan]),
               max_dist=np.array([5.0, 5.0, 1.0, 2.0, 5.0, np.nan]), flags=np.zeros(6, np.uint8))
    st = M.new_state(6, 1)
    want_st, vis, ntm, fresh = M.frustum(pts, rig, F["scales"], st)
    want = dict(state=want_st, visible_inc=vis, n_to_match=ntm, fresh=fresh)
    assert fresh[1, 0] == 1 and want_st["level"][4, 0] == 7            # behind the camera yet in view; infinite ratio: the top level
    # a NaN distance with a finite projection (a NaN in MtMc only): it passes both comparisons of :241, level 0, NaN viewing cosine
    T = rig["MtMc"][0].copy()
    T[0, 3] = np.nan
    rig2 = dict(rig, MtMc=[T])
    w2, vis2, ntm2, fresh2 = M.frustum(pts, rig2, F["scales"], st)
    assert fresh2[0, 0] == 1 and w2["level"][0, 0] == 0 and np.isnan(w2["view_cos"][0, 0])
    for device in (False, True):
        got = run(env, (pts, rig, st, F["desc"][:6], F["mask"][:6], F, np.zeros(F["n"], np.uint8)), device, search=False)
        P.compare_fields(got, want, device)
        got = run(env, (pts, rig2, st, F["desc"][:6], F["mask"][:6], F, np.zeros(F["n"], np.uint8)), device, search=False)
        P.compare_fields(got, dict(state=w2, visible_inc=vis2, n_to_match=ntm2, fresh=fresh2), ("nan", device))


# ---------------------------------------------------------------------------------------------- the existing entry point, refusals, staging
def test_existing_search_by_projection_on_the_compacted_list_gives_the_same_matches(env):
    """ties the slot form to mcs_search_by_projection; the optional active / row arguments, absent there, changed nothing"""
    pkg, ctx = env["pkg"], env["ctx"]
    cap = pkg._capi
    sc, want = scene("8000")
    pts, rig, st, desc, mask, F, asg = sc
    got = run(env, sc, True)
    sl = M.searched_slots(pts, got["state"])
    ii, cc = np.array([s[0] for s in sl]), np.array([s[1] for s in sl])
    g = got["state"]
    px, py, vc = (np.ascontiguousarray(g[k][ii, cc]) for k in ("proj_x", "proj_y", "view_cos"))
    lv, pc = np.ascontiguousarray(g["level"][ii, cc], np.int32), np.ascontiguousarray(cc, np.int32)
    dd, mm = np.ascontiguousarray(desc[ii]), np.ascontiguousarray(mask[ii])
    a2 = np.ascontiguousarray(asg, np.uint8).copy()
    p = cap.np_ptr
    mp = cap.ProjectionSet(p(px), p(py), p(vc), p(lv), p(pc), p(dd), p(mm), len(ii), 32)
    sc8 = np.ascontiguousarray(F["scales"], np.float64)
    fv = cap.FrameView(p(F["keys"]), p(F["desc"]), p(F["mask"]), p(F["cam"]), p(a2), F["n"], 32, F["nr"], p(F["width"]), p(F["height"]), p(sc8), 8)
    match, nm = np.full(len(ii), -9, np.int32), np.zeros(1, np.int32)
    pkg.check(pkg.lib().mcs_search_by_projection(ctx.h, C.byref(mp), C.byref(fv), 3.0, 0.8, 32, cap.MEM_HOST, p(match), p(nm)))
    assert int(nm[0]) == got["nmatches"] and np.array_equal(match, got["match"][ii, cc]) and np.array_equal(a2, got["assigned"])
    rest = np.ones(got["match"].shape, bool)
    rest[ii, cc] = False
    assert (got["match"][rest] == -1).all()


def test_refusals_and_the_empty_call(env):
    pkg, ctx, G = env["pkg"], env["ctx"], env["G"]
    cap, L = pkg._capi, pkg.lib()
    sc, _ = scene("2000")
    c = P.Call(pkg, G, sc, False)
    # deferred searches are refused, the frustum test alone is not
    pkg.check(L.mcs_ctx_set_async_search(ctx.h, 1))
    try:
        assert c.run(ctx) == cap.MCS_ERR_UNSUPPORTED
        f = P.Call(pkg, G, sc, False, search=False)
        pkg.check(f.run(ctx))
    finally:
        pkg.check(L.mcs_ctx_set_async_search(ctx.h, 0))
    # argument errors
    keep = (c.frame.nr_cams, c.frame.nlevels, c.frame.mask, c.pts.n)
    c.frame.nr_cams = 2
    assert c.run(ctx) == cap.MCS_ERR_INVALID
    c.frame.nr_cams = keep[0]
    c.frame.nlevels = 0
    assert c.run(ctx) == cap.MCS_ERR_INVALID
    c.frame.nlevels = keep[1]
    c.frame.mask = None
    assert c.run(ctx) == cap.MCS_ERR_INVALID and b"masks" in L.mcs_last_error()
    c.frame.mask = keep[2]
    c.dim = 24
    assert c.run(ctx) == cap.MCS_ERR_INVALID and b"dim" in L.mcs_last_error()
    c.dim = 32
    c.pts.n = -1
    assert c.run(ctx) == cap.MCS_ERR_INVALID
    # a stale in-view slot of a seen point with a level outside the pyramid (host kind: refused before anything runs)
    c.pts.n = keep[3]
    seen = int(np.flatnonzero(sc[0]["flags"] == M.LP_SEEN)[0])
    c.init["in_view"][seen, 0], c.init["level"][seen, 0] = 1, 8
    assert c.run(ctx) == cap.MCS_ERR_INVALID and b"level" in L.mcs_last_error()
    c.init["level"][seen, 0] = 0
    pkg.check(c.run(ctx))
    # n = 0: a successful no-op, both kinds
    for device in (False, True):
        e = P.Call(pkg, G, sc, device)
        e.pts.n = 0
        pkg.check(e.run(ctx))
        ctx.synchronize()
        assert int(e.out["n_to_match"][1]()[0]) == 0 and int(e.out["nmatches"][1]()[0]) == 0


def test_host_kind_call_between_other_host_kind_calls_reuses_the_staging_block(env):
    """as tests/test_gpu_staging_reuse.py: on ONE context a search, the local-map chain (larger: the block regrows), a smaller search, the chain again — each
    equal to the same call on a fresh context"""
    import test_gpu_staging_reuse as R
    mcs, G = env["pkg"], env["G"]

    def chain_job(name):
        sc, _ = scene(name)

        def job(mcs_, ctx):
            c = P.Call(mcs_, G, sc, False)
            mcs_.check(c.run(ctx))
            r = c.read()
            return [r["match"], r["assigned"], r["visible_inc"], np.array([r["nmatches"], r["n_to_match"]])] + [r["state"][k] for k in sorted(r["state"])]
        return job

    jobs = [("search small", R.search_job(1, 600)), ("local map 2000", chain_job("2000")), ("window", R.window_job(3, 1500)), ("local map 8000", chain_job("8000")),
            ("search small again", R.search_job(1, 600)), ("local map 2000 again", chain_job("2000"))]
    shared = mcs.Context(0)
    got = [job(mcs, shared) for _, job in jobs]
    shared.close()
    for (name, job), g in zip(jobs, got):
        fresh = mcs.Context(0)
        want = job(mcs, fresh)
        fresh.close()
        assert len(g) == len(want), name
        for k, (a, b) in enumerate(zip(g, want)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (name, k)


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import gpu_common as G
    assert os.environ.get("MCS_NO_OVERLAP") == "1"
    e = dict(G=G, pkg=G.mcs, ctx=G.ctx())
    for name in ("2000", "8000_64"):
        sc, want = scene(name)
        for device in (False, True):
            check_chain(run(e, sc, device), want, sc, True, ("no overlap", name, device))
    print("child ok")
