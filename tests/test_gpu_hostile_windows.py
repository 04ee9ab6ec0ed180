"""-m gpu: the hostile window cases (tests/hostile_windows.py) on the device.  match, nmatches, `assigned` after the call, accepted_out and dist equal the
independent definition bit for bit, in both memory kinds, and the two kinds return identical bytes.  Every case goes through the raw entry point of its rule
(mcs_search_by_projection, mcs_window_match, mcs_window_best); the cluster, chain and order cases go through the slot form as well
(mcs_search_local_points with 1, 3 and 5 cameras, mcs_window_search_frames).

What a one-token change of csrc/mcs_project.hip would break, and where it shows (the first, fourth and fifth were made in the definition and moved 13, 45 and
46 cases; the others follow from the case data):
  member_key, radius test `>` -> `>=`          geometry/*: probes 0 and 2 sit at |kp - x| == r exactly and must match
  member_key, key `cell << 20 | index` swapped order/*: the first member in column-major cell order wins every tie, and it is never the lowest index
  member_key, cvRound -> floor                 geometry/128x96/*, levels/*: bins k + 1/2 (to even) and 63.5 -> 64 (dropped) move cells and members
  k_proj_greedy, the secondIdx claim check     chain/*: probe j's runner-up is probe j - 1's best; without the check lane j commits "no match" in the round in
                                               which lane j - 1 takes it, where the sequential loop accepts (149 links, rounds 63 / 64 and 127 / 128 included)
  k_proj_greedy, `cnt > kListK` -> `>=`        changes no result: a 16-member window then counts as full, which only sends a probe with fewer than two free
                                               entries into the exact rescan.  cluster/*/16 and /17 sit on both sides of the boundary; the other direction
                                               (17 members taken for a complete list) fails cluster/*/17 and situation/*
  make_window / member_key, int_x86 removed    pinned, geometry/*: NaN, infinite and huge centres, radii and keypoints (the kernels failed these before int_x86)"""
import numpy as np
import pytest

import frustum_model as M
import frustum_pack
import hostile_windows as H
import window_pack as W

pytestmark = pytest.mark.gpu

_want = {}


def want(c):
    if c["name"] not in _want:
        _want[c["name"]] = H.run(c)
    return _want[c["name"]]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


@pytest.mark.parametrize("group", ["geometry", "decision", "order", "cluster", "chain", "collision", "big", "steal", "empty"])
def test_raw_entry_points(env, group):
    cases = [c for c in H.cases() if c["group"] == group]
    assert cases
    for c in cases:
        host = W.run(env["pkg"], env["G"], env["ctx"], c, False)
        dev = W.run(env["pkg"], env["G"], env["ctx"], c, True)
        W.compare(host, want(c), (c["name"], "host"))
        W.compare(dev, want(c), (c["name"], "device"))
        assert sorted(host) == sorted(dev) and all(np.asarray(host[k]).tobytes() == np.asarray(dev[k]).tobytes() for k in host), c["name"]


def test_pinned_answers_on_the_device(env):
    c = next(c for c in H.cases() if c["name"] == "pinned")
    for device in (False, True):
        assert np.array_equal(W.run(env["pkg"], env["G"], env["ctx"], c, device)["match"], c["expect"])


def test_more_than_65536_features_are_refused(env):
    c = next(c for c in H.cases() if c["name"] == "big/assigned0/r1")
    F = c["frame"]
    grow = lambda a: np.concatenate([a, a[:1]])
    F2 = dict(F, keys=grow(F["keys"]), desc=grow(F["desc"]), cam=grow(F["cam"]), assigned=grow(F["assigned"]))
    assert len(F2["keys"]) == 65537
    for rule in (1, "best", 0):
        c2 = dict(c, frame=F2, rule=rule)
        if rule == 0:
            c2 = H.as_rule0(c2, "big/65537/r0", th=0.5)
        for device in (False, True):
            with pytest.raises(env["pkg"].McsError):
                W.run(env["pkg"], env["G"], env["ctx"], c2, device)


SLOT_CASES = ["cluster/identical/40/r0", "cluster/near/200/r0/ratio0.8", "cluster/near/17/r0/ratio1.0", "situation/B-accept/r0", "situation/C/r0", "situation/forty/r0",
              "chain/r0", "order/zero/r0", "order/equal/r0"]


@pytest.mark.parametrize("nr", [1, 3, 5])
def test_slot_form_local_points(env, nr):
    """mcs_search_local_points on caller-written stale slots == mcs_search_by_projection on the compacted list == the definition"""
    G, pkg, ctx = env["G"], env["pkg"], env["ctx"]
    cams = [G.cams3()[k % 3] for k in range(nr)]
    rig = M.make_rig(cams, 0, with_masks=False)
    # a world point some camera sees: the fresh point whose arrival lets the search run at all
    rng = np.random.default_rng(nr)
    cand = rng.normal(0, 2.0, (200, 3))
    _uv, inm = M.project(rig, cand)
    fresh_pos = cand[np.flatnonzero(inm.any(axis=1))[0]]
    for name in SLOT_CASES:
        c = next(c for c in H.cases() if c["name"] == name)
        assert int(c["frame"]["width"][0]) == cams[0]["width"] and int(c["frame"]["height"][0]) == cams[0]["height"]
        scene, slot = W.slot_scene(c, nr, rig, fresh_pos, np.random.default_rng(7), next_above=not name.startswith("chain"))
        n = len(scene[0]["pos"])
        results = []
        for device in (False, True):
            call = frustum_pack.Call(pkg, G, scene, device, desc_masks=False, th=c["th"], nnratio=c["nnratio"])
            pkg.check(call.run(ctx))
            if device:
                ctx.synchronize()
            got = call.read()
            assert got["n_to_match"] >= 1, name
            st = got["state"]
            seen = scene[0]["flags"] != 0
            for k in ("in_view", "level"):
                assert np.array_equal(st[k][seen], scene[2][k][seen]), (name, k)                      # the caller's stale fields are not written
            for k in ("proj_x", "proj_y", "view_cos"):
                assert frustum_pack.same_doubles(st[k][seen], scene[2][k][seen]), (name, k)
            cc, slots = W.compacted(c, scene, st)
            assert set(slot.tolist()) <= set(slots.tolist()) and len(slots) == len(slot) + got["n_to_match"], name
            exp = H.run(cc)
            match = np.full(n * nr, -1, np.int32)
            match[slots] = exp["match"]
            where = (name, nr, "device" if device else "host")
            assert np.array_equal(got["match"].reshape(-1), match), (where, np.flatnonzero(got["match"].reshape(-1) != match)[:8].tolist())
            assert got["nmatches"] == exp["nmatches"] and np.array_equal(got["assigned"], exp["assigned"]), where
            flat = W.run(pkg, G, ctx, cc, device)                                                     # the list form on the same probes
            assert np.array_equal(flat["match"], got["match"].reshape(-1)[slots]) and flat["nmatches"] == got["nmatches"], where
            assert np.array_equal(flat["assigned"], got["assigned"]), where
            results.append(got)
            assert (exp["match"] >= 0).sum() >= 1, name
        assert np.array_equal(results[0]["match"], results[1]["match"]) and np.array_equal(results[0]["assigned"], results[1]["assigned"]), name


def test_slot_form_window_search_frames(env):
    """the rule 1 cases whose probes are keypoints, through mcs_window_search_frames (its own zeroed `taken` scratch)"""
    count = 0
    for c in H.cases():
        if c["group"] not in ("cluster", "chain", "order", "collision") or not W.keypoint_probes(c):
            continue
        count += 1
        w = want(c)
        for device in (False, True):
            got = W.window_search_frames(env["pkg"], env["G"], env["ctx"], c, device)
            W.compare(got, w, (c["name"], "frames", device))
    assert count >= 6


def test_back_to_back_device_calls(env):
    """three device-kind calls of different sizes enqueued with no wait in between: each result equals its result when run alone"""
    pkg, G, ctx = env["pkg"], env["G"], env["ctx"]
    for names in (["cluster/near/200/r1/ratio0.8", "collision/r1", "situation/B-accept/r1"], ["collision/r3", "situation/steal-waves/r3", "steal/r3"],
                  ["cluster/identical/200/r0", "collision/r0", "decision/ratio-tie/r0"], ["geometry/754x480/best", "collision/r2", "cluster/near/40/r2/ratio0.8"]):
        cs = [next(c for c in H.cases() if c["name"] == n) for n in names]
        alone = [W.run(pkg, G, ctx, c, True) for c in cs]
        calls = [W.Call(pkg, G, c, True) for c in cs]
        for call in calls:
            call.enqueue(ctx)
        ctx.synchronize()
        for c, call, a in zip(cs, calls, alone):
            got = call.read()
            W.compare(got, a, (c["name"], "back to back"))
            W.compare(got, want(c), (c["name"], "back to back / definition"))
