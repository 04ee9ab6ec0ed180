"""-m gpu: mcs_triangulate_matches and mcs_create_new_map_points (cLocalMapping::CreateNewMapPoints, src/cLocalMapping.cpp:223-381) against the
line-by-line model of tests/newpoints_model.py: match12, verdict codes, accepted lists, final valid1 equal; x3D, baselines and median depths bit for bit
(their whole chain is + - * / and sqrt on both sides; only the projection reaches a libm call, and no compared quantity of these scenes lies within
1e-9 of its threshold — asserted on the model, also without a GPU in tests/test_newpoints_cpu.py).

These are well-behaved scenes.  The edge cases are in tests/test_gpu_hostile_newpoints.py (cases: tests/hostile_newpoints.py): tied, NaN and infinite depths at
every tile size of the median kernel and the gate at exactly 0.01, rigs beyond 256 camera pairs, compaction at the wave and chunk boundaries, comparisons exactly on
their thresholds, hostile camera models in the projection, entries outside their arrays, a repeated first keyframe and masked descriptors."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import newpoints_model as M
import newpoints_pack as P

pytestmark = pytest.mark.gpu

SCENES = {"3cam_5": dict(seed=11, nr_cams=3, n_points=900, n_neigh=5), "8cam_20": dict(seed=12, nr_cams=8, n_points=2400, n_neigh=20)}
_cache = {}


def scene(name):
    if name not in _cache:
        kf1, nb = M.make_scene(**SCENES[name])
        res, v1 = M.create_new_map_points(kf1, nb)
        _cache[name] = (kf1, nb, res, v1)
    return _cache[name]


def given_matches(kf1, nb, seed):
    """matches for part 1: every neighbour searched on its own (no dependence), plus a random partner for 70 % of the features left over"""
    rng = np.random.default_rng(seed)
    out = []
    for kf2 in nb:
        m12 = M.oracle_search(kf1, ~kf1.has_mp, kf2, M.essential_matrices(kf1, kf2), False)
        free = np.flatnonzero((m12 < 0) & (rng.random(kf1.n) < 0.7))
        m12[free] = rng.integers(0, kf2.n, len(free))
        out.append(m12)
    return out


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


def check_conditions(res):
    c = M.scene_conditions(res)
    assert c["gated"] >= 1 and c["accepted"] >= 100 and c["near"] == 0, c
    return c["codes"]


def test_model_conditions_hold():
    """every verdict code occurs over the scenes, a neighbour is gated, >= 100 accepted per scene, nothing within 1e-9 of a threshold, and later
    searches lose queries to earlier acceptances"""
    codes = set()
    for name in SCENES:
        kf1, nb, res, v1 = scene(name)
        codes |= check_conditions(res)
        assert res[-1]["queries"] < res[0]["queries"] - 100
    assert codes == set(range(9)), codes


@pytest.mark.parametrize("name", list(SCENES))
@pytest.mark.parametrize("device", [False, True])
def test_triangulate_given_matches(env, name, device):
    kf1, nb, _, _ = scene(name)
    matches = given_matches(kf1, nb, 5)
    assert sum(int((m >= 0).sum()) for m in matches) >= 3000
    skipped = np.zeros(len(nb), np.uint8)
    skipped[1] = 1
    want = [M.triangulate_matches(kf1, kf2, m, skipped=bool(sk)) for kf2, m, sk in zip(nb, matches, skipped)]
    assert sum(int(w["near"].sum()) for w in want) == 0
    got = P.triangulate(env["pkg"], env["ctx"], env["G"], [(kf1, kf2) for kf2 in nb], matches, device=device, skipped=skipped)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "%s pair %d" % (name, s), with_search=False)
    assert any(len(w["idx1"]) for w in want)


def test_degenerate_pairs_on_the_device(env):
    """a NaN ray is accepted with a NaN point, a zero ray takes the singular-A branch (Matx22d::inv() = 0), parallel rays stop at the parallax check: as the
    model, bit for bit"""
    import test_newpoints_cpu as H
    nan = float("nan")
    X = [0.3, 0.2, 4.0]
    k1, r1 = H.observe(H.pose(0), X)
    k2, r2 = H.observe(H.pose(1.0), X)
    rays1 = [r1, [nan, nan, nan], [0.0, 0.0, 0.0], r2, r1]
    a = H.rig1(H.pose(0), [k1] * 5, rays1)
    b = H.rig1(H.pose(1.0), [k2] * 5, [r2] * 5)
    m12 = np.array([0, 1, 2, 3, -1], np.int32)
    want = M.triangulate_matches(a, b, m12)
    assert want["verdict"].tolist() == [M.ACCEPTED, M.ACCEPTED, M.BEHIND_1, M.PARALLAX, M.NO_MATCH] and np.isnan(want["x3D"][1]).all()
    for device in (False, True):
        got = P.triangulate(env["pkg"], env["ctx"], env["G"], [(a, b)], [m12], device=device)[0]
        P.compare(got, want, "degenerate pairs", with_search=False)


@pytest.mark.parametrize("name", list(SCENES))
def test_chain_equals_model(env, name):
    kf1, nb, want, v1 = scene(name)
    check_conditions(want)
    got, gv1 = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=True)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "%s neighbour %d" % (name, s))
    assert np.array_equal(gv1, v1)


def test_chain_host_kind_equals_device_kind(env):
    kf1, nb, want, v1 = scene("3cam_5")
    gd, vd = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=True)
    gh, vh = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=False)
    assert np.array_equal(vd, vh) and np.array_equal(vh, v1)
    for s, (a, b) in enumerate(zip(gd, gh)):
        P.compare(a, b, "host vs device, neighbour %d" % s)
        assert a["fallbacks"] == b["fallbacks"]
        P.compare(b, want[s], "host kind, neighbour %d" % s)


def test_chain_split_in_two_calls(env):
    kf1, nb, want, v1 = scene("8cam_20")
    k = 7
    ga, va = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb[:k], device=True)
    gb, vb = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb[k:], device=True, valid1=va)
    for s, (g, w) in enumerate(zip(ga + gb, want)):
        P.compare(g, w, "split call, neighbour %d" % s)
    assert np.array_equal(vb, v1)


def test_chain_own_essential_matrices(env):
    """the caller's E blocks (as the sweep takes them) instead of the setup kernel's"""
    kf1, nb, want, v1 = scene("3cam_5")
    E = np.stack([M.essential_matrices(kf1, kf2) for kf2 in nb])
    got, gv1 = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=True, E=E)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "own E, neighbour %d" % s)
    assert np.array_equal(gv1, v1)


def test_chain_check_orientation(env):
    kf1, nb, _, _ = scene("3cam_5")
    want, v1 = M.create_new_map_points(kf1, nb, check_ori=True)
    plain, _ = M.create_new_map_points(kf1, nb, check_ori=False)
    assert sum(int((w["match12"] >= 0).sum()) for w in want) < sum(int((w["match12"] >= 0).sum()) for w in plain)   # the filter removes something
    assert M.scene_conditions(want)["near"] == 0
    for device in (True, False):
        got, gv1 = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=device, check_ori=True)
        for s, (g, w) in enumerate(zip(got, want)):
            P.compare(g, w, "checkOrientation, neighbour %d" % s)
        assert np.array_equal(gv1, v1)


def sweep_then_triangulate(env, kf1, nb):
    """what the library offered before: mcs_search_triangulation_sweep over all neighbours with ONE shared valid array, then per-pair triangulation"""
    pkg, ctx, G = env["pkg"], env["ctx"], env["G"]
    cap = pkg._capi
    ns, n1, nmax, dim = len(nb), kf1.n, max(k.n for k in nb), kf1.desc.shape[1]
    d2, v2, g2, r2 = np.zeros((ns * nmax, dim), np.uint8), np.zeros(ns * nmax, np.uint8), np.zeros(ns * nmax, np.int32), np.zeros((ns * nmax, 3))
    for s, k in enumerate(nb):
        lo = s * nmax
        d2[lo:lo + k.n], v2[lo:lo + k.n], g2[lo:lo + k.n], r2[lo:lo + k.n] = k.desc, ~k.has_mp, k.cam, k.rays
    v1 = np.ascontiguousarray(~kf1.has_mp, np.uint8)
    q = cap.DescSet(pkg.np_ptr(kf1.desc), None, pkg.np_ptr(v1), pkg.np_ptr(kf1.cam), n1, dim)
    t = cap.DescSet(pkg.np_ptr(d2), None, pkg.np_ptr(v2), pkg.np_ptr(g2), nmax, dim)
    E = np.ascontiguousarray(np.stack([M.essential_matrices(kf1, k) for k in nb]))
    m12, nm, fb = np.full(ns * n1, -1, np.int32), np.zeros(ns, np.int32), np.zeros(ns, np.int32)
    pkg.check(pkg.lib().mcs_search_triangulation_sweep(ctx.h, ns, q, 0, t, nmax, pkg.np_ptr(kf1.rays), pkg.np_ptr(r2), pkg.np_ptr(E), 9 * kf1.nr * kf1.nr, kf1.nr,
                                                       dim, 16, 0, pkg.np_ptr(m12), pkg.np_ptr(nm), pkg.np_ptr(fb)))
    matches = [m12[s * n1:(s + 1) * n1] for s in range(ns)]
    return matches, P.triangulate(pkg, ctx, G, [(kf1, k) for k in nb], matches)


def test_sweep_cannot_reproduce_the_loop_but_the_chain_does(env):
    """the neighbour loop is sequential: from the second searched neighbour on, the batched sweep matches features the reference no longer looks for"""
    kf1, nb, want, v1 = scene("8cam_20")
    queries = [w["queries"] for w in want]
    assert all(b <= a for a, b in zip(queries, queries[1:])) and queries[-1] < queries[0]   # the later searches really lose queries
    matches, tri = sweep_then_triangulate(env, kf1, nb)
    first = next(s for s, w in enumerate(want) if not w["skipped"])
    assert np.array_equal(matches[first], want[first]["match12"])   # the first searched neighbour sees the same valid flags either way
    differ = [s for s, w in enumerate(want) if not np.array_equal(matches[s], w["match12"])]
    assert min(differ) >= 1 and any(not want[s]["skipped"] for s in differ), differ
    got, gv1 = P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=True)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "neighbour %d" % s)
    assert np.array_equal(gv1, v1)


def test_chain_without_stream_overlap_in_a_child_process(env):
    """MCS_NO_OVERLAP=1 (read when the context is created): everything in order on one stream, same outputs"""
    e = dict(os.environ, MCS_NO_OVERLAP="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_refusals(env):
    pkg, ctx, G = env["pkg"], env["ctx"], env["G"]
    kf1, nb, _, _ = scene("3cam_5")
    bare = M.KF(nb[0].cams, nb[0].M_c, nb[0].M_t, nb[0].keys, nb[0].cam, nb[0].rays, nb[0].desc, None, np.zeros(nb[0].n, bool), nb[0].mp_pos)
    for device in (False, True):   # a neighbour without a map point: refused before anything runs
        P.chain(pkg, ctx, G, kf1, [nb[0], bare], device=device, expect=pkg._capi.MCS_ERR_INVALID)
    pkg.check(pkg.lib().mcs_ctx_set_async_search(ctx.h, 1))
    try:
        P.chain(pkg, ctx, G, kf1, nb[:2], device=True, expect=pkg._capi.MCS_ERR_UNSUPPORTED)
    finally:
        pkg.check(pkg.lib().mcs_ctx_set_async_search(ctx.h, 0))
    got, _ = P.chain(pkg, ctx, G, kf1, nb[:2], device=True)   # and the context still works
    assert got[0]["nmatches"] > 0


def test_frontend_on_device_extracted_keyframes(env):
    """smoke: CreateNewMapPoints over cMultiKeyFrame objects extracted on the device from synth.py's images (no rigid scene behind them, so no condition
    on the number accepted): the outputs are consistent with themselves and with the raw call's model"""
    FE = importlib.import_module("multicol-slam_amd.frontend")
    G = env["G"]
    cams = G.cams3()
    models = [FE.cCamModelGeneral_.from_dict(c) for c in cams]
    ex = FE.mdBRIEFextractorOct(_nfeatures=400, ctx=env["ctx"])
    rng = np.random.default_rng(3)
    kfs = []
    for f in range(3):
        Mt = np.eye(4)
        Mt[:3, 3] = [0.3 * f, 0.05 * f, 0.0]
        sys_ = FE.cMultiCamSys_(models, M_c=M.S.rig_poses(3), M_t=Mt)
        F = FE.cMultiFrame(G.synth.synth_multiframe(f, cams), 0.0, ex, None, sys_)
        kf = FE.cMultiKeyFrame(F)
        for i in rng.permutation(F.totalN)[:F.totalN // 5]:
            kf.mvpMapPoints[i] = FE.cMapPoint(Mt[:3, 3] + sys_.MtMc[int(kf.keypoint_to_cam[i])][:3, :3] @ (kf.mvKeysRays[i] * rng.uniform(2, 6)))
        kfs.append(kf)
    res, v1 = FE.CreateNewMapPoints(kfs[0], kfs[1:], featDim=ex.GetDescriptorSize(), ctx=env["ctx"])
    start = np.array([m is None for m in kfs[0].mvpMapPoints])
    taken = np.zeros(len(start), bool)
    for r, kf in zip(res, kfs[1:]):
        assert r["medianDepth"] == kf.ComputeSceneMedianDepth(2)
        assert abs(r["baseline"] - np.linalg.norm(kf.GetCameraCenter() - kfs[0].GetCameraCenter())) < 1e-12 and not r["skipped"]
        assert np.array_equal(r["idx1"], np.flatnonzero(r["verdict"] == 1)) and np.array_equal(r["idx2"], r["match12"][r["idx1"]])
        assert not taken[np.flatnonzero(r["match12"] >= 0)].any() and start[np.flatnonzero(r["match12"] >= 0)].all()
        taken[r["idx1"]] = True
    assert np.array_equal(v1, start & ~taken)


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import gpu_common as G
    assert os.environ.get("MCS_NO_OVERLAP") == "1"
    kf1, nb, want, v1 = scene("8cam_20")
    for device in (True, False):
        got, gv1 = P.chain(G.mcs, G.ctx(), G, kf1, nb, device=device)
        for s, (g, w) in enumerate(zip(got, want)):
            P.compare(g, w, "no overlap, neighbour %d" % s)
        assert np.array_equal(gv1, v1)
    print("child ok")
