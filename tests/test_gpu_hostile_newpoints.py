"""-m gpu: mcs_triangulate_matches and mcs_create_new_map_points (csrc/mcs_newpoints.hip) against the model of tests/newpoints_model.py on the hostile cases of
tests/hostile_newpoints.py, in host and device memory kind: verdicts, accepted lists, match12, nmatches, skipped flags and the final valid1 equal; x3D, accepted
x3D, baselines and median depths bit for bit (newpoints_pack.compare; a NaN equals any NaN).  No tolerance anywhere: what every case is there for, and that no
verdict standing on a reprojection error or on z <= 0 lies within 1e-9 of its threshold, is asserted on the model in tests/test_newpoints_hostile_cpu.py.
Refusals are pinned by code and text."""
import numpy as np
import pytest

import hostile_newpoints as HN
import newpoints_model as M
import newpoints_pack as P

pytestmark = pytest.mark.gpu
KINDS = [pytest.param(False, id="host"), pytest.param(True, id="device")]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return dict(G=G, pkg=G.mcs, ctx=G.ctx())


def chain(env, kf1, nb, device, **kw):
    return P.chain(env["pkg"], env["ctx"], env["G"], kf1, nb, device=device, **kw)


def triangulate(env, pairs, matches, device, **kw):
    return P.triangulate(env["pkg"], env["ctx"], env["G"], pairs, matches, device=device, **kw)


def check_chain(env, key, kf1, nb, device, **kw):
    want, v1 = HN.chain_model(key, kf1, nb)
    got, gv1 = chain(env, kf1, nb, device, **kw)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "%s, neighbour %d" % (key, s))
    assert np.array_equal(gv1, v1)
    return got


def chain_refused(env, kf1, nb, device, text, **kw):
    pkg = env["pkg"]
    chain(env, kf1, nb, device, expect=pkg._capi.MCS_ERR_INVALID, **kw)
    assert pkg.lib().mcs_last_error().decode() == text


def triangulate_refused(env, pairs, matches, device, text):
    pkg = env["pkg"]
    with pytest.raises(pkg.McsError) as e:
        triangulate(env, pairs, matches, device)
    assert e.value.code == pkg._capi.MCS_ERR_INVALID and str(e.value).endswith(": " + text), str(e.value)


# ---------------------------------------------------------------------------------------------- 1: median depth and the gate
@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("name", list(HN.median_calls()))
def test_median_depth_and_gate(env, name, device):
    """k_np_median on 1 .. 1025 depths: distinct, all equal, a run of ties over the tile boundary, negative / zero / infinite medians, NaN depths in the last
    ranks; the gate at the double 0.01 and its neighbours; a shorter neighbour behind a longer one in the same call"""
    kf1, nb, exp = HN.median_calls()[name]
    got = check_chain(env, name, kf1, nb, device)
    for g, e in zip(got, exp):
        assert P.same_bits([g["median"]], [e["median"]]) and g["skipped"] == e["skipped"], e


def test_map_point_camera_outside_the_rig(env):
    """device kind: the depth is NaN and sorts last; host kind: refused"""
    kf1, nb, exp = HN.outside_camera_call()
    got = check_chain(env, "outside", kf1, nb, True)
    for g, e in zip(got, exp):
        assert P.same_bits([g["median"]], [e["median"]]) and g["skipped"] == e["skipped"], e
    chain_refused(env, kf1, nb, False, "map point camera outside the rig")


# ---------------------------------------------------------------------------------------------- 2: essential matrices beyond 256 pairs
@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("own_E", [False, True], ids=["kernel E", "caller E"])
@pytest.mark.parametrize("nr", HN.RIG_SIZES)
def test_rigs_beyond_256_camera_pairs(env, nr, own_E, device):
    kf1, nb = HN.rig_scene(nr)
    E = np.stack([M.essential_matrices(kf1, kf2) for kf2 in nb]) if own_E else None
    check_chain(env, ("rig", nr), kf1, nb, device, E=E)


# ---------------------------------------------------------------------------------------------- 3: compaction
@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n1", HN.COMPACT_N1)
def test_compaction_boundaries(env, n1, device):
    """every accept pattern of one n1 in one call (one pair each: the per-pair offsets); in device kind the rows past acc_count keep what the caller wrote
    (a host-kind call copies the whole staged arrays back: those rows are unspecified there)"""
    cases = HN.compact_pairs(n1)
    pairs, matches = [(a, b) for _, a, b, _, _ in cases], [m for _, _, _, m, _ in cases]
    want = HN.pair_model(("compact", n1), pairs, matches)
    got, raw = triangulate(env, pairs, matches, device, raw=True)
    for s, ((name, _, _, _, acc), g, w) in enumerate(zip(cases, got, want)):
        P.compare(g, w, "n1 = %d, %s" % (n1, name), with_search=False)
        k = int(acc.sum())
        assert int(raw["acc_count"][s]) == k == len(g["idx1"]) and (np.diff(g["idx1"]) > 0).all()
        if device:
            assert (raw["acc_idx1"][s * n1 + k:(s + 1) * n1] == -9).all() and (raw["acc_idx2"][s * n1 + k:(s + 1) * n1] == -9).all(), name
            assert (raw["acc_x3D"][3 * (s * n1 + k):3 * (s + 1) * n1] == -7.0).all(), name
    if device and n1 == 0:
        assert (raw["acc_idx1"] == -9).all() and (raw["acc_x3D"] == -7.0).all() and (raw["verdict"] == -9).all()


@pytest.mark.parametrize("device", KINDS)
def test_chain_with_an_empty_current_keyframe(env, device):
    """n1 = 0: nothing to match, baseline and median are written all the same"""
    nb = HN.median_calls()["n3"][1][:2]
    got = check_chain(env, "n1=0", HN.empty_current_keyframe(), nb, device)
    assert [g["nmatches"] for g in got] == [0, 0] and all(len(g["idx1"]) == 0 for g in got) and got[0]["median"] == 2.0 and got[0]["baseline"] > 1.0


@pytest.mark.parametrize("device", KINDS)
def test_chain_with_a_featureless_neighbour(env, device):
    """a neighbour with map points and no feature: no match, the next neighbour is searched as usual"""
    nb = [HN.featureless_neighbour(), HN.median_calls()["n3"][1][0]]
    got = check_chain(env, "n2=0", HN.current_keyframe(), nb, device)
    assert got[0]["nmatches"] == 0 and got[0]["median"] == 4.0 and got[1]["nmatches"] > 0


# ---------------------------------------------------------------------------------------------- 4: exact thresholds
@pytest.mark.parametrize("device", KINDS)
def test_thresholds_in_the_last_place(env, device):
    """cosParallax > cosThresh and dist > maxDIST are strict: equal passes, one place below stops"""
    a, b, m12 = HN.threshold_pair()
    base = HN.pair_model("threshold", [(a, b)], [m12])[0]
    cp, dmax = float(base["cosParallax"][0]), float(max(base["dist1"][0], base["dist2"][0]))
    for kw, verdict in ((dict(), M.ACCEPTED), (dict(cosThresh=cp), M.ACCEPTED), (dict(cosThresh=float(np.nextafter(cp, 0.0))), M.PARALLAX),
                        (dict(maxDIST=dmax), M.ACCEPTED), (dict(maxDIST=float(np.nextafter(dmax, 0.0))), M.DISTANCE)):
        want = HN.pair_model(("threshold", tuple(kw.items())), [(a, b)], [m12], **kw)[0]
        assert want["verdict"].tolist() == [verdict]
        got = triangulate(env, [(a, b)], [m12], device, **kw)[0]
        P.compare(got, want, "thresholds %s" % kw, with_search=False)


@pytest.mark.parametrize("device", KINDS)
def test_exact_right_angle_and_zero_distance(env, device):
    """cosParallax == 0.0 is not < 0; a point on a rig centre has dist == 0; a point in a camera centre has z == 0 <= 0"""
    cases = HN.exact_pairs()
    pairs, matches = [(a, b) for _, a, b in cases], [np.array([0], np.int32)] * len(cases)
    want = HN.pair_model("exact", pairs, matches)
    assert [int(w["verdict"][0]) for w in want] == [M.ACCEPTED, M.DISTANCE, M.BEHIND_2]
    got = triangulate(env, pairs, matches, device)
    for (label, _, _), g, w in zip(cases, got, want):
        P.compare(g, w, label, with_search=False)


# ---------------------------------------------------------------------------------------------- 5: camera models in the projection
@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("name", list(HN.camera_rigs()))
def test_camera_models(env, name, device):
    """np_world_to_cam: polynomial degrees 1, 6, 12 and 16 side by side in one rig (the struct holds 1e3 behind a short polynomial), affine terms away from the
    identity, principal points in a corner and outside the image"""
    kf1, nb = HN.camera_scene(name)
    check_chain(env, ("cam", name), kf1, nb, device)


@pytest.mark.parametrize("deg", [0, 17])
def test_bad_polynomial_degree_is_refused_in_host_kind(env, deg):
    kf1, nb = HN.bad_degree_scene(deg)
    chain_refused(env, kf1, nb, False, "bad polynomial degree")
    a, b, m12 = HN.threshold_pair()
    cams = [dict(a.cams[0], invP_deg=deg)]
    triangulate_refused(env, [(HN.with_cameras(a, cams), b)], [m12], False, "bad polynomial degree")
    triangulate_refused(env, [(a, HN.with_cameras(b, cams))], [m12], False, "bad polynomial degree")


# ---------------------------------------------------------------------------------------------- 6: guards and staging
GUARDS = {"match12": dict(match=True, cam1=False, cam2=False), "keypoint_to_cam 1": dict(match=False, cam1=True, cam2=False),
          "keypoint_to_cam 2": dict(match=False, cam1=False, cam2=True), "all": dict(match=True, cam1=True, cam2=True)}


@pytest.mark.parametrize("which", list(GUARDS))
def test_entries_outside_their_arrays_in_device_kind(env, which):
    """match12 = -7, INT_MIN, kf2.n, INT_MAX and cameras -1, nr_cams on either side: no match on exactly those rows, every other row as without them"""
    g = HN.guard_inputs()
    kf1, kf2, m_in, m_want = HN.guarded(g, **GUARDS[which])
    want = HN.pair_model(("guard", which), [(g["kf1"], g["kf2"])], [m_want])[0]
    got = triangulate(env, [(kf1, kf2)], [m_in], True)[0]
    P.compare(got, want, which, with_search=False)
    clean = triangulate(env, [(g["kf1"], g["kf2"])], [g["match12"]], True)[0]
    stopped = m_want != g["match12"]
    assert stopped.sum() == 4 * sum(GUARDS[which].values())
    assert (got["verdict"][stopped] == M.NO_MATCH).all() and not got["x3D"][stopped].any()
    assert np.array_equal(got["verdict"][~stopped], clean["verdict"][~stopped]) and P.same_bits(got["x3D"][~stopped], clean["x3D"][~stopped])


def test_entries_outside_their_arrays_in_host_kind(env):
    """refused one by one; a negative match12 entry of any size is "no match", as in device kind"""
    g = HN.guard_inputs()
    pair = [(g["kf1"], g["kf2"])]
    negative = {}
    for r, v in g["bad_match"].items():
        m = g["match12"].copy()
        m[r] = v
        if v >= 0:
            triangulate_refused(env, pair, [m], False, "match12 entry outside the second keyframe")
        else:
            negative[r] = v
    assert sorted(negative.values()) == [HN.INT_MIN, -7]
    m_in, m_want = g["match12"].copy(), g["match12"].copy()
    for r, v in negative.items():
        m_in[r], m_want[r] = v, -1
    P.compare(triangulate(env, pair, [m_in], False)[0], HN.pair_model(("guard", "negative"), pair, [m_want])[0], "negative entries", with_search=False)
    for side, bad in ((0, g["bad_cam1"]), (1, g["bad_cam2"])):
        for i, v in bad.items():
            kf = pair[0][side]
            c = kf.cam.copy()
            c[i] = v
            kfs = list(pair[0])
            kfs[side] = HN.clone(kf, cam=c)
            triangulate_refused(env, [tuple(kfs)], [g["match12"]], False, "keypoint_to_cam outside the rig")


@pytest.mark.parametrize("device", KINDS)
def test_first_keyframes_a_b_a(env, device):
    """host kind stages a repeated first keyframe once (A, B, A: the third pair shares the first one's copy): equal to three single-pair calls and to the model"""
    pairs, matches = HN.aba_pairs()
    want = HN.pair_model("aba", pairs, matches)
    got = triangulate(env, pairs, matches, device)
    for s, (g, w) in enumerate(zip(got, want)):
        P.compare(g, w, "A, B, A: pair %d" % s, with_search=False)
        single = triangulate(env, [pairs[s]], [matches[s]], device)[0]
        P.compare(g, single, "A, B, A: pair %d against a call of its own" % s, with_search=False)


@pytest.mark.parametrize("device", KINDS)
def test_masked_descriptors_through_the_chain(env, device):
    kf1, nb = HN.masked_scene()
    check_chain(env, "masked", kf1, nb, device)
    for mixed in ((kf1, [nb[0], HN.without_masks(nb[1])]), (HN.without_masks(kf1), nb)):
        chain_refused(env, mixed[0], mixed[1], device, "neighbour: descriptor stride / masks differ")
