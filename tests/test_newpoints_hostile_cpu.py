"""No GPU: every condition that tests/test_gpu_hostile_newpoints.py relies on, asserted on the model (tests/newpoints_model.py) and the case table
(tests/hostile_newpoints.py) alone: each case reaches what it is there for, the model's medians and gates equal answers derived by hand, the cases that are to
show a defect would show it (sensitivity), and no verdict that stands on a reprojection error or on z <= 0 lies within 1e-9 of its threshold (near_proj == 0;
where nothing is built onto a threshold on purpose, near == 0 altogether)."""
import math

import numpy as np
import pytest

import hostile_newpoints as HN
import newpoints_model as M
from newpoints_pack import same_bits

chain_model = HN.chain_model


def near_of(res, what="near"):
    return sum(int(r[what].sum()) for r in res)


# ---------------------------------------------------------------------------------------------- 1: median depth and the gate
def test_depths_are_the_chosen_numbers():
    """row 2 of MtMc_inv is (0, 0, 1, -tz) and every depth comes out as the double the builder chose"""
    for pattern in HN.MEDIAN_PATTERNS:
        for n in (4, 257):
            d, tx, tz, infx = HN.median_depths(pattern, n)
            kf = HN.depth_neighbour(d, tx, tz, infx)
            assert kf.MtMc_inv[0][2].tolist() == [0.0, 0.0, 1.0, -float(tz)]
            pos, cam = M.map_points(kf)
            with np.errstate(all="ignore"):
                z = M.mv(kf.MtMc_inv[cam], np.concatenate([pos, np.ones((n, 1))], axis=1))[:, 2]
            assert same_bits(z, d), (pattern, n)
            assert np.isinf(pos[infx, 0]).all() and np.isfinite(pos[infx, 2]).all()


@pytest.mark.parametrize("name", list(HN.median_calls()))
def test_median_calls(name):
    """the model's median and gate equal the hand-derived ones for every neighbour; gated and searched neighbours alternate; searched neighbours find matches
    until the current keyframe runs out of features; nothing near a threshold but the gate triples"""
    kf1, nb, exp = HN.median_calls()[name]
    res, v1 = chain_model(name, kf1, nb)
    assert len(nb) >= 6
    for r, e, kf in zip(res, exp, nb):
        assert same_bits([r["median"]], [e["median"]]) and r["skipped"] == e["skipped"], (e, r["median"], r["skipped"])
        assert len(kf.mp[1]) == e["n_mp"] and kf.n == HN.SEEN
        assert (r["verdict"] == M.SKIPPED).all() == r["skipped"]
    sk = [r["skipped"] for r in res]
    assert any(sk) and not all(sk) and any(a != b for a, b in zip(sk, sk[1:]))
    assert sum(int((r["match12"] >= 0).sum() > 0) for r in res) >= 3      # the search is live behind the gate
    assert near_of(res) == 0
    assert sum(r["gate_near"] for r in res) == (6 if name == "gate" else 0)


def test_median_patterns_reach_their_edges():
    for n in HN.MEDIAN_COUNTS:
        r = HN.rank(n)
        d, (lo, hi) = HN.tie_depths(n)
        s = sorted(d.tolist())
        assert s[r] == 5.0 and (d[lo:hi] == 5.0).all() and (d == 5.0).sum() == hi - lo
        if n > 1:
            assert hi - lo >= 2
        if n > HN.TILE:
            assert lo < HN.TILE - 1 and hi > HN.TILE                     # the run lies across the first tile boundary (indices 255 and 256)
        assert len(set(d.tolist())) == n - (hi - lo) + 1                  # everything else is distinct
        assert len(set(HN.median_depths("equal", n)[0].tolist())) == 1
        dd = HN.median_depths("distinct", n)[0]
        assert (np.diff(dd) < 0).all()
        assert HN.expected_median(HN.median_depths("negative", n)[0]) < 0
        for p in ("zero", "zero_at_kf1"):
            z, tx, tz, _ = HN.median_depths(p, n)
            assert HN.expected_median(z) == 0.0 and not np.signbit(HN.expected_median(z)) and (tx == 0 and tz == 0) == (p == "zero_at_kf1")
        assert np.isinf(HN.median_depths("inf", n)[0]).any()
        minor, major = HN.median_depths("nan_minor", n), HN.median_depths("nan_major", n)
        assert math.isnan(HN.expected_median(major[0])) and np.isnan(major[0]).sum() * 2 > n
        assert not math.isnan(HN.expected_median(minor[0]))
        if n >= 5:
            assert np.isnan(minor[0]).any() and minor[3].any() and (np.isnan(minor[0]) & ~minor[3]).any()   # both sources of a NaN depth
    lengths = [n for _, n in HN.MIXED]
    assert any(b < a for a, b in zip(lengths, lengths[1:])) and any(b > a for a, b in zip(lengths, lengths[1:])) and max(lengths) == 1025


def test_nan_depths_sort_last_in_the_model():
    """np.sort puts NaN behind every number, infinities included: the ordering the device is held to"""
    kf = HN.depth_neighbour([HN.NAN, HN.INF, 2.0, HN.NAN, -HN.INF], 1.0, 1)
    assert M.scene_median_depth(kf) == HN.INF                              # -inf, 2, inf, NaN, NaN: rank 2
    assert M.scene_median_depth(HN.depth_neighbour([HN.NAN, HN.INF, 2.0, -HN.INF], 1.0, 1)) == 2.0   # -inf, 2, inf, NaN: rank 1
    kf = HN.depth_neighbour([HN.NAN, HN.INF, HN.NAN, HN.NAN], 1.0, 1)
    assert math.isnan(M.scene_median_depth(kf))                             # inf, NaN, NaN, NaN: rank 1
    with np.errstate(all="ignore"):
        assert M.gate(HN.current_keyframe(), kf)[2] is False                # a NaN ratio does not gate


def test_gate_triples_are_what_the_search_finds():
    lo, at, hi = np.nextafter(0.01, 0.0), np.float64(0.01), np.nextafter(0.01, 1.0)
    for med, bs in HN.GATE_TRIPLES:
        assert bs == HN.find_gate_triple(med)
        assert [np.float64(b) / np.float64(med) for b in bs] == [lo, at, hi]
    kf1, nb, exp = HN.median_calls()["gate"]
    for kf, e, (med, b) in zip(nb, exp, [(m, b) for m, bs in HN.GATE_TRIPLES for b in bs]):
        baseline, median, skipped, near = M.gate(kf1, kf)
        assert (baseline, median) == (b, med) and skipped == e["skipped"] and near   # sqrt(b * b) == b for these
    assert [e["skipped"] for e in exp] == [True, False, False] * 2


def test_outside_cameras_give_nan_depths():
    kf1, nb, exp = HN.outside_camera_call()
    res, _ = chain_model("outside", kf1, nb)
    for r, e, kf in zip(res, exp, nb):
        assert same_bits([r["median"]], [e["median"]]) and r["skipped"] == e["skipped"]
    assert set(np.concatenate([kf.mp[1] for kf in nb]).tolist()) == set(HN.OUTSIDE_CAMS) | {0}
    assert near_of(res) == 0


# ---------------------------------------------------------------------------------------------- 2: essential matrices beyond 256 pairs
@pytest.mark.parametrize("nr", HN.RIG_SIZES)
def test_rig_scenes_need_the_later_essential_matrices(nr):
    """with the blocks t >= 256 zeroed the search loses matches at 17 and 32 cameras (at 16 there are exactly 256 blocks: nothing to lose)"""
    kf1, nb = HN.rig_scene(nr)
    res, _ = chain_model(("rig", nr), kf1, nb)
    assert near_of(res) == 0 and not any(r["skipped"] for r in res) and sum(len(r["idx1"]) for r in res) >= 20
    cut, _ = M.create_new_map_points(kf1, nb, search=HN.search_with_later_blocks_zeroed)
    differ = [not np.array_equal(a["match12"], b["match12"]) for a, b in zip(res, cut)]
    assert any(differ) == (nr * nr > HN.SETUP_TRIP), differ
    if nr * nr > HN.SETUP_TRIP:   # the search only pairs features of the same camera index: block c * nr + c, beyond 256 for the last cameras
        late = [c for c in range(nr) if c * nr + c >= HN.SETUP_TRIP]
        assert late and any(np.isin(kf1.cam[np.flatnonzero(r["match12"] >= 0)], late).any() for r in res)


# ---------------------------------------------------------------------------------------------- 3: compaction
@pytest.mark.parametrize("n1", HN.COMPACT_N1)
def test_compaction_rows(n1):
    """an accepted row is accepted, a rejected one stops at the parallax check, the accepted points are all different (a row taken from the wrong place shows)"""
    pairs = HN.compact_pairs(n1)
    assert len(pairs) >= 3 and {p[0] for p in pairs} >= {"all", "none", "second"}
    if n1 > 1024:
        assert len(pairs) == len(HN.COMPACT_PATTERNS)
    for name, a, b, m12, acc in pairs:
        r = M.triangulate_matches(a, b, m12)
        assert np.array_equal(r["verdict"] == M.ACCEPTED, acc) and (r["verdict"][~acc] == M.PARALLAX).all(), name
        assert r["near"].sum() == 0
        assert np.array_equal(r["idx1"], np.flatnonzero(acc)) and np.array_equal(r["idx2"], n1 - 1 - np.flatnonzero(acc))
        assert len(np.unique(r["acc_x3D"], axis=0)) == int(acc.sum())
    assert int(HN.accept_pattern("every65", 2049).sum()) == 31 and HN.accept_pattern("i1024", 1024) is None


def test_empty_keyframes_in_the_model():
    nb = HN.median_calls()["n3"][1][:2]
    res, v1 = chain_model("n1=0", HN.empty_current_keyframe(), nb)
    assert len(v1) == 0 and all(len(r["idx1"]) == 0 and len(r["match12"]) == 0 for r in res) and not math.isnan(res[0]["median"])
    kf1 = HN.current_keyframe()
    res, v1 = chain_model("n2=0", kf1, [HN.featureless_neighbour(), nb[0]])
    assert (res[0]["match12"] == -1).all() and res[0]["median"] == 4.0 and not res[0]["skipped"] and (res[1]["match12"] >= 0).any()


# ---------------------------------------------------------------------------------------------- 4: exact thresholds
def test_threshold_pair_turns_on_the_last_place():
    a, b, m12 = HN.threshold_pair()
    r = M.triangulate_matches(a, b, m12)
    cp, dmax = float(r["cosParallax"][0]), float(max(r["dist1"][0], r["dist2"][0]))
    assert r["verdict"].tolist() == [M.ACCEPTED] and 0 < cp < M.COS_THRESH and dmax < M.MAX_DIST and r["near"].sum() == 0
    for kw, want in ((dict(cosThresh=cp), M.ACCEPTED), (dict(cosThresh=float(np.nextafter(cp, 0.0))), M.PARALLAX),
                     (dict(maxDIST=dmax), M.ACCEPTED), (dict(maxDIST=float(np.nextafter(dmax, 0.0))), M.DISTANCE)):
        q = M.triangulate_matches(a, b, m12, **kw)
        assert q["verdict"].tolist() == [want], kw
        assert q["near_proj"].sum() == 0 and q["near"].sum() == 1           # on the threshold by construction; the projection is nowhere near one
        assert same_bits(q["x3D"], r["x3D"]) if want != M.PARALLAX else not q["x3D"].any()


def test_exact_pairs():
    want = {"orthogonal": (M.ACCEPTED, [0.0, 0.0, 2.0]), "on centre": (M.DISTANCE, [0.0, 0.0, 0.0]), "in camera": (M.BEHIND_2, [0.0, 0.0, 2.0])}
    for label, a, b in HN.exact_pairs():
        r = M.triangulate_matches(a, b, np.array([0], np.int32))
        assert (int(r["verdict"][0]), r["x3D"][0].tolist()) == want[label], (label, r["verdict"], r["x3D"])
        assert r["near_proj"].sum() == (1 if label == "in camera" else 0)    # z == 0 exactly there: + - * only, no libm call stands behind it
        if label != "in camera":
            assert r["cosParallax"][0] == 0.0 and not np.signbit(r["cosParallax"][0])
        if label == "on centre":
            assert r["dist1"][0] == 0.0 and r["dist2"][0] == 2.0
        if label == "in camera":
            assert (a.MtMc_inv[0] == np.rint(a.MtMc_inv[0])).all() and (b.MtMc_inv[0] == np.rint(b.MtMc_inv[0])).all()


# ---------------------------------------------------------------------------------------------- 5: camera models
@pytest.mark.parametrize("name", list(HN.camera_rigs()))
def test_camera_scenes(name):
    """the verdicts stand on these cameras' own terms: the same keyframes under plain cameras (and, for the short polynomials, under the padding read as
    coefficients) are decided differently; nothing within 1e-9 of a threshold"""
    kf1, nb = HN.camera_scene(name)
    res, _ = chain_model(("cam", name), kf1, nb)
    assert near_of(res) == 0 and sum(int((r["match12"] >= 0).sum()) for r in res) >= 60
    codes = set(np.concatenate([r["verdict"] for r in res]).tolist())
    assert codes & {M.REPROJ_1, M.REPROJ_2, M.ACCEPTED} and len(codes) >= 4, codes

    def verdicts(change):
        out = []
        for r, kf2 in zip(res, nb):
            with np.errstate(all="ignore"):
                out.append(M.triangulate_matches(HN.with_cameras(kf1, change(kf1.cams)), HN.with_cameras(kf2, change(kf2.cams)), r["match12"])["verdict"])
        return np.concatenate(out)
    mine = np.concatenate([M.triangulate_matches(kf1, kf2, r["match12"])["verdict"] for r, kf2 in zip(res, nb)])
    assert not np.array_equal(verdicts(HN.plain_cameras), mine)
    if any("invP_pad" in c for c in kf1.cams):
        assert not np.array_equal(verdicts(HN.padded_cameras), mine)
    assert {len(c["invP"]) for c in kf1.cams} == {len(c["invP"]) for c in nb[0].cams}


def test_camera_table_covers_the_issue():
    rigs = HN.camera_rigs()
    degs = [sorted(len(c["invP"]) for c in r) for r in rigs.values()]
    assert [1, 12, 16] in degs and [1, 6, 16] in degs
    assert all(all(v != 0.0 for v in c["invP"]) for r in rigs.values() for c in r)                       # every coefficient live
    assert any(abs(c["d"]) > 0.1 and abs(c["e"]) > 0.1 and abs(c["c"] - 1) > 0.1 for c in rigs["affine"] + rigs["corners"])
    assert all(not (0 <= c["u0"] < HN.CAM_W and 0 <= c["v0"] < HN.CAM_H) for c in rigs["outside"])


# ---------------------------------------------------------------------------------------------- 6: guards and staging
def test_guard_inputs_hit_rows_that_matter():
    g = HN.guard_inputs()
    clean = M.triangulate_matches(g["kf1"], g["kf2"], g["match12"])
    assert clean["near"].sum() == 0 and len(clean["idx1"]) >= 20
    kf1, kf2, m_in, m_want = HN.guarded(g)
    stopped = np.flatnonzero(m_want != g["match12"])
    assert len(stopped) == 12 and (clean["verdict"][stopped] != M.NO_MATCH).all() and (clean["verdict"][stopped] == M.ACCEPTED).any()
    assert sorted(g["bad_match"].values()) == [HN.INT_MIN, -7, g["kf2"].n, HN.INT_MAX]
    assert set(kf1.cam[list(g["bad_cam1"])].tolist()) == {-1, kf1.nr} and set(kf2.cam[list(g["bad_cam2"])].tolist()) == {-1, kf2.nr}
    want = M.triangulate_matches(g["kf1"], g["kf2"], m_want)
    rest = np.setdiff1d(np.arange(kf1.n), stopped)
    assert np.array_equal(want["verdict"][rest], clean["verdict"][rest]) and (want["verdict"][stopped] == M.NO_MATCH).all()


def test_aba_and_masked_scenes():
    pairs, matches = HN.aba_pairs()
    (A, _), (B, _), (A2, _) = pairs
    assert A is A2 and A.n == B.n and not np.array_equal(A.rays, B.rays)
    res = [M.triangulate_matches(a, b, m) for (a, b), m in zip(pairs, matches)]
    assert all(len(r["idx1"]) >= 10 and r["near"].sum() == 0 for r in res)
    assert not np.array_equal(res[0]["verdict"], res[2]["verdict"]) and not np.array_equal(res[1]["verdict"], res[2]["verdict"])
    kf1, nb = HN.masked_scene()
    res, _ = chain_model("masked", kf1, nb)
    plain, _ = chain_model("unmasked", HN.without_masks(kf1), [HN.without_masks(k) for k in nb])
    assert near_of(res) == 0 and sum(len(r["idx1"]) for r in res) >= 20
    assert any(not np.array_equal(a["match12"], b["match12"]) for a, b in zip(res, plain))   # the masks take part in the search
    zeros = 1.0 - np.unpackbits(kf1.mask[:, 10:]).mean()
    assert 0.08 < zeros < 0.17 and not nb[0].mask[::5, :10].any() and all(k.mask is not None for k in [kf1] + nb)
