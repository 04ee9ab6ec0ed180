"""The hostile window cases (tests/hostile_windows.py) on the CPU: the independent definition equals the oracle through every oracle entry point that can
express a case, the answers pinned on x86 hold, and the cases are not vacuous - the conditions are computed from the definition's own trace.  No GPU."""
import os

import numpy as np
import pytest

import hostile_windows as H
import oracle_lib as O


def by_group(group):
    return [c for c in H.cases() if c["group"] == group]


_results = {}


def definition(c):
    """the definition's result per case, computed once and shared"""
    if c["name"] not in _results:
        _results[c["name"]] = H.run(c)
    return _results[c["name"]]


def tight(c):
    """the oracle reads rows of exactly dim bytes"""
    return c["frame"]["desc"].shape[1] == c["dim"] and c["probes"]["desc"].shape[1] == c["dim"]


def oracle_view(F):
    return O.frame_view(F["keys"], F["desc"], F["mask"], F["cam"], F["width"], F["height"])


def uniform_int_radius(P):
    r = P["r"]
    return len(r) > 0 and np.all(r == r[0]) and np.isfinite(r[0]) and float(r[0]) == int(r[0]) and abs(int(r[0])) < 2**31


def oracle_forms(c):
    """[(entry point, result dict with the fields that entry point gives)]"""
    F, P, rule, dim = c["frame"], c["probes"], c["rule"], c["dim"]
    if not tight(c):
        return []
    masks = P["mask"] is not None
    n = len(P["cam"])
    out = []
    if rule == 0:
        asg = F["assigned"].copy() if len(F["assigned"]) else np.zeros(1, np.uint8)
        nm, match = O.search_by_projection(P["x"], P["y"], P["view_cos"], P["level"], P["cam"], P["desc"], P["mask"], F["keys"], F["desc"], F["mask"], F["cam"], asg,
                                           F["width"], F["height"], F["scales"], c["th"], c["nnratio"], masks)
        out.append(("search_by_projection", dict(match=match, nmatches=nm, assigned=asg[:len(F["keys"])])))
    elif rule in ("best", "best_taken", 2):
        fv, _keep = oracle_view(F)
        md = c["max_dist"] if rule != 2 else H.thresholds(dim, masks)[0]
        nm, match, dist, asg = O.window_best(P["x"], P["y"], P["r"], P["lo"], P["hi"], P["cam"], P["desc"], P["mask"], fv, F["assigned"], md, rule != "best", dim, masks)
        res = dict(match=match, nmatches=nm)
        if rule != 2:
            res["dist"] = dist
        if rule != "best":
            res["assigned"] = asg[:len(F["keys"])]
        out.append(("window_best", res))
    elif rule == 3:
        if n and uniform_int_radius(P) and np.array_equal(P["lo"], P["hi"]):
            k1 = np.zeros(n, H.KP_DTYPE)
            k1["octave"] = P["lo"]
            f1, _k1 = O.frame_view(k1, P["desc"], P["mask"], P["cam"], F["width"], F["height"])
            f2, _k2 = oracle_view(F)
            nm, m12, _pm = O.search_for_initialization(f1, f2, np.stack([P["x"], P["y"]], axis=1), int(P["r"][0]), c["nnratio"], dim, masks)
            out.append(("search_for_initialization", dict(match=m12, nmatches=nm)))
    elif rule == 1:
        with np.errstate(over="ignore"):
            x32, y32 = P["x"].astype(np.float32), P["y"].astype(np.float32)
        if (n and uniform_int_radius(P) and np.all(P["lo"] == -1) and np.all(P["hi"] == -1) and not F["assigned"].any() and np.array_equal(x32.astype(np.float64), P["x"])
                and np.array_equal(y32.astype(np.float64), P["y"])):
            k1 = np.zeros(n, H.KP_DTYPE)
            k1["x"], k1["y"] = x32, y32
            f1, _k1 = O.frame_view(k1, P["desc"], P["mask"], P["cam"], F["width"], F["height"])
            f2, _k2 = oracle_view(F)
            nm, m21 = O.window_search(f1, np.ones(n, np.uint8), f2, int(P["r"][0]), 0, -1, c["nnratio"], dim, masks)
            match = np.full(n, -1, np.int32)
            match[m21[m21 >= 0]] = np.nonzero(m21 >= 0)[0]
            out.append(("window_search", dict(match=match, nmatches=nm, assigned=(m21 >= 0).astype(np.uint8))))
    return out


@pytest.mark.parametrize("group", ["geometry", "decision", "order", "cluster", "chain", "collision", "big", "steal", "empty"])
def test_definition_equals_oracle(group):
    forms = {}
    for c in by_group(group):
        want = definition(c)
        for entry, got in oracle_forms(c):
            forms[entry] = forms.get(entry, 0) + 1
            for k, v in got.items():
                assert np.array_equal(np.asarray(v), np.asarray(want[k])), (c["name"], entry, k, np.asarray(v).tolist()[:40], np.asarray(want[k]).tolist()[:40])
    assert forms, group
    # every entry point that can express a rule of this group was exercised
    rules = {c["rule"] for c in by_group(group) if tight(c)}
    assert ("search_by_projection" in forms) == (0 in rules) and ("window_best" in forms) == bool(rules & {2, "best", "best_taken"})


def test_every_oracle_entry_point_is_reached():
    seen = set()
    for c in H.cases():
        if c["group"] in ("big", "collision", "geometry"):
            continue
        seen |= {e for e, _ in oracle_forms(c)}
    assert seen == {"search_by_projection", "window_best", "search_for_initialization", "window_search"}


def test_pinned_x86_answers():
    c = next(c for c in H.cases() if c["name"] == "pinned")
    assert np.array_equal(definition(c)["match"], c["expect"])
    (entry, got), = oracle_forms(c)
    assert np.array_equal(got["match"], c["expect"]), got["match"]
    assert H.x86_int(np.nan) == H.INT_MIN and H.x86_int(2.0 ** 31) == H.INT_MIN and H.x86_int(-2.0 ** 31) == -2**31 and H.x86_int(-2.0 ** 31 - 1) == H.INT_MIN
    assert H.x86_int(2.0 ** 31 - 1) == 2**31 - 1 and [int(v) for v in H.cv_round(np.array([0.5, 1.5, 2.5, 63.5, -0.5]))] == [0, 2, 2, 64, 0]


def test_geometry_cases_are_not_vacuous():
    """the windows that should hold something do, the dropped bins are dropped, and the non-finite probes find nothing"""
    for c in by_group("geometry"):
        if not c["name"].endswith("/best") or not c["name"].startswith("geometry/"):
            continue
        r = definition(c)
        F = c["frame"]
        G = H.Grid(F)
        dropped = np.nonzero(G.cell_of < 0)[0]
        assert len(dropped) >= 4 and not np.isin(r["match"], dropped).any(), c["name"]
        # a dropped keypoint inside a probe's radius exists (so "never a member" is tested), e.g. the one at (w - 0.01, 10)
        P = c["probes"]
        kx, ky = F["keys"]["x"].astype(np.float64), F["keys"]["y"].astype(np.float64)
        with np.errstate(invalid="ignore"):
            inside = [(abs(kx[j] - P["x"]) <= P["r"]) & (abs(ky[j] - P["y"]) <= P["r"]) for j in dropped]
        assert np.any(inside), c["name"]
        assert (r["match"][:4] >= 0).tolist() == [True, False, True, False], (c["name"], r["match"][:4])      # |kp - x| == r, and the next double
        assert r["match"][4] >= 0 and r["match"][5] < 0 and (r["match"][10:14] < 0).all() and (r["match"][14:18] >= 0).all(), (c["name"], r["match"][:20])
        with np.errstate(invalid="ignore"):
            wild = ~(np.isfinite(P["x"]) & np.isfinite(P["y"]) & np.isfinite(P["r"])) | (abs(P["x"]) >= 1e12) | (abs(P["y"]) >= 1e12) | (abs(P["r"]) >= 1e12)
        assert wild.sum() >= 13 and (r["match"][wild] < 0).all(), c["name"]
    # round-half-even on the 128 x 96 lattice: bins k + 0.5 go to the even neighbour
    F = next(c for c in H.cases() if c["name"] == "geometry/128x96/best")["frame"]
    G = H.Grid(F)
    on = F["keys"]["x"] % 2 == 1
    bx = (F["keys"]["x"].astype(np.float64) * 0.5)[on]
    cells = G.cell_of[on]
    assert np.all((cells < 0) | (cells // H.ROWS % 2 == 0)) and np.any(bx % 2 == 1.5) and np.any(bx % 2 == 0.5)
    # level modes: the takes per mode stop where the mode says
    c = next(c for c in H.cases() if c["name"] == "levels/128x96/taken")
    took = (definition(c)["match"] >= 0).reshape(len(H.LEVEL_MODES), 9).sum(axis=1)
    assert took[H.LEVEL_MODES.index((5, 2))] == 0 and took[H.LEVEL_MODES.index((-2, -2))] == 0 and took[H.LEVEL_MODES.index((-1, -1))] == 9 and took.max() == 9


def test_decision_cases_are_not_vacuous():
    for c in by_group("decision"):
        r = definition(c)
        if "/max" in c["name"] or "ratio-tie" in c["name"] or len(r["match"]) != 8:
            continue
        # distances TH_HIGH, TH_HIGH + 1, TH_LOW, TH_LOW + 1, ... one member each
        want = [True, False, True, True] if c["rule"] != 3 else [False, False, True, False]
        assert (r["match"][:4] >= 0).tolist() == want, (c["name"], r["match"])
    tie = {c["name"]: definition(c)["match"].tolist() for c in by_group("decision") if "ratio-tie" in c["name"]}
    assert tie["decision/ratio-tie/r1"][0] == 0 and tie["decision/ratio-tie/r3"][0] == -1 and tie["decision/ratio-tie/r0-level0"][0] == 0
    assert tie["decision/ratio-tie/r0"][3] == 5 and tie["decision/ratio-tie/r1-all-levels"][3] == -1      # a closer runner-up on another octave: rule 0 applies no ratio
    assert tie["decision/ratio-tie/r1"][2] == 4                                                           # a single member: second = INT_MAX


def test_tie_cases_pick_the_visiting_order_not_the_index():
    for c in by_group("order"):
        r = definition(c)
        other = [p for p, t in enumerate(r["trace"]) if t and t["members"] and r["match"][p] >= 0 and t["lowest_tied"] != r["match"][p]]
        assert len(other) >= 2, c["name"]


def test_cluster_cases_use_up_the_short_lists():
    for rule in (0, 1, 2, 3):
        sit, used_up = {}, 0
        for c in by_group("cluster"):
            if c["rule"] != rule:
                continue
            for t in definition(c)["trace"]:
                if t and t["members"] and t["full"]:
                    used_up += t["listed_free"] == 0
                    sit[t["situation"]] = sit.get(t["situation"], 0) + 1
        assert used_up >= 10, (rule, used_up)
        for s in ("C", "D") if rule == 2 else ("A", "B", "C", "D"):
            assert sit.get(s, 0) >= 1, (rule, sit)
    # the hand-built situations are what their names say, and a window with every member assigned exists
    for c in by_group("cluster"):
        if c["name"].startswith("situation/") and c["rule"] in (0, 1):
            want = c["name"].split("/")[1][0]
            if want in "ABCD":
                assert definition(c)["trace"][0]["situation"] == want, c["name"]
        if "all-assigned" in c["name"]:
            assert (definition(c)["match"] < 0).all()
    got = {c["name"]: definition(c)["match"].tolist() for c in by_group("cluster") if c["name"].startswith("situation/")}
    for rule in (0, 1):
        assert got["situation/A/r%d" % rule] == [14] and got["situation/B-accept/r%d" % rule] == [15] and got["situation/B-reject/r%d" % rule] == [-1]
        assert got["situation/C/r%d" % rule][0] == 16 and got["situation/D/r%d" % rule] == [-1, -1]


def test_chain_links_flip():
    for c in by_group("chain"):
        G = H.Grid(c["frame"])
        full = H.run(c, grid=G)["match"]
        assert (full >= 0).all()
        for j in c["links"]:
            alone = H.run(c, skip={j - 1}, grid=G, only=j)["match"][j]
            assert (alone >= 0) != (full[j] >= 0), (c["name"], j)


def test_collision_cases_collide():
    for c in by_group("collision"):
        tr = definition(c)["trace"]
        pairs = 0
        for b in range(len(tr)):
            for a in range(b - b % 64, b):
                if tr[a] and tr[b] and tr[a]["members"] and tr[b]["members"] and tr[a]["best"] >= 0:
                    pairs += any(f >= 0 and f != tr[a]["best"] and (f & 4095) == (tr[a]["best"] & 4095) for f in (tr[b]["best"], tr[b]["second"]))
        assert pairs >= 4, (c["name"], pairs)
        assert (definition(c)["match"] >= 0).sum() >= 100


def test_big_frame_matches_its_last_feature():
    for c in by_group("big"):
        m = definition(c)["match"]
        assert len(c["frame"]["keys"]) == 65536 and len(m) <= 8
        if "assigned0" in c["name"]:
            assert 65535 in m and (0 in m or c["rule"] == "best"), (c["name"], m)
        elif c["rule"] not in (3, "best"):
            assert 65535 not in m and 0 in m, (c["name"], m)


def test_steals():
    for c in by_group("steal"):
        r = definition(c)
        assert r["steals"] >= c["min_steals"] and r["nmatches"] == (r["accepted"] >= 0).sum() - r["steals"] == (r["match"] >= 0).sum()
        m, a = r["match"], r["accepted"]
        assert a[[0, 1, 2, 3]].tolist() == [0, 0, 0, 0] and m[[0, 1, 2, 3, 4, 5]].tolist() == [-1, -1, -1, 0, -1, -1]      # stolen three times; equal does not steal
        assert m[[10, 70, 130, 199]].tolist() == [-1, -1, 1, -1] and m[[20, 21, 22]].tolist() == [-1, -1, 2] and a[20] == 2 and a[21] == -1
        assert m[[63, 64, 127, 128]].tolist() == [-1, -1, -1, 3]


REF_SO = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "libmcs_ref.so")


@pytest.mark.skipif(not os.path.exists(REF_SO), reason="oracle/_ref not built (needs the reference checkout)")
def test_hostile_centres_through_the_reference(tmp_path):
    """What the compiled reference can express of the table: its frames come from images only, but SearchForInitialization takes any centre.  The geometry
    probes' centres (outside the image, non-finite, huge) replace the first vbPrevMatched entries of a natural frame pair; reference == definition."""
    import importlib
    import ref_scene
    import test_io_formats as T
    import test_oracle_vs_ref_match as R
    synth = importlib.import_module("multicol-slam_amd.synth")
    io = importlib.import_module("multicol-slam_amd.io")
    voc = str(tmp_path / "voc.yml")
    R.flat_vocabulary(voc)
    cams = synth.lafida_cameras()
    masks = [np.ascontiguousarray(synth.mirror_mask(c)) for c in cams]
    S = ref_scene.RefScene(cams, masks, [io.cayley2hom(c) for c in T.CAYLEY], voc, nfeatures=400, do_dBrief=0, learnMasks=0)
    try:
        poses = [np.eye(4), R.motion(0.4, [0.02, -0.01, 0.015])]
        fr = [S.frame(S.add_frame(synth.synth_multiframe(f, cams), 0.04 * f, poses[f])) for f in range(2)]
        n0 = fr[0]["n"]
        F = H.frame(np.ascontiguousarray(fr[1]["keys"]), fr[1]["desc"], cam=fr[1]["cam"], size=(R.W, R.H), nr_cams=R.NC)
        F["scales"] = np.cumprod([1.0] + [float(np.float32(1.2))] * 7)
        xyr = H.geometry_probes((R.W, R.H), np.random.default_rng(5))
        prev = np.stack([fr[0]["keys"]["x"], fr[0]["keys"]["y"]], axis=1).astype(np.float64)
        prev[:len(xyr)] = xyr[:, :2]
        octave = fr[0]["keys"]["octave"].astype(np.int32)
        for window in (5, 60):
            p, m12 = prev.copy(), np.zeros(n0, np.int32)
            cnt = S.L.rs_search_init(S.h, 0, 1, p.ctypes.data, window, 0.9, 0, m12.ctypes.data)
            c = H.case("reference/init/%d" % window, "geometry", 3, F, H.probes(prev[:, 0], prev[:, 1], float(window), fr[0]["desc"], octave, octave, fr[0]["cam"]), nnratio=0.9)
            r = H.run(c)
            assert cnt == r["nmatches"] and np.array_equal(m12, r["match"]), (window, int((m12 != r["match"]).sum()))
            wild = ~np.isfinite(prev).all(axis=1) | (np.abs(prev) >= 1e12).any(axis=1)
            assert wild.sum() >= 8 and (m12[wild] < 0).all() and cnt > 20
    finally:
        S.close()
