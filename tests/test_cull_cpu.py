"""tests/cull_model.py against hand-derived values: cLocalMapping::KeyFrameCulling (src/cLocalMapping.cpp:517-593) with the erasures of
cMultiKeyFrame::SetBadFlag / cMapPoint::EraseAllObservations, and cLocalMapping::MapPointCulling (:187-221).  Each case names a quirk of the reference and fails
if the model "fixes" it.  The same cases run on the device in tests/test_gpu_cull.py."""
import pytest

import covis_model as M
import cull_model as CM

CASES = CM.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_case(case):
    name, rows, octs, bad, kfs, ne, want = case
    res = CM.keyframe_culling(CM.store_of(rows, bad), octs, kfs, ne)
    for k, v in want.items():
        assert res[k] == v, (name, k, res[k], v)


def by_name(name):
    c = next(c for c in CASES if c[0] == name)
    return CM.keyframe_culling(CM.store_of(c[1], c[3]), c[2], c[4], c[5])


def test_a_point_at_two_features_counts_twice_and_is_judged_per_feature():
    r = by_name("two_features_two_octaves")
    assert r["n_mps"] == [2] and r["n_redundant"] == [1] and r["octave_rejects"] == 1


def test_observations_3_is_not_examined_and_4_is():
    # point 0 with observers 1 .. n: at n == 3 the octave loop never runs; at n == 4 it runs (and finds three others, never five)
    for n, examined in ((3, False), (4, True)):
        rows = {k: [0] for k in range(1, n + 1)}
        seen = []

        class Probe(dict):
            def __getitem__(self, k):
                seen.append(k)
                return dict.__getitem__(self, k)
        st = CM.store_of(rows)
        octs = {k: [0] for k in rows}
        m = CM._Map(st, octs)
        m.st.octaves = Probe(m.st.octaves)
        orig = CM._Map
        try:
            CM._Map = lambda s, o: m
            r = CM.keyframe_culling(st, octs, [1])
        finally:
            CM._Map = orig
        assert r["n_mps"] == [1] and r["n_redundant"] == [0]
        assert bool(seen) == examined, (n, seen)


def test_thresholds_of_the_ratio():
    assert by_name("nine_of_ten")["verdict"] == [0]                    # 9 > 9.0 is false
    assert by_name("ten_of_ten")["verdict"] == [1]
    assert by_name("nineteen_of_twenty")["verdict"] == [1]             # 19 > 18.0
    assert by_name("no_points")["verdict"] == [0]                      # 0 > 0.0 is false


def test_not_erase_changes_nothing_downstream():
    r = by_name("not_erase")
    assert r["verdict"] == [2, 1] and r["store"].kf_bad[1] is False and r["store"].kf_bad[2] is True
    # keyframe 1 still observes: keyframe 2 saw six others; without not_erase it would have seen five
    assert by_name("seven_both_culled")["verdict"] == [1, 1] and by_name("six_then_five")["verdict"] == [1, 0]


def test_the_cascade_depends_on_the_order():
    ab, ba = by_name("cascade_ab"), by_name("cascade_ba")
    assert ab["culled"] == [1, 2] and ba["culled"] == [1]              # B's verdict follows from whether A went first
    assert ab["bad_points"] == [200, 201] and ab["store"].pt_bad == {200, 201}
    assert all(p == -1 for p in ab["store"].rows[8])                   # cMapPoint::SetBadFlag nulled the entries of the remaining observer


def test_bad_points_order_and_state():
    r = by_name("bad_point_order_culled")
    assert r["bad_points"] == [302, 300, 301, 305, 304]
    assert CM.observations(r["store"], [300, 0]) == [0, 9]             # until the caller erases them the culled rows still count for OTHER calls
    st = CM.erase_culled(r["store"], r["culled"])
    assert CM.observations(st, [0, 300]) == [7, 0]


def test_three_observers_go_bad_four_do_not():
    r = by_name("three_observers_go_bad")
    assert r["bad_points"] == [100] and 101 not in r["store"].pt_bad


def test_map_point_culling_branches():
    rows, bad, cur, pts = CM.point_cases()
    st = CM.store_of(rows, bad)
    r = CM.map_point_culling(st, cur, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], [p[3] for p in pts])
    assert r["verdict"] == [p[4] for p in pts]
    assert set(r["verdict"]) == {0, 1, 2, 3, 4}
    assert r["remaining"] == [p[0] for p in pts if p[4] == 0]
    assert r["store"].pt_bad == {0, 2, 1} and st.pt_bad == {0}        # a deep copy
    assert CM.observations(r["store"], [1, 2, 3]) == [0, 0, 3]


def test_map_point_culling_boundaries():
    st = CM.store_of({1: [0, 1], 2: [0, 1], 3: [0]})                   # point 0: three observations, point 1: two
    run = lambda cur, p, f, v, first: CM.map_point_culling(st, cur, [p], [f], [v], [first])["verdict"][0]
    assert run(5, 1, 1, 1, 4) == 0 and run(5, 1, 1, 1, 3) == 3         # two observations: age 1 stays, age 2 goes bad
    assert run(5, 0, 1, 1, 3) == 0 and run(5, 0, 1, 1, 2) == 4         # three observations: age 2 stays, age 3 leaves
    assert run(5, 1, 1, 1, 6) == 3 and run(5, 0, 1, 1, 6) == 4         # first id above the current one: the unsigned difference wraps
    assert run(5, 0, 249, 1000, 5) == 2 and run(5, 0, 250, 1000, 5) == 0
    assert run(5, 0, 0, 0, 5) == 0 and run(5, 0, 7, 0, 5) == 0         # NaN and inf are not below a quarter
    assert run(0, 0, 1, 1, 0) == 0


def test_random_generator_is_not_vacuous_and_order_matters():
    st, octs = CM.random_cull_store(1, 24, 60)
    ids = sorted(st.rows)
    fwd = CM.keyframe_culling(st, octs, ids)
    CM.not_vacuous(fwd)
    rev = CM.keyframe_culling(st, octs, ids[::-1])
    assert dict(zip(ids, fwd["verdict"])) != dict(zip(ids[::-1], rev["verdict"]))
    assert isinstance(st, M.Store) and not st.pt_bad                   # the input is untouched
