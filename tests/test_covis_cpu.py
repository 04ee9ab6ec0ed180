"""tests/covis_model.py against hand-derived cases of cTracking::UpdateReferenceKeyFrames / UpdateReferencePoints (src/cTracking.cpp:1024-1123) and
cMultiKeyFrame::UpdateConnections (src/cMultiKeyFrame.cpp:406-500).  Each case fails if the quirk it names is "fixed" in the model.  The same stores
and voters run on the device in tests/test_gpu_covis.py (covis_model.HAND_CASES)."""
import math

import covis_model as M


def store(rows, bad_points=(), bad_kfs=(), t=None):
    s = M.Store()
    for k in sorted(rows):
        s.set_keyframe(k, rows[k])
    s.pt_bad = set(bad_points)
    for k in bad_kfs:
        s.kf_bad[k] = True
    for k, v in (t or {}).items():
        s.t[k] = tuple(v)
    return s


def test_a_point_at_two_voter_features_votes_twice():
    s = store({1: [0, 1, 2]})
    r = M.update_reference(s, [0, 0, 1, 1, 2], (0, 0, 0))          # 5 features, 3 distinct points: count 5 > 4
    assert r["local_kfs"] == [1] and r["weights"] == [5] and r["ref_kf"] == 1
    assert M.update_reference(s, [0, 1, 2, -1, -1], (0, 0, 0))["local_kfs"] == []   # once each: 3
    s = store({1: [0, 0, 0], 2: [0]})
    assert M.update_connections(s, 1)["counter"] == {2: 3}        # :419-441 run per feature too


def test_a_point_at_two_keyframe_features_counts_that_keyframe_once():
    s = store({1: [0, 0, 0, 0, 0, 1]})
    r = M.update_reference(s, [0, 1], (0, 0, 0))
    assert r["local_kfs"] == []                                    # observations holds keyframe 1 once per point: count 2, not 6
    s = store({1: [7], 2: [7, 7, 7]})
    assert M.update_connections(s, 1)["counter"] == {2: 1}


def test_bad_voter_points_are_nulled_in_place_and_do_not_vote():
    s = store({1: [0, 1, 2, 3, 4, 5]}, bad_points=[5])
    r = M.update_reference(s, [0, 1, 2, 3, 5, -1, 5], (0, 0, 0))
    assert r["frame_points"] == [0, 1, 2, 3, -1, -1, -1] and r["local_kfs"] == []   # 4 votes
    r = M.update_reference(s, [0, 1, 2, 3, 4, 5], (0, 0, 0))
    assert r["weights"] == [5] and r["local_points"] == [0, 1, 2, 3, 4]             # the bad point is not a local point either (:1042)
    # UpdateConnections copies the row (:414): nothing is nulled, the bad point is only skipped
    s = store({1: [0, 5], 2: [0, 5]}, bad_points=[5])
    assert M.update_connections(s, 1)["counter"] == {2: 1} and s.rows[1] == [0, 5]


def test_local_threshold_is_count_above_four():
    s = store({1: [0, 1, 2, 3], 2: [0, 1, 2, 3, 4]})
    r = M.update_reference(s, [0, 1, 2, 3, 4], (0, 0, 0))
    assert r["local_kfs"] == [2] and r["weights"] == [5] and r["ref_kf"] == 2       # 4 is out, 5 is in


def test_connection_threshold_is_count_at_least_thirty():
    pts = list(range(30))
    s = store({1: pts, 2: pts[:29], 3: pts})
    r = M.update_connections(s, 1)
    assert r["counter"] == {2: 29, 3: 30} and r["ordered"] == [3] and r["weights"] == [30]


def test_reference_keyframe_tie_goes_to_the_lower_id():
    s = store({4: [0, 1, 2, 3, 4], 9: [0, 1, 2, 3, 4], 11: [0, 1, 2, 3, 4, 5]})
    assert M.update_reference(s, [0, 1, 2, 3, 4], (0, 0, 0))["ref_kf"] == 4        # :1103 is a strict >
    assert M.update_reference(s, [0, 1, 2, 3, 4, 5], (0, 0, 0))["ref_kf"] == 11
    assert M.update_reference(s, [0, 1], (0, 0, 0))["ref_kf"] == -1                # no local keyframe: NULL


def test_fallback_to_the_single_maximum():
    s = store({1: [0, 1, 2, 3], 2: [0, 1], 3: [2, 3], 4: [9]})
    r = M.update_connections(s, 1)
    assert r["counter"] == {2: 2, 3: 2} and r["ordered"] == [2] and r["weights"] == [2]   # first of the maximum, :457 is a strict >


def test_empty_counter_leaves_the_lists_unchanged():
    s = store({1: [0, 1], 2: [2, 3], 3: [-1, -1]})
    assert M.update_connections(s, 1) == dict(counter={}, ordered=None, weights=None)
    assert M.update_connections(s, 3)["ordered"] is None


def test_equal_weights_order_by_descending_id():
    pts = list(range(31))
    s = store({1: pts, 2: pts[:30], 5: pts, 7: pts[:30], 8: pts[1:]})
    r = M.update_connections(s, 1)
    assert r["ordered"] == [5, 8, 7, 2] and r["weights"] == [31, 30, 30, 30]        # sort ascending (weight, key), then push_front


def test_first_occurrence_order_across_keyframes():
    s = store({1: [5, 3, -1, 5, 1, 0, 2], 2: [9, 3, 8, 0, 1, 2, 7, 5]})
    r = M.update_reference(s, [0, 1, 2, 3, 5], (0, 0, 0))
    assert r["local_kfs"] == [1, 2]                                                # 5 and 5 votes
    assert r["local_points"] == [5, 3, 1, 0, 2, 9, 8, 7]


def test_a_bad_keyframe_is_not_local_but_still_counts_as_a_connection():
    pts = list(range(30))
    s = store({1: pts, 2: pts, 3: pts[:6]}, bad_kfs=[2])
    r = M.update_reference(s, pts[:6], (0, 0, 0))
    assert r["local_kfs"] == [1, 3] and r["ref_kf"] == 1
    assert M.update_connections(s, 1)["ordered"] == [2]                            # no isBad() on the keyframe side of UpdateConnections
    s = store({1: pts[:5], 2: pts[:6]}, bad_kfs=[2])
    assert M.update_reference(s, pts[:6], (0, 0, 0))["ref_kf"] == 1                # a bad keyframe cannot be the reference either (:1100 precedes :1103)


def test_distance_is_the_cv_norm_sum():
    s = store({1: [0, 1, 2, 3, 4]}, t={1: (0.1, 0.2, 0.3)})
    r = M.update_reference(s, [0, 1, 2, 3, 4], (1.0, 2.0, 3.0))
    dx, dy, dz = 1.0 - 0.1, 2.0 - 0.2, 3.0 - 0.3
    assert r["dists"] == [math.sqrt(((0.0 + dx * dx) + dy * dy) + dz * dz)]


def test_erased_keyframes_observe_nothing():
    s = store({1: [0, 1, 2, 3, 4], 2: [0, 1, 2, 3, 4]})
    s.erase(1)
    r = M.update_reference(s, [0, 1, 2, 3, 4], (0, 0, 0))
    assert r["local_kfs"] == [2] and s.holes == 1


def test_observers_is_observations_for_every_point():
    s = M.random_store(3, 12, 40, 150)
    obs = s.observers()
    for p in range(150):
        assert obs.get(p, []) == s.observations(p)
