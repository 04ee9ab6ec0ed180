"""Plain-Python restatement of the two reference functions behind mcs_covis_cull_keyframes / mcs_covis_cull_points:
    cLocalMapping::KeyFrameCulling        src/cLocalMapping.cpp:517-593
      cMultiKeyFrame::SetBadFlag          src/cMultiKeyFrame.cpp:574-670 (the observation part; spanning tree, map and database stay with the caller)
      cMapPoint::EraseAllObservations     src/cMapPoint.cpp:96-116
      cMapPoint::SetBadFlag               src/cMapPoint.cpp:185-204
    cLocalMapping::MapPointCulling        src/cLocalMapping.cpp:187-221
over a covis_model.Store, statement by statement, with the reference's line numbers, the sequential erasures included.  Every function works on a deep copy
of the store, which gains `octaves`: mnId -> GetKeyPoint(i).octave per feature (a keyframe without an entry reads level 0).

The store's assumption (covis_model.py) with its culling clause: point p is observed by exactly the live keyframes whose row holds p, and a keyframe's FIRST
observation of p (mit->second[0]) is the entry with the smallest feature index."""
import copy

import numpy as np

import covis_model as M

MAX_NR_OBS = 5                                                    # :522


class _Map:
    """the copy the functions work on: rows (mvpMapPoints), the points' mObservations, octaves"""

    def __init__(self, store, octaves):
        self.st = copy.deepcopy(store)
        self.st.octaves = {k: [int(o) for o in (octaves or {}).get(k, [0] * len(r))] for k, r in self.st.rows.items()}
        for k, r in self.st.rows.items():
            assert len(self.st.octaves[k]) == len(r), "one octave per feature"
        self.obs = {}                                             # p -> {mnId: [feature indices in AddObservation order]}; a bad point has none (:193)
        for k in sorted(self.st.rows):
            for i, p in enumerate(self.st.rows[k]):
                if p >= 0 and p not in self.st.pt_bad:
                    self.obs.setdefault(p, {}).setdefault(k, []).append(i)
        self.bad_points = []

    def point_set_bad(self, p):                                   # cMapPoint::SetBadFlag
        self.st.pt_bad.add(p)                                     # :191
        obs = self.obs.pop(p, {})                                 # :192-193
        for k in sorted(obs):                                     # :195
            for i in obs[k]:
                self.st.rows[k][i] = -1                           # :200 EraseMapPointMatch
        self.bad_points.append(p)

    def erase_all_observations(self, p, kf):                      # cMapPoint::EraseAllObservations
        bad = False
        o = self.obs.get(p)
        if o is not None and kf in o:                             # :101
            del o[kf]                                             # :103
            if len(o) <= 2:                                       # :109
                bad = True
        if bad:
            self.point_set_bad(p)                                 # :115


def keyframe_culling(store, octaves, kfs, not_erase=None):
    """-> dict(verdict, n_mps, n_redundant [per listed keyframe], bad_points (in the order they go bad), culled, to_be_erased, octave_rejects (features with
    Observations() > 3 and five or more other observers of which fewer than five pass the octave test), store (the copy afterwards: culled keyframes are bad
    and observe nothing any more, but stay in `rows` — the caller erases them))"""
    m = _Map(store, octaves)
    st = m.st
    assert len(set(kfs)) == len(kfs)
    verdict, n_mps, n_red, culled, tbe, octave_rejects = [], [], [], [], [], 0
    for idx, kf in enumerate(kfs):                                # :527
        if kf == 0:                                               # :531
            verdict.append(3); n_mps.append(0); n_red.append(0)
            continue
        row = list(st.rows[kf])                                   # :534 GetMapPointMatches
        nRedundantObservations, nMPs = 0, 0                       # :536-537
        for i in range(len(row)):                                 # :538
            p = row[i]
            if p < 0:                                             # :541
                continue
            if p in st.pt_bad:                                    # :543
                continue
            nMPs += 1                                             # :545
            observations = m.obs.get(p, {})
            if len(observations) > 3:                             # :548
                scaleLevel = st.octaves[kf][i]                    # :551
                nObs = 0                                          # :555
                for kfi in sorted(observations):                  # :557, address order -> id order (the break only fires once nObs >= 5 holds)
                    if kfi == kf:                                 # :561
                        continue
                    if len(observations[kfi]) > 0:                # :567
                        scaleLeveli = st.octaves[kfi][observations[kfi][0]]   # :571
                        if scaleLeveli <= scaleLevel + 1:         # :572
                            nObs += 1
                        if nObs >= MAX_NR_OBS:                    # :574
                            break
                if nObs >= MAX_NR_OBS:                            # :580
                    nRedundantObservations += 1
                elif len(observations) - (1 if kf in observations else 0) >= MAX_NR_OBS:
                    octave_rejects += 1
        n_mps.append(nMPs); n_red.append(nRedundantObservations)
        if nRedundantObservations > 0.9 * nMPs:                   # :589
            # cMultiKeyFrame::SetBadFlag; mnId == 0 cannot get here (:578)
            if not_erase is not None and not_erase[idx]:          # :580
                verdict.append(2); tbe.append(kf)                 # :582 mbToBeErased
                continue
            for i in range(len(st.rows[kf])):                     # :591
                if st.rows[kf][i] >= 0:                           # :592
                    m.erase_all_observations(st.rows[kf][i], kf)
            st.kf_bad[kf] = True                                  # :664
            verdict.append(1); culled.append(kf)
        else:
            verdict.append(0)
    return dict(verdict=verdict, n_mps=n_mps, n_redundant=n_red, bad_points=m.bad_points, culled=culled, to_be_erased=tbe, octave_rejects=octave_rejects,
                store=st)


def erase_culled(store, culled):
    """what the caller does with the verdict == 1 keyframes"""
    for k in culled:
        store.erase(k)
        store.octaves.pop(k, None)
    return store


def observations(store, ids):
    """cMapPoint::Observations() (src/cMapPoint.cpp:158-162) under the store's assumption; a bad point has none"""
    obs = store.observers()
    return [0 if int(p) in store.pt_bad else len(obs.get(int(p), [])) for p in ids]


def map_point_culling(store, current_kf, ids, found, visible, first_kf):
    """-> dict(verdict (the table of mcs_c.h: 1 bad, 2 found ratio, 3 few observations, 4 old enough, 0 stays), remaining, store (the copy afterwards))"""
    st = copy.deepcopy(store)
    nobs = dict(zip([int(p) for p in ids], observations(st, ids)))
    nCurrentKFid = int(current_kf) % (1 << 64)                    # :191 const unsigned long int
    verdict, remaining = [], []
    assert len(set(int(p) for p in ids)) == len(ids)
    for p, f, v, first in zip(ids, found, visible, first_kf):     # :192
        p = int(p)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.float64(int(f)) / np.float64(int(v))       # cMapPoint::GetFoundRatio: static_cast<double>(mnFound) / mnVisible
        d = (nCurrentKFid - int(first)) % (1 << 64)               # unsigned long - long
        if p in st.pt_bad:                                        # :195
            verdict.append(1)
        elif ratio < 0.25:                                        # :200
            st.pt_bad.add(p); nobs[p] = 0                         # :202
            verdict.append(2)
        elif d >= 2 and nobs[p] <= 2:                             # :206-207
            st.pt_bad.add(p); nobs[p] = 0                         # :209
            verdict.append(3)
        elif d >= 3:                                              # :213
            verdict.append(4)
        else:
            verdict.append(0); remaining.append(p)                # :219
    return dict(verdict=verdict, remaining=remaining, store=st)


# ---------------------------------------------------------------------------------------------- generators
def store_of(rows, bad_pts=(), bad_kfs=()):
    st = M.Store()
    for k in sorted(rows):
        st.set_keyframe(k, rows[k])
    st.pt_bad = set(bad_pts)
    for k in bad_kfs:
        st.kf_bad[k] = True
    return st


def random_cull_store(seed, n_kf, n_feat, extra_lens=(), top_level=7, id0=1, id_step=3, point0=0):
    """-> (store, octaves).  Two thirds of the keyframes ("dense") share a pool of n_feat points, each holding nine tenths of it, so that a dense point has more
    than five other observers until one or two dense keyframes are culled; a twentieth of every dense row comes from a pool of points with three or four
    observers (those go bad when an observer is culled).  The rest ("sparse") hold points of their own with few observers and are kept.  Octaves: a base level
    per keyframe (mostly 3, some 1 or 6: levels 0 .. 7 all occur) with a per-feature spread of one level either way, so that some features see observers two levels above them.  A tenth
    of the entries is NULL, a twentieth repeats another entry.  extra_lens: further keyframes of these row lengths over the dense pool."""
    rng = np.random.default_rng(seed)
    n_dense = max(2, (2 * n_kf + 2) // 3)
    dense_pool = point0 + np.arange(n_feat)
    rare_pool = point0 + n_feat + np.arange(max(4, n_feat // 3))
    sparse0 = point0 + n_feat + len(rare_pool)
    n_rare = max(1, n_feat // 20)
    rows, octs = [], []
    rare_obs = {int(p): 0 for p in rare_pool}
    for k in range(n_kf + len(extra_lens)):
        if k < n_dense:
            row = rng.permutation(dense_pool)[:n_feat]
            row[rng.random(n_feat) < 0.1] = -1
            free = [p for p in rare_pool if rare_obs[int(p)] < 3 + (int(p) & 1)]
            pick = rng.permutation(free)[:n_rare] if free else []
            for j, p in zip(rng.permutation(n_feat)[:len(pick)], pick):
                row[j] = p
                rare_obs[int(p)] += 1
        elif k < n_kf:
            row = sparse0 + rng.integers(0, 2 * n_feat, n_feat)
            row[rng.random(n_feat) < 0.1] = -1
        else:
            L = extra_lens[k - n_kf]
            row = rng.choice(dense_pool, L)
            row[rng.random(L) < 0.1] = -1
        n = len(row)
        rep = np.flatnonzero(rng.random(n) < 0.05)
        if len(rep) and k >= n_dense:
            row[rep] = row[rng.integers(0, n, len(rep))]
        elif len(rep):                                            # a dense row repeats dense points only: the observers of the rare ones stay as counted
            src = rng.integers(0, n, len(rep))
            ok = np.isin(row[rep], dense_pool) & np.isin(row[src], dense_pool)
            row[rep[ok]] = row[src[ok]]
        base = int(rng.choice([3, 3, 3, 3, 1, 6])) if top_level >= 7 else max(0, top_level - 1)
        o = np.clip(base + rng.integers(-1, 2, n), 0, top_level)
        rows.append(row.astype(np.int64)); octs.append(o.astype(np.uint8))
    order = rng.permutation(len(rows))                            # dense, sparse and extra keyframes interleave in id order
    st, octaves = M.Store(), {}
    for j, k in enumerate(order):
        kid = id0 + id_step * j
        st.set_keyframe(kid, rows[k])
        octaves[kid] = octs[k].tolist()
    return st, octaves


def not_vacuous(res):
    """what every randomised case asserts on the MODEL's result"""
    assert 1 in res["verdict"] and 0 in res["verdict"], res["verdict"]
    assert len(res["bad_points"]) > 0
    assert res["octave_rejects"] > 0


# ---------------------------------------------------------------------------------------------- hand-derived cases (tests/test_cull_cpu.py states what each shows)
def _obs_case(n_obs, level_of_others=0, own_level=0, n_feat_own=1):
    """keyframe 1 holds point 0 (n_feat_own times); keyframes 2 .. n_obs hold it too: Observations() == n_obs"""
    rows = {1: [0] * n_feat_own}
    octs = {1: [own_level] * n_feat_own}
    for k in range(2, n_obs + 1):
        rows[k] = [0]
        octs[k] = [level_of_others]
    return rows, octs


def hand_cases():
    """[(name, rows, octaves, bad points, listed keyframes, not_erase or None, expected dict of the fields worth stating)]"""
    C = []
    r, o = _obs_case(6)
    C.append(("five_others_cull", r, o, [], [1], None, dict(verdict=[1], n_mps=[1], n_redundant=[1], bad_points=[])))
    r, o = _obs_case(5)
    C.append(("four_others_keep", r, o, [], [1], None, dict(verdict=[0], n_mps=[1], n_redundant=[0])))
    # a point at two features counts twice and is judged per feature with that feature's octave: others at level 3; feature 0 at level 2 (3 <= 3 counts),
    # feature 1 at level 1 (3 <= 2 does not)
    r, o = _obs_case(6, level_of_others=3)
    r[1], o[1] = [0, 0], [2, 1]
    C.append(("two_features_two_octaves", r, o, [], [1], None, dict(verdict=[0], n_mps=[2], n_redundant=[1])))
    # Observations() exactly 3 is not examined, 4 is (with four observers nObs is 3 at most: examined but never redundant; so show it through 10 points)
    rows = {1: list(range(10))}
    octs = {1: [0] * 10}
    for k in range(2, 8):
        rows[k], octs[k] = list(range(10)), [0] * 10
    C.append(("ten_of_ten", rows, octs, [], [1], None, dict(verdict=[1], n_mps=[10], n_redundant=[10])))
    rows9 = {k: list(v) for k, v in rows.items()}
    for k in range(4, 8):
        rows9[k] = rows9[k][:9] + [-1]                            # point 9: observers 1, 2, 3 only -> Observations() == 3, not examined
    C.append(("nine_of_ten", rows9, octs, [], [1], None, dict(verdict=[0], n_mps=[10], n_redundant=[9])))
    rows20 = {k: list(range(20)) for k in range(1, 8)}
    octs20 = {k: [0] * 20 for k in range(1, 8)}
    for k in range(3, 8):
        rows20[k] = rows20[k][:19] + [-1]                         # point 19: observers 1, 2 -> not examined; 19 > 0.9 * 20 = 18.0
    C.append(("nineteen_of_twenty", rows20, octs20, [], [1], None, dict(verdict=[1], n_mps=[20], n_redundant=[19], bad_points=[19])))
    C.append(("no_points", {1: [-1, -1], 2: [0]}, {}, [], [1], None, dict(verdict=[0], n_mps=[0], n_redundant=[0])))
    # pKF itself is never counted, even when the feature under test is not its first entry of the point: five observers in all -> four others
    r, o = _obs_case(5)
    r[1], o[1] = [0, 0, 0], [0, 0, 0]
    C.append(("self_never_counts", r, o, [], [1], None, dict(verdict=[0], n_mps=[3], n_redundant=[0])))
    # an observer counts by its FIRST entry's octave only: observers hold the point twice, first at level 3, then at level 0; pKF's feature at level 1
    r, o = _obs_case(6)
    for k in range(2, 7):
        r[k], o[k] = [0, 0], [3, 0]
    o[1] = [1]
    C.append(("first_entry_octave", r, o, [], [1], None, dict(verdict=[0], n_redundant=[0])))
    o2 = {k: list(v) for k, v in o.items()}
    o2[1] = [2]                                                   # octave_j == octave + 1 counts
    C.append(("octave_plus_one", r, o2, [], [1], None, dict(verdict=[1], n_redundant=[1])))
    # the top level: octave + 1 == nlevels
    r, o = _obs_case(6, level_of_others=15, own_level=15)
    C.append(("top_level", r, o, [], [1], None, dict(verdict=[1], n_redundant=[1])))
    r, o = _obs_case(6, level_of_others=15, own_level=13)
    C.append(("top_level_rejects", r, o, [], [1], None, dict(verdict=[0], n_redundant=[0])))
    # mnId == 0 is skipped
    rows0 = {0: [0], 1: [0], 2: [0], 3: [0], 4: [0], 5: [0], 6: [0]}
    C.append(("id_zero_skipped", rows0, {}, [], [0, 1], None, dict(verdict=[3, 1], n_mps=[0, 1], n_redundant=[0, 1])))
    # not_erase: verdict 2, nothing changes downstream: [1, 2] on seven observers culls 1 and, with six left, 2 as well; under not_erase[0] keyframe 1 stays
    rows7 = {k: [0] for k in range(1, 8)}
    C.append(("seven_both_culled", rows7, {}, [], [1, 2], None, dict(verdict=[1, 1])))
    C.append(("not_erase", rows7, {}, [], [1, 2], [1, 0], dict(verdict=[2, 1], culled=[2], to_be_erased=[1])))
    rows6 = {k: [0] for k in range(1, 7)}
    C.append(("six_then_five", rows6, {}, [], [1, 2], None, dict(verdict=[1, 0], n_redundant=[1, 0])))
    # a point with 3 observers goes bad when one is culled, one with 4 does not: keyframe 1 holds 20 redundant points, point 100 (observers 1, 8, 9) and
    # point 101 (observers 1, 8, 9, 10)
    rowsb = {k: list(range(20)) for k in range(1, 8)}
    rowsb[1] = list(range(20)) + [100, 101]
    rowsb[8], rowsb[9], rowsb[10] = [100, 101], [101, 100], [101]
    C.append(("three_observers_go_bad", rowsb, {}, [], [1], None, dict(verdict=[1], n_mps=[22], n_redundant=[20], bad_points=[100])))
    # the cascade: keyframes 1 .. 7 observe points 0 .. 19 (B = 2 only 0 .. 8); points 200 and 201 have the observers A = 1, B = 2 and 8.
    # [A, B]: A is culled (20 of 22 redundant), 200 and 201 are left with two observers and go bad, B then counts nine points, each with five other observers
    # left: culled.  [B, A]: B counts eleven points of which nine are redundant (9 > 9.9 is false): kept; A is culled afterwards.
    rowsc = {k: list(range(20)) for k in range(1, 8)}
    rowsc[1] = list(range(20)) + [200, 201]
    rowsc[2] = list(range(9)) + [200, 201]
    rowsc[8] = [200, 201]
    C.append(("cascade_ab", rowsc, {}, [], [1, 2], None, dict(verdict=[1, 1], n_mps=[22, 9], n_redundant=[20, 9], bad_points=[200, 201])))
    C.append(("cascade_ba", rowsc, {}, [], [2, 1], None, dict(verdict=[0, 1], n_mps=[11, 22], n_redundant=[9, 20], bad_points=[200, 201])))
    # a bad point in a row is not counted and not erased (it does not appear in bad_points again)
    rowsd = {k: [0, 50] for k in range(1, 8)}
    C.append(("bad_point_in_row", rowsd, {}, [50], [1], None, dict(verdict=[1], n_mps=[1], n_redundant=[1], bad_points=[])))
    # the order of bad_points: keyframes in list order, within one by the feature index of the point's first entry (300 sits at features 1 and 4)
    rowsf = {k: list(range(40)) for k in range(1, 10)}
    rowsf[5] = [302, 300] + list(range(40)) + [301, 300]
    rowsf[3] = list(range(40)) + [305, 304]
    for p in (300, 301, 302, 304, 305):
        rowsf[20 + p] = [p]
        rowsf[400 + p] = [p]
    C.append(("bad_point_order_culled", rowsf, {}, [], [5, 3], None, dict(verdict=[1, 1], bad_points=[302, 300, 301, 305, 304])))
    return C


def point_cases():
    """MapPointCulling: (rows, bad points, current keyframe id, [(point, found, visible, first keyframe id, expected verdict)])"""
    rows = {1: [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 2: [0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 10], 3: [0, -1, 2, 3, 4, 5, 6, 7, 8, -1, 10]}
    cur = 10
    pts = [
        (0, 0, 10, 10, 1),      # bad first, whatever else holds
        (2, 24, 100, 10, 2),    # 0.24 < 0.25
        (3, 25, 100, 10, 0),    # 0.25 is not below; age 0
        (4, 0, 0, 9, 0),        # 0 / 0 = NaN: not below; age 1
        (5, 3, 0, 8, 0),        # 3 / 0 = inf: not below; age 2 with three observations: stays
        (1, 5, 10, 8, 3),       # age 2, two observations
        (9, 5, 10, 9, 0),       # age 1, one observation: too young for the test
        (6, 5, 10, 7, 4),       # age 3, three observations: leaves the list
        (7, 5, 10, 8, 0),       # age 2, three observations: stays
        (8, 5, 10, 11, 4),      # first id above the current one: the difference wraps, three observations -> leaves
        (10, 1, 4, 10, 0),      # exactly a quarter
    ]
    return rows, [0], cur, pts
