"""Stores beyond 1024 keyframe slots for mcs_covis_* (DESIGN.md sections 4h and 4i), shared by tests/test_covis_tiles_cpu.py and tests/test_gpu_covis_tiles.py.
k_covis_local and k_covis_scan walk the slots 1024 at a time inside one workgroup and carry their state (base, wtot[16], best) from step to step in LDS,
k_covis_order ranks with strided loops over the slots, and mcs_covis_cull_keyframes sends its list to the device 128 entries per launch.  Rows here are short
(at most 46 features): the slot count is under test, not the row.

A case is a recipe (rows, poses, erased and bad keyframes, bad points) from which a covis_model.Store and a covis_pack.Both are built alike, with the model's
results computed ONCE per case and shared by both memory kinds and by the CPU test.  "Step" below is slot // 1024; slot k holds the keyframe kid_of(k)."""
import copy
import functools

import numpy as np

import covis_model as M
import cull_model as CM

STEP = 1024
SIZES = [1023, 1024, 1025, 2049, 3073]
HUB = 40                                   # points 0 .. 39: the frame's row, and what the keyframes share
ID0, ID_STEP = 7, 2


def kid_of(slot):
    return ID0 + ID_STEP * slot


def slot_of(kid):
    return (kid - ID0) // ID_STEP


def steps(S):
    return (S + STEP - 1) // STEP


class Case:
    """a recipe and what the model says about it"""


def apply(case, target):
    """replay the recipe on a covis_model.Store or a covis_pack.Both (same method names, except the flags)"""
    is_model = isinstance(target, M.Store)
    for k in range(case.S):
        target.set_keyframe(kid_of(k), case.rows[k])
    ids = [kid_of(k) for k in range(case.S)]
    if is_model:
        for k, t in zip(ids, case.poses):
            target.t[k] = tuple(float(v) for v in t)
    else:
        target.set_pose(ids, case.poses)
    for k in case.erased:
        target.erase(kid_of(k))
    for k in case.bad_slots:
        if is_model:
            target.kf_bad[kid_of(k)] = True
        else:
            target.set_bad(kid_of(k))
    if case.bad_points:
        if is_model:
            target.pt_bad |= set(case.bad_points)
        else:
            target.set_points_bad(sorted(case.bad_points))
    return target


def model_of(case):
    return apply(case, M.Store())


def both_of(case, pkg, G, device):
    from covis_pack import Both
    return apply(case, Both(pkg, G, case.S, case.max_feat, case.max_pts, device))


# ---------------------------------------------------------------------------------------------- section 1: hub stores of S slots
HUB_SIZES = [0, 3, 4, 5, 6, 29, 30, 31, 35]


def own(k):
    """the three points only keyframe k (and, for the first, its lower neighbour) holds"""
    return [HUB + 3 * k, HUB + 3 * k + 1, HUB + 3 * k + 2]


def hub_slots(S):
    """one keyframe per step holds the whole hub and is queried: the middle of a full step, the last slot of a short one"""
    return [min(s * STEP + 517, S - 1) for s in range(steps(S))]


@functools.lru_cache(maxsize=None)
def tile_case(S):
    """S keyframes over 40 hub points.  Every keyframe holds a random subset of the hub (so the frame's vote for it is that subset's size, give or take the
    frame's repeat and the bad hub point: around both thresholds, 4 / 5 and 29 / 30), three points of its own, one of its upper neighbour's, one NULL and one
    repeat, permuted.  Forced: the keyframes that are erased or bad would be local; slot 3 is not local and holds a point of the LAST step's hub keyframe."""
    rng = np.random.default_rng(9000 + S)
    c = Case()
    c.S, c.max_feat, c.max_pts = S, 48, HUB + 3 * S
    c.hubs = hub_slots(S)
    c.full_rows = sorted(c.hubs + [100])                          # slot 100 holds the whole hub too: the hub keyframes tie with each other across steps
    c.erased = [5, 700] + ([1023] if S in (1024, 1025) else []) + ([1024] if S >= 2049 else []) + ([2050] if S >= 3073 else [])
    c.bad_slots = [9, 1022] + ([1030, 2047] if S >= 2049 else []) + ([2049, 3000] if S >= 3073 else [])
    c.stray = 3                                                   # a keyframe of step 0 that is not local
    c.stray_point = own(c.hubs[-1])[2]
    c.rows = []
    for k in range(S):
        n = int(rng.choice(HUB_SIZES))
        if k in c.erased or k in c.bad_slots:
            n = 31
        if k == c.stray:
            n = 3
        hub = list(range(HUB)) if k in c.full_rows else [int(p) for p in rng.permutation(HUB)[:n]]
        row = hub + own(k) + [c.stray_point if k == c.stray and steps(S) > 1 else own((k + 1) % S)[0], -1]
        row.append(own(k)[2] if k in c.full_rows else row[int(rng.integers(0, len(row) - 1))])   # the repeat (a hub keyframe repeats a point of its own: its
        c.rows.append([int(row[i]) for i in rng.permutation(len(row))])                      # weights are the others' hub sizes exactly)
    c.poses = rng.normal(0, 2, (S, 3))
    c.bad_points = [HUB - 1] + [own(k)[1] for k in range(11, S, 97)]
    frame = list(range(HUB)) + [17, -1, HUB - 1]                  # the hub, one repeat, one NULL and the bad hub point once more
    c.frame = [int(frame[i]) for i in rng.permutation(len(frame))]
    c.frame_t = (0.25, -1.5, 0.75)
    st = model_of(c)
    obs = st.observers()
    c.ref = M.update_reference(st, c.frame, c.frame_t, obs)
    # the queries: the hub keyframe of every step, an ordinary keyframe of the first and one of the last full step or beyond
    c.queries = [kid_of(k) for k in c.hubs] + [kid_of(12), kid_of(S - 3)]
    c.conn = {q: M.update_connections(st, q, obs) for q in c.queries}
    c.batch = (c.queries[:steps(S)] + [kid_of(12), kid_of(S - 3)])[:3]   # three queries from as many steps as the store has
    # off[] of k_covis_scan at the first local slot of step 1 = the local points that the local keyframes of step 0 emit
    c.full = len(c.ref["local_points"])
    first1 = next((i for i, k in enumerate(c.ref["local_kfs"]) if slot_of(k) >= STEP), None)
    c.off_step1 = None if first1 is None else len(M.update_reference_points(st, c.ref["local_kfs"][:first1]))
    c.caps = [c.full, c.full - 1, 0] + ([] if c.off_step1 is None else [c.off_step1 - 1, c.off_step1, c.off_step1 + 1])
    return c


def emitters(st, local_kfs):
    """the local keyframes through which at least one point enters local_points, and point -> that keyframe"""
    via, marked = {}, set()
    for k in local_kfs:
        for p in st.rows[k]:
            if p >= 0 and p not in marked and p not in st.pt_bad:
                marked.add(p)
                via[p] = k
    return via


def cross_step_ties(res):
    """True if two entries of the ordered list carry the same weight and lie in different steps"""
    seen = {}
    for k, w in zip(res["ordered"], res["weights"]):
        seen.setdefault(w, set()).add(slot_of(k) // STEP)
    return any(len(v) > 1 for v in seen.values())


def assert_tile_case_does_its_job(c):
    """on the MODEL's output: the case reaches every step of every kernel it is there for"""
    S, st, ref = c.S, model_of(c), c.ref
    ns = steps(S)
    local_steps = [slot_of(k) // STEP for k in ref["local_kfs"]]
    assert set(local_steps) == set(range(ns)), "local keyframes in every step"
    assert len(st.rows) == S - len(c.erased) and sum(st.kf_bad.values()) == len(c.bad_slots)
    assert all(kid_of(k) not in ref["local_kfs"] for k in c.bad_slots)
    assert 0.5 * S < len(ref["local_kfs"]) < 0.8 * S
    if S >= 2049:
        assert len(ref["local_kfs"]) > STEP                       # the local rank itself passes 1024
    via = emitters(st, ref["local_kfs"])
    assert set(slot_of(k) // STEP for k in via.values()) == set(range(ns)), "every step emits local points"
    assert ref["frame_points"] != c.frame and ref["frame_points"].count(-1) == 3      # the bad hub point is nulled twice
    assert len(set(ref["weights"])) > 6 and len(ref["local_points"]) > S
    if ns > 1:
        p, holder = c.stray_point, kid_of(c.stray)
        assert p in st.rows[holder] and holder not in ref["local_kfs"] and slot_of(holder) < STEP
        assert slot_of(via[p]) >= (ns - 1) * STEP                 # enters through the last step, although a keyframe of step 0 holds it
        assert c.off_step1 is not None and 0 < c.off_step1 - 1 and c.off_step1 + 1 < c.full - 1
    assert ref["ref_kf"] == kid_of(100)                           # every hub keyframe has the greatest count: the first of them
    for q in c.queries:
        r = c.conn[q]
        others = set(slot_of(k) // STEP for k in st.rows if k != q)
        if slot_of(q) in c.hubs:
            assert len(r["ordered"]) > 0.2 * S and len(set(r["weights"])) <= 8
            if len(others) > 1:
                assert cross_step_ties(r), "equal weights in different steps"
    assert any(slot_of(q) >= STEP for q in c.queries) == (ns > 1)
    assert len(set(slot_of(q) // STEP for q in c.batch)) == min(ns, 3) and len(c.batch) == 3


# ---------------------------------------------------------------------------------------------- section 2: pinned slots, S = 2049
PIN_S = 2049
G_, H_, E_, BADP = 0, 1, 2, 3              # held by every slot; by slots 7 and 1030; by slot 2048; a bad point held by every slot
Q30, Q29, QMAX, QONE, QEMPTY = 1029, 100, 2000, 1022, 1600    # the slots of the query keyframes
PIN_BAD = 1200


def pa(k):
    """slot k's own point: a frame that holds it c times votes c for slot k alone"""
    return 10 + k


@functools.lru_cache(maxsize=None)
def pinned_case():
    c = Case()
    c.S, c.max_feat, c.max_pts = PIN_S, 32, 10 + PIN_S
    c.rows = []
    for k in range(PIN_S):
        row = [pa(k), G_, -1, pa(k), BADP] if k % 2 == 0 else [G_, BADP, pa(k), -1]
        if k in (7, 1030):
            row.append(H_)
        if k == PIN_S - 1:
            row.append(E_)
        if k == Q30:
            row = [G_] * 30 + [pa(k)]
        if k == Q29:
            row = [G_] * 29 + [pa(k)]
        if k == QMAX:
            row = [G_] * 10 + [H_] * 5 + [pa(k)]
        if k == QONE:
            row = [G_] * 29 + [E_, pa(k)]
        c.rows.append(row)
    rng = np.random.default_rng(77)
    c.poses = rng.normal(0, 1, (PIN_S, 3))
    c.erased, c.bad_slots, c.bad_points = [], [PIN_BAD], [BADP]
    return c


def votes(*pairs):
    """a frame row that votes `count` for slot `slot`, for every (slot, count)"""
    return [pa(k) for k, n in pairs for _ in range(n)]


def _k(*slots):
    return [kid_of(k) for k in slots]


LAST = PIN_S - 1
# update_reference on the pinned store: (name, frame row, the expected fields, stated by hand)
PINNED_FRAMES = [
    ("5_then_4_across_the_step", votes((1023, 5), (1024, 4)), dict(local_kfs=_k(1023), weights=[5], ref_kf=kid_of(1023))),
    ("4_then_5_across_the_step", votes((1023, 4), (1024, 5)), dict(local_kfs=_k(1024), weights=[5], ref_kf=kid_of(1024))),
    # the greatest count twice, in steps 1 and 2: the lower slot; slot 1200 has more votes but is bad
    ("tie_in_later_steps_below_a_bad_one", votes((10, 5), (PIN_BAD, 9), (1500, 7), (LAST, 7)),
     dict(local_kfs=_k(10, 1500, LAST), weights=[5, 7, 7], ref_kf=kid_of(1500))),
    ("maximum_in_the_last_slot", votes((10, 5), (1500, 7), (LAST, 8)), dict(local_kfs=_k(10, 1500, LAST), weights=[5, 7, 8], ref_kf=kid_of(LAST))),
    ("only_the_last_slot", votes((LAST, 5)), dict(local_kfs=_k(LAST), weights=[5], ref_kf=kid_of(LAST), local_points=[pa(LAST), G_, E_])),
    ("no_slot", votes((1023, 4), (1024, 4), (LAST, 4)), dict(local_kfs=[], weights=[], ref_kf=-1, local_points=[])),
]
# every slot local (with slot PIN_BAD good for the call): five votes for the point that every row holds.  The walk meets G_ in slot 0, H_ in slot 7 and E_ in
# slot QONE (before that row's own point); everything else is the slots' own points in order.
ALL_FRAME = [G_] * 5
ALL_POINTS = ([pa(0), G_] + [pa(k) for k in range(1, 8)] + [H_] + [pa(k) for k in range(8, QONE)] + [E_] + [pa(k) for k in range(QONE, PIN_S)])
EMPTY_ROW = [-1, BADP, pa(QEMPTY), -1]     # the row that QEMPTY holds for one query: NULLs, a bad point and a point nobody else holds


def pinned_connections(live):
    """update_connections on the pinned store, stated by hand: query slot -> (ordered ids, weights); `live` = the ids the store holds at the time"""
    others = sorted((k for k in live if k != kid_of(Q30)), reverse=True)
    return {
        Q30: (others, [30] * len(others)),                        # every other slot at exactly 30: all of them, by descending id
        Q29: (_k(0), [29]),                                       # every other slot at 29: the single fallback is the first
        QMAX: (_k(7) if kid_of(7) in live else _k(1030), [15]),   # the maximum below 30 in steps 0 and 1: the first that is there
        QONE: (_k(LAST), [30]),                                   # exactly one slot reaches 30, the last
    }


# ---------------------------------------------------------------------------------------------- section 3: culling at size
CULL_LIST_LENGTHS = [127, 128, 129, 257]
CHUNK = 128                                # mcs_covis_cull_keyframes: list entries per k_cull_put_list launch


@functools.lru_cache(maxsize=None)
def cull_list_case(n_list):
    """300 keyframes x 24 features (cull_model.random_cull_store) and a list of n_list permuted ids with not_erase on every fifth entry.  The 257-entry case
    holds keyframe id 0, listed at index 128."""
    c = Case()
    c.store, c.octaves = CM.random_cull_store(500 + n_list, 300, 24, id0=0 if n_list == 257 else 1)
    rng = np.random.default_rng(n_list)
    ids = [int(k) for k in rng.permutation(sorted(c.store.rows))]
    if n_list == 257:
        ids.remove(0)
        ids.insert(CHUNK, 0)
    c.ids = ids[:n_list]
    c.not_erase = [int(i % 5 == 4) for i in range(n_list)]
    c.want = CM.keyframe_culling(c.store, c.octaves, c.ids, c.not_erase)
    return c


def assert_cull_list_case_does_its_job(c):
    """a list of 129 has one entry in its second chunk, so it can show one verdict there: a culled keyframe.  The list of 257 shows verdicts 0, 1, 2 and 3
    beyond index 128 and has one entry in a third chunk."""
    CM.not_vacuous(c.want)
    v = c.want["verdict"]
    assert 2 in v
    if len(v) > CHUNK:
        assert 1 in v[CHUNK:], "a keyframe of the second chunk is culled"
    if len(v) == 257:
        assert 0 in v[CHUNK:] and 2 in v[CHUNK:] and v[CHUNK] == 3 and c.ids[CHUNK] == 0       # mnId == 0 is skipped (src/cLocalMapping.cpp:531)
        assert 1 in v[2 * CHUNK:] or 0 in v[2 * CHUNK:]                                        # and the one entry of the third chunk is judged


def clustered_cull_store(seed, S, n_feat=16, cluster=12):
    """-> (store, octaves): a store that keeps a share of its keyframes when every one is listed.  Keyframe slot k belongs to cluster k mod C (C = S / cluster
    clusters, so a cluster's members lie `C` slots apart, in every step); a cluster shares a pool of n_feat points, each member holding most of it.  A point
    stays redundant while five OTHER members observe it, so the chain culls a cluster down to about six members.  Per cluster a few "rare" points have exactly
    three observers: such a point goes bad with the first of them that is culled.  Octaves as in cull_model.random_cull_store: a base level per keyframe
    (mostly 3, some 1 or 6) with a spread of one level either way."""
    rng = np.random.default_rng(seed)
    C = max(1, S // cluster)
    members = [list(range(c, S, C)) for c in range(C)]
    rows = [None] * S
    octs = [None] * S
    for c, ms in enumerate(members):
        pool = c * 2 * n_feat + np.arange(n_feat)
        rare = c * 2 * n_feat + n_feat + np.arange(4)
        for k in ms:
            row = rng.permutation(pool)
            row[rng.random(n_feat) < 0.1] = -1
            rows[k] = row
        for p in rare:
            for k in rng.permutation(ms)[:3]:
                free = np.flatnonzero(np.isin(rows[k], pool) | (rows[k] < 0))
                rows[k][free[int(rng.integers(0, len(free)))]] = p
        for k in ms:
            base = int(rng.choice([3, 3, 3, 3, 1, 6]))
            octs[k] = np.clip(base + rng.integers(-1, 2, n_feat), 0, 7).astype(np.uint8).tolist()
    st, octaves = M.Store(), {}
    for k in range(S):
        st.set_keyframe(kid_of(k), rows[k])
        octaves[kid_of(k)] = octs[k]
    return st, octaves


@functools.lru_cache(maxsize=None)
def cull_tile_case(S):
    """S slots, a few erased and bad, two bad points; every live keyframe listed in a permuted order, not_erase on every seventh entry"""
    c = Case()
    c.S = S
    c.store, c.octaves = clustered_cull_store(4000 + S, S)
    c.erased = [kid_of(k) for k in (4, 1023, 1024)]
    c.bad_kfs = [kid_of(k) for k in (8, 1025, S - 1)]
    c.bad_points = [1, 40]
    st = copy.deepcopy(c.store)
    for k in c.erased:
        st.erase(k)
    for k in c.bad_kfs:
        st.kf_bad[k] = True
    st.pt_bad |= set(c.bad_points)
    c.before = st
    rng = np.random.default_rng(S)
    c.ids = [int(k) for k in rng.permutation(sorted(st.rows))]
    c.not_erase = [int(i % 7 == 3) for i in range(len(c.ids))]
    c.want = CM.keyframe_culling(st, {k: v for k, v in c.octaves.items() if k in st.rows}, c.ids, c.not_erase)
    return c


def bad_point_causes(c):
    """for every bad point of the call that had exactly three observers before it: the keyframe whose culling made it bad — the first culled observer in list
    order (src/cMapPoint.cpp:109: two are left)"""
    obs = c.before.observers()
    culled = set(c.want["culled"])
    out = {}
    for p in c.want["bad_points"]:
        if len(obs[p]) == 3 and p not in c.before.pt_bad:
            out[p] = next(k for k in c.ids if k in culled and k in obs[p])
    return out


def assert_cull_tile_case_does_its_job(c):
    CM.not_vacuous(c.want)
    v = dict(zip(c.ids, c.want["verdict"]))
    late = [k for k in c.ids if slot_of(k) >= STEP]
    assert sum(v[k] == 1 for k in late) > 10 and sum(v[k] == 0 for k in late) > 10 and any(v[k] == 2 for k in late)
    n1 = c.want["verdict"].count(1)
    assert 0.2 * c.S < n1 < 0.8 * c.S                           # a share is kept
    causes = bad_point_causes(c)
    assert sum(slot_of(k) >= STEP for k in causes.values()) > 5 and sum(slot_of(k) < STEP for k in causes.values()) > 5
    assert len(c.ids) > 8 * CHUNK and len(c.ids) % CHUNK != 0


def packed_halves_case():
    """-> (rows, octaves, listed ids, culled count): 1100 keyframes x 4 features; point 0 at level 0 and point 1 at level 1 in every row (the two halves of
    one packed 16-bit counter word), point 2 at level 2; odd slots hold point 3 (4 of 4 redundant: culled), even ones a point of their own (3 of 4: kept)."""
    rows = {kid_of(k): [0, 1, 2, 3 if k % 2 else 1000 + k] for k in range(1100)}
    octs = {k: [0, 1, 2, 2] for k in rows}
    listed = [kid_of(k) for k in range(900, 1100)]                # 200 entries: a second chunk, slots on either side of 1024
    return rows, octs, listed, 100
