"""The cases of mcs_covis_update_points, shared by tests/test_mappoints_cpu.py and tests/test_gpu_mappoints.py.  A case is a recipe —
keyframe rows, octaves, descriptors, poses, erased and bad keyframes, bad points — from which a mappoint_model.MapStore and a device store are built alike,
plus the calls (listed ids, positions, reference keyframes) made on it.  The model's answers are computed once per case and shared.

Rows are short (at most 46 features): what is under test is the number of slots, the length of a point's segment (its (keyframe, feature) entries) and the
length of the list."""
import functools

import numpy as np

import cull_model as CM
import covis_model as M
import mappoint_model as MM

NLEVELS = 8
SCALES = np.cumprod([1.0] + [float(np.float32(1.2))] * (NLEVELS - 1))      # mvScaleFactors of the reference's extractor (scaleFactor is a float)
STEP = 1024


class Case:
    """a recipe: kids (slot order), rows / octaves (None: never set) / desc / mask / poses per kid, erased, bad_kfs, bad_points, dim, masks, capacities"""


def random_descriptors(c, rng):
    c.desc = {k: rng.integers(0, 256, (len(c.rows[k]), c.dim), dtype=np.uint8) for k in c.kids}
    c.mask = {k: rng.integers(0, 256, (len(c.rows[k]), c.dim), dtype=np.uint8) for k in c.kids} if c.masks else None


def model_of(c):
    ms = MM.MapStore()
    for k in c.kids:
        ms.set_keyframe(k, c.rows[k])
        ms.s.t[k] = tuple(float(v) for v in c.poses[k])
        if c.octaves.get(k) is not None:
            ms.set_octaves(k, c.octaves[k])
        ms.set_descriptors(k, c.desc[k], c.mask[k] if c.masks else None)
    for k in c.erased:
        ms.erase(k)
    for k in c.bad_kfs:
        ms.s.kf_bad[k] = True
    ms.s.pt_bad |= set(c.bad_points)
    return ms


def device_of(c, FE, ctx, device=False):
    """the same recipe through frontend.cCovisibility (descriptors and octaves go in with the memory kind under test)"""
    st = FE.cCovisibility(len(c.kids), c.max_feat, c.max_pts, ctx=ctx)
    for k in c.kids:
        st.SetKeyFrame(k, c.rows[k])
        if c.octaves.get(k) is not None:
            st.SetOctaves(k, c.octaves[k], device=device)
        st.SetDescriptors(k, c.desc[k], c.mask[k] if c.masks else None, device=device)
    st.SetPose(c.kids, [c.poses[k] for k in c.kids])
    for k in c.erased:
        st.EraseKeyFrame(k)
    for k in c.bad_kfs:
        st.SetBadFlag(k)
    if c.bad_points:
        st.SetPointsBad(sorted(c.bad_points))
    return st


def start_desc(c, ids, seed=1):
    """the listed points' current descriptors (and masks): recognisable bytes that no keyframe row holds"""
    rng = np.random.default_rng(seed)
    d = rng.integers(0, 256, (len(ids), c.dim), dtype=np.uint8)
    d[:, 0] = 0xA5
    return d, (d ^ 0xFF if c.masks else None)


def run_model(c, ms, call, with_desc=True, max_points=None):
    ids, pos, ref = call
    d, m = start_desc(c, ids)
    return MM.update_points(ms, ids, pos, ref, SCALES, d if with_desc else None, m if with_desc else None, max_points)


# ---------------------------------------------------------------------------------------------- 1. the small store: one point per quirk
A, B, CB, D, E, FK, G = 3, 5, 8, 9, 12, 20, 21                   # CB and G are bad, E is erased, D never gets octaves
(P_N1, P_N2, P_N3, P_TWO, P_BADOBS, P_ALLBAD, P_NONE, P_BAD, P_REFNOT, P_REFERASED, P_REFBAD, P_TOP, P_OVER, P_NOOCT, P_CENTRE) = range(15)
SMALL_REF = {P_N1: A, P_N2: B, P_N3: FK, P_TWO: B, P_BADOBS: A, P_ALLBAD: CB, P_NONE: A, P_BAD: A, P_REFNOT: FK, P_REFERASED: E, P_REFBAD: CB, P_TOP: FK,
             P_OVER: FK, P_NOOCT: D, P_CENTRE: A}
SMALL_MAX_PTS = 40


@functools.lru_cache(maxsize=None)
def small_case(dim, masks):
    rng = np.random.default_rng(100 + dim + int(masks))
    c = Case()
    c.dim, c.masks, c.max_feat, c.max_pts = dim, masks, 12, SMALL_MAX_PTS
    c.kids = [A, B, CB, D, E, FK, G]
    c.rows = {A: [P_N1, P_N2, P_N3, P_TWO, P_BADOBS, P_BAD, P_REFNOT, P_REFERASED, P_REFBAD, P_CENTRE, -1],
              B: [P_N2, P_N3, P_TWO, P_BAD, P_TWO, P_REFNOT, P_CENTRE],          # P_TWO at features 2 and 4: two rows, one normal term
              CB: [P_BADOBS, P_ALLBAD, P_REFBAD, -1],
              D: [P_NOOCT, -1],
              E: [P_REFERASED, P_N1, P_N3],                                      # erased: observes nothing
              FK: [P_N3, P_BADOBS, P_TOP, P_OVER, -1, P_TOP],
              G: [P_ALLBAD]}
    c.octaves = {k: rng.integers(0, NLEVELS, len(c.rows[k])).tolist() for k in c.kids}
    c.octaves[D] = None
    c.octaves[FK] = [1, 3, NLEVELS - 1, NLEVELS + 1, 0, 2]                       # P_TOP: first at the top level, again at level 2; P_OVER beyond the table
    c.poses = {k: rng.normal(0, 2, 3) for k in c.kids}
    c.erased, c.bad_kfs, c.bad_points = [E], [CB, G], [P_BAD]
    random_descriptors(c, rng)
    # P_N3: rows (A, 2), (B, 1), (FK, 0) with d01 = d02 = d12 = 4 — every median equal: the strict '<' keeps row 0
    for (k, f), byte in (((A, 2), 0x00), ((B, 1), 0x0F), ((FK, 0), 0x33)):
        c.desc[k][f] = 0
        c.desc[k][f][0] = byte
        if masks:
            c.mask[k][f] = 0xFF
    ids = list(range(15))
    pos = rng.normal(0, 3, (15, 3))
    pos[P_CENTRE] = c.poses[B]                                                   # exactly on keyframe B's camera centre
    c.call = (ids, pos, [SMALL_REF[p] for p in ids])
    c.want = run_model(c, model_of(c), c.call)
    return c


def assert_small_case_does_its_job(c):
    """from the model's own decisions: every status, quirk and boundary of the small store is reached"""
    ms, w = model_of(c), c.want
    st = dict(zip(c.call[0], w["status"].tolist()))
    assert st[P_BAD] == 1 and st[P_REFERASED] == 2 and st[P_OVER] == 3 and sorted(set(st.values())) == [0, 1, 2, 3]
    assert all(st[p] == 0 for p in st if p not in (P_BAD, P_REFERASED, P_OVER))
    nd = dict(zip(c.call[0], w["n_desc"].tolist()))
    assert (nd[P_NONE], nd[P_N1], nd[P_N2], nd[P_N3]) == (0, 1, 2, 3) and nd[P_ALLBAD] == 0
    info = {p: MM.update_normal_and_depth(ms, p, c.call[1][i], c.call[2][i], SCALES)[1] for i, p in enumerate(c.call[0])}
    assert info[P_TWO]["n"] == 2 and nd[P_TWO] == 3                              # two features of one keyframe: two rows, one normal term
    assert MM.collect_rows(ms, P_TWO) == [(A, 3), (B, 2), (B, 4)]
    assert info[P_BADOBS]["n"] == 3 and nd[P_BADOBS] == 2                        # a bad observer: in the normal, not in the rows
    assert info[P_ALLBAD]["n"] == 2 and nd[P_ALLBAD] == 0 and not np.isnan(w["normal"][P_ALLBAD]).any()
    assert info[P_NONE]["n"] == 0 and info[P_NONE]["level"] == 1 and np.isnan(w["normal"][P_NONE]).all() and np.isfinite(w["min_dist"][P_NONE])
    assert info[P_REFNOT]["level"] == 1 and FK not in ms.observations(P_REFNOT)
    assert ms.s.kf_bad[CB] and info[P_REFBAD]["level"] == ms.octaves[CB][2] and info[P_ALLBAD]["level"] == ms.octaves[CB][1]
    assert info[P_TOP]["level"] == NLEVELS - 1                                   # reads scale_factors[0] for the far end
    top = np.float64(SCALES[-1]) * MM.cv_norm([np.float64(a) - np.float64(b) for a, b in zip(c.call[1][P_TOP], ms.s.t[FK])]) * np.float64(SCALES[0])
    assert w["max_dist"][P_TOP] == top
    assert D not in ms.octaves and info[P_NOOCT]["level"] == 0
    assert np.isnan(w["normal"][P_CENTRE]).all() and np.isfinite(w["max_dist"][P_CENTRE])
    # the tie: all three medians are 4
    rows = MM.collect_rows(ms, P_N3)
    mk = (lambda r: ms.mask[r[0]][r[1]]) if c.masks else (lambda r: None)
    d = [[MM.distance(ms.desc[a[0]][a[1]], ms.desc[b[0]][b[1]], mk(a), mk(b)) for b in rows] for a in rows]
    assert rows == [(A, 2), (B, 1), (FK, 0)] and d[0][1] == d[0][2] == d[1][2] == 4
    assert (w["best_kf"][P_N3], w["best_feat"][P_N3]) == (A, 2)
    # statuses 1 / 2 / 3 keep every sentinel; N = 0 keeps the descriptor but reads -1
    d0, m0 = start_desc(c, c.call[0])
    for p in (P_BAD, P_REFERASED, P_OVER):
        assert w["normal"][p].tolist() == [MM.SENTINEL["normal"]] * 3 and w["n_desc"][p] == MM.SENTINEL["n_desc"] and np.array_equal(w["desc"][p], d0[p])
    for p in (P_NONE, P_ALLBAD):
        assert np.array_equal(w["desc"][p], d0[p]) and w["best_kf"][p] == -1 and w["best_feat"][p] == -1
    assert all(not np.array_equal(w["desc"][p], d0[p]) for p in (P_N1, P_N2, P_N3, P_TWO, P_BADOBS))


# ---------------------------------------------------------------------------------------------- 2. segment lengths
SEG_LENGTHS = {1025: [63, 64, 65, 127, 128, 129, 1023, 1024, 1025], 2049: [129, 1025, 2049]}
ID0, ID_STEP = 4, 3


def kid_of(slot):
    return ID0 + ID_STEP * slot


@functools.lru_cache(maxsize=None)
def segment_case(S):
    """S slots; point i has exactly SEG_LENGTHS[S][i] (keyframe, feature) entries: its observers are spread over every 1024-slot step and two or more of them
    hold it at two features.  Slot 1023 is erased (and 1024 where the store goes on beyond it), keyframes of both steps are bad, the reference keyframe of every
    point is the last slot — bad but live in the 1025 store.  Camera centres of mixed magnitude (1e-2 .. 1e2)."""
    rng = np.random.default_rng(7000 + S)
    c = Case()
    c.S, c.dim, c.masks = S, (32 if S == 1025 else 16), S == 1025
    c.kids = [kid_of(k) for k in range(S)]
    holes = [1023] + ([1024] if S > 1025 else [])
    c.erased = [kid_of(k) for k in holes]
    c.ref_slot = S - 1
    bad = [9, 600, 1024] if S == 1025 else [9, 1022, 1030, 2040]
    c.bad_kfs = [kid_of(k) for k in bad]
    live = [k for k in range(S) if k not in holes]
    lengths = SEG_LENGTHS[S]
    held = {k: [] for k in range(S)}
    c.n_obs = []
    for i, L in enumerate(lengths):
        doubles = max(2, L - len(live))
        m = L - doubles
        assert doubles <= m <= len(live)
        forced = [0, c.ref_slot] + bad[:2]
        rest = [k for k in live if k not in forced]
        obs = forced + [int(k) for k in rng.permutation(rest)[:m - len(forced)]]
        twice = set(int(k) for k in rng.permutation(obs)[:doubles])
        for k in obs:
            held[k] += [i, i] if k in twice else [i]
        c.n_obs.append(m)
    c.rows, c.octaves, c.poses = {}, {}, {}
    for k in range(S):
        row = held[k] + [100 + k, -1]
        row = [int(row[j]) for j in rng.permutation(len(row))]
        c.rows[kid_of(k)] = row
        c.octaves[kid_of(k)] = rng.integers(0, NLEVELS, len(row)).tolist()
        c.poses[kid_of(k)] = rng.normal(0, 1, 3) * 10.0 ** int(rng.integers(-2, 3))
    c.max_feat, c.max_pts = max(len(r) for r in c.rows.values()), 100 + S
    assert c.max_feat <= 46
    c.bad_points = [100 + 17]
    random_descriptors(c, rng)
    order = [int(i) for i in rng.permutation(len(lengths))]
    ms = model_of(c)
    pos, ref = rng.normal(0, 5, (len(order), 3)), kid_of(c.ref_slot)
    for i, p in enumerate(order):                                 # a position at which the order of the sum shows in the bits (drawn again until it does)
        while normal_in_reverse(ms, p, pos[i]).tobytes() == np.array(MM.update_normal_and_depth(ms, p, pos[i], ref, SCALES)[1]["normal"]).tobytes():
            pos[i] = rng.normal(0, 5, 3)
    c.call = (order, pos, [ref] * len(order))
    c.want = run_model(c, ms, c.call)
    return c


def normal_in_reverse(ms, p, pos):
    """the same terms summed in DESCENDING slot order"""
    with np.errstate(all="ignore"):
        s = [np.float64(0.0)] * 3
        n = 0
        for k in reversed(list(ms.observations(p))):
            d = [np.float64(pos[j]) - np.float64(ms.s.t[k][j]) for j in range(3)]
            ia = np.float64(1.0) / MM.cv_norm(d)
            s = [s[j] + d[j] * ia for j in range(3)]
            n += 1
        ia = np.float64(1.0) / np.float64(n)
        return np.array([x * ia for x in s])


def assert_segment_case_does_its_job(c):
    ms, w = model_of(c), c.want
    lengths = SEG_LENGTHS[c.S]
    ids, pos, _ = c.call
    assert sorted(ids) == list(range(len(lengths))) and (w["status"] == 0).all()
    ref = kid_of(c.ref_slot)
    for i, p in enumerate(ids):
        obs = ms.observations(p)
        L = sum(len(v) for v in obs.values())
        assert L == lengths[p] and len(obs) == c.n_obs[p] and sum(len(v) == 2 for v in obs.values()) >= 2
        nbad = sum(len(v) for k, v in obs.items() if ms.s.kf_bad[k])
        assert nbad >= 2 and w["n_desc"][i] == L - nbad                         # bad observers in the segment, not among the rows
        steps = set((k - ID0) // ID_STEP // STEP for k in obs)
        assert steps == set(range((c.S + STEP - 1) // STEP)) and ref in obs     # observers in every step, the reference keyframe in the last
        assert (ref - ID0) // ID_STEP // STEP == max(steps)
        rev = normal_in_reverse(ms, p, pos[i])
        assert rev.tobytes() != w["normal"][i].tobytes(), "the order of the sum must show in the bits"
        assert np.allclose(rev, w["normal"][i], rtol=0, atol=1e-12)
    assert all(kid_of(k) not in ms.s.rows for k in ([1023] + ([1024] if c.S > 1025 else [])))
    assert ms.s.kf_bad[ref] == (c.S == 1025)
    assert len(set(w["best_kf"].tolist())) > 1


# ---------------------------------------------------------------------------------------------- 3. list lengths
LIST_LENGTHS = [1, 255, 256, 257]
LIST_POINTS = 520


@functools.lru_cache(maxsize=None)
def list_case():
    """45 keyframes of cull_model.random_cull_store (so that mcs_covis_cull_keyframes culls some of them) and 12 more over points 200 .. 519; lists of 1, 255,
    256 and 257 distinct ids out of [0, 520) — some of them observed by nobody — in descending and in shuffled order"""
    rng = np.random.default_rng(31)
    st, octs = CM.random_cull_store(17, 45, 44)
    c = Case()
    c.dim, c.masks = 32, True
    c.rows = {k: [int(p) for p in st.rows[k]] for k in st.rows}
    c.octaves = dict(octs)
    last = max(c.rows)
    for j in range(12):
        k = last + 2 + 2 * j
        row = rng.integers(200 + 25 * j, 245 + 25 * j, 30)
        row[rng.random(30) < 0.2] = -1
        c.rows[k] = [int(p) for p in row]
        c.octaves[k] = rng.integers(0, NLEVELS, 30).tolist()
    c.kids = sorted(c.rows)
    c.cull_list = sorted(st.rows)
    c.poses = {k: rng.normal(0, 2, 3) for k in c.kids}
    c.erased, c.bad_kfs, c.bad_points = [c.kids[7]], [c.kids[3], c.kids[50]], [5, 300]
    c.cull_list.remove(c.kids[7])
    c.max_feat, c.max_pts = 44, LIST_POINTS
    random_descriptors(c, rng)
    c.calls = {}
    for n in LIST_LENGTHS:
        for order in ("descending", "shuffled"):
            ids = [int(p) for p in rng.permutation(LIST_POINTS)[:n]]
            if order == "descending":
                ids.sort(reverse=True)
            obs_kids = [k for k in c.kids if k not in c.erased]
            c.calls[(n, order)] = (ids, rng.normal(0, 3, (n, 3)), [int(obs_kids[int(j)]) for j in rng.integers(0, len(obs_kids), n)])
    ms = model_of(c)
    c.want = {key: run_model(c, ms, call) for key, call in c.calls.items()}
    return c


def assert_list_case_does_its_job(c):
    for (n, order), (ids, _, _) in c.calls.items():
        assert len(ids) == n == len(set(ids))
        assert (ids == sorted(ids, reverse=True)) == (order == "descending" or n == 1)
    w = c.want[(257, "shuffled")]
    assert set(w["status"].tolist()) >= {0} and (w["n_desc"][w["status"] == 0] > 2).sum() > 50 and np.isnan(w["normal"]).any()
