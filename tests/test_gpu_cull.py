"""-m gpu: mcs_covis_set_keyframe_octaves / _cull_keyframes / _observations / _cull_points (cLocalMapping::KeyFrameCulling, src/cLocalMapping.cpp:517-593, with
the erasures of cMultiKeyFrame::SetBadFlag; cLocalMapping::MapPointCulling, :187-221) against tests/cull_model.py, host kind and device kind, bit for bit:
everything compared is an integer.  After every call the store's state is read back through mcs_covis_observations and a following mcs_covis_update_reference
(tests/cull_pack.py).  The shapes are the smallest at which the kernels can go wrong: rows around the 16-byte load (4 entries), the wave (64) and the chain's
workgroup stride (1024); 1, 2 and 33 listed keyframes; slots around the wave-per-slot grid (4 per workgroup) and 64; point ids beyond 16 bits; more than 255
observers at one level; both counter widths.

Every randomised case asserts on the MODEL's result that a keyframe is culled and one is kept, that a point goes bad and that a feature is rejected by the
octave test alone (cull_model.not_vacuous).  The exception is stated where it applies: a store of fewer than six live keyframes cannot cull at all, because a
redundant feature needs five OTHER observers (nObs >= 5, :580)."""
import importlib

import numpy as np
import pytest

import covis_model as M
import cull_model as CM
from cull_pack import CullBoth

pytestmark = pytest.mark.gpu
KINDS = [False, True]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return importlib.import_module("multicol-slam_amd"), G


def max_point(st):
    return max([p for r in st.rows.values() for p in r] + list(st.pt_bad) + [0])


def row_length_store(L):
    """20 keyframes x L features; below 63 features the generator's proportions do not hold, so 20 x 40 plus three keyframes of L features"""
    return CM.random_cull_store(1000 + L, 20, L) if L >= 63 else CM.random_cull_store(1000 + L, 20, 40, extra_lens=(L, L, L))


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("L", [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_row_lengths_two_calls_and_a_shorter_row(env, L, device):
    pkg, G = env
    st, octs = row_length_store(L)
    assert set(o for v in octs.values() for o in v) == set(range(8))              # octaves over all of 0 .. 7
    b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
    rng = np.random.default_rng(L)
    ids = [int(k) for k in rng.permutation(sorted(st.rows))]
    first = b.check_cull(ids[:len(ids) // 2], where="first")
    CM.not_vacuous(first)
    # a second call on the same store: the scratch (marks, counters) must be clean, the flags of the first call must hold
    rest = [k for k in ids if k in b.m.rows]
    b.check_cull(rest[::-1], where="second")
    # a row replaced by a shorter one: its octaves read 0 until they are set again; the old tail must not count
    k = max(b.m.rows, key=lambda q: len(b.m.rows[q]))
    short = [p for p in st.rows[k] if p not in b.m.pt_bad][:max(1, len(st.rows[k]) // 2)] or [-1]
    b.set_keyframe(k, short)
    b.check_observations(where="shorter row")
    b.check_cull([q for q in sorted(b.m.rows)], where="level 0")
    if k in b.m.rows:
        b.set_octaves(k, octs[k][:len(short)])
        b.check_cull([q for q in sorted(b.m.rows)][::-1], where="octaves again")


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n_list", [1, 2, 33])
def test_listed_keyframes(env, n_list, device):
    pkg, G = env
    st, octs = CM.random_cull_store(33, 40, 48)
    ids = sorted(st.rows)
    full = CM.keyframe_culling(st, octs, ids)
    b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
    if n_list == 33:
        CM.not_vacuous(b.check_cull(ids[:33]))
        return
    # one or two listed keyframes cannot show a culled and a kept keyframe, bad points and an octave reject in one call: the calls of the case do together
    culled, kept = full["culled"][0], next(k for k, v in zip(ids, full["verdict"]) if v == 0 and k > full["culled"][0])
    lists = [[culled], [kept]] if n_list == 1 else [[kept, culled]]
    res = [b.check_cull(l) for l in lists]
    assert [v for r in res for v in r["verdict"]].count(1) == 1 and [v for r in res for v in r["verdict"]].count(0) == 1
    assert sum(len(r["bad_points"]) for r in res) > 0 and sum(r["octave_rejects"] for r in res) > 0


def test_the_order_of_the_list_decides(env):
    pkg, G = env
    st, octs = CM.random_cull_store(3, 24, 60)
    ids = sorted(st.rows)
    fwd, rev = CM.keyframe_culling(st, octs, ids), CM.keyframe_culling(st, octs, ids[::-1])
    assert dict(zip(ids, fwd["verdict"])) != dict(zip(ids[::-1], rev["verdict"]))  # checked on the model: the cascade is real in this store
    for order in (ids, ids[::-1]):
        for device in KINDS:
            CM.not_vacuous(CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1).check_cull(order))


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("S", [1, 4, 5, 64, 65])
def test_slot_counts_with_holes_and_a_bad_observer(env, S, device):
    pkg, G = env
    st, octs = CM.random_cull_store(300 + S, S, 40)
    b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
    ids = sorted(st.rows)
    if S > 5:
        for k in ids[3::9]:
            b.erase(k)
        b.set_bad(sorted(b.m.rows)[2])                                             # a bad keyframe still observes: the reference has no test there
        b.set_points_bad(b.points()[5:7])
    assert b.d.slots() == S and b.d.size() == len(b.m.rows)
    live = [int(k) for k in np.random.default_rng(S).permutation(sorted(b.m.rows))]
    not_erase = [int(i % 5 == 1) for i in range(len(live))]
    w = b.check_cull(live, not_erase)
    if S > 5:
        CM.not_vacuous(w)
        assert 2 in w["verdict"]
        assert ids[-1] in live and b.d.slots() == S                                # the last slot (slot 64 of 65: a second workgroup of the wave-per-slot grid)
    else:
        # fewer than six live keyframes: no feature has five other observers, nothing can be culled (see the module's docstring); the counters are still checked
        assert set(w["verdict"]) == {0} and sum(w["n_mps"]) > 0 and sum(w["n_redundant"]) == 0
    b.check_cull(sorted(b.m.rows))


@pytest.mark.parametrize("device", KINDS)
def test_point_ids_beyond_16_bits_and_the_top_level(env, device):
    pkg, G = env
    st, octs = CM.random_cull_store(5, 20, 64, point0=66000)
    octs = {k: [o + 8 for o in v] for k, v in octs.items()}                        # levels 8 .. 15: octave + 1 == MCS_MAX_LEVELS at the top
    assert max(o for v in octs.values() for o in v) == 15                          # MCS_MAX_LEVELS - 1
    b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
    w = b.check_cull(sorted(st.rows))
    CM.not_vacuous(w)
    assert min(w["bad_points"]) > 65536


@pytest.mark.parametrize("max_kf", [300, 65536])
def test_more_than_255_observers_at_one_level(env, max_kf):
    """300 keyframes x 4 features observe points 0, 1, 2 at level 2: a counter narrower than 9 bits wraps.  max_kf = 65536 runs the same through the 32-bit
    counters of a store with 65 536 slots or more.  Even keyframes hold a point of their own (3 of 4 redundant: kept), odd ones point 3 (4 of 4: culled)."""
    pkg, G = env
    rows = {k + 1: [0, 1, 2, 3 if k % 2 else 1000 + k] for k in range(300)}
    octs = {k: [2, 2, 2, 2] for k in rows}
    st = CM.store_of(rows)
    listed = list(range(100, 133))
    want = CM.keyframe_culling(st, octs, listed)
    assert want["verdict"].count(1) == 17 and want["verdict"].count(0) == 16 and want["n_redundant"][:2] == [4, 3]
    for device in KINDS:
        b = CullBoth.of(pkg, G, st, octs, device, max_kf=max_kf, max_feat=4, max_pts=1400)
        assert b.d.observations([0, 3, 1000, 1399]) == [300, 150, 1, 0]
        b.check_cull(listed)
        assert b.d.observations([0, 3]) == [300 - 17, 150 - 17]


@pytest.mark.parametrize("device", KINDS)
def test_cap_below_at_and_above_the_bad_points(env, device):
    pkg, G = env
    st, octs = CM.random_cull_store(21, 20, 40)
    ids = sorted(st.rows)
    full = len(CM.keyframe_culling(st, octs, ids)["bad_points"])
    assert full > 3
    for cap in (full + 5, full, full - 1, 1, 0):
        b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
        w = b.check_cull(ids, cap=cap)                                             # n_bad_points reports the FULL count; every bad point is flagged whatever cap
        CM.not_vacuous(w)


HAND = CM.hand_cases()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_cases(env, case):
    pkg, G = env
    name, rows, octs, bad, kfs, ne, want = case
    for device in KINDS:
        b = CullBoth.of(pkg, G, CM.store_of(rows, bad), octs, device)
        w = b.check_cull(kfs, ne, where=name)
        for k, v in want.items():
            assert w[k] == v, (name, k)


@pytest.mark.parametrize("device", KINDS)
def test_octave_rows(env, device):
    pkg, G = env
    r, o = CM._obs_case(6, level_of_others=3, own_level=1)
    b = CullBoth.of(pkg, G, CM.store_of(r), o, device, max_feat=4)
    assert b.check_cull([1], erase=False)["verdict"] == [0]                        # 3 <= 1 + 1 is false
    assert b.d.set_octaves(1, [2, 2]) == -1 and b.d.set_octaves(99, [2]) == -1     # one octave per feature of a live keyframe
    assert b.d.set_octaves(1, [16]) == (0 if device else -1)                       # host kind refuses, device kind clamps to MCS_MAX_LEVELS - 1
    if device:
        b.m.octaves[1] = [15]
    b.check_cull([1], erase=False)
    b.set_octaves(1, [2])
    b.set_keyframe(1, [0])                                                         # the same length: the octaves stay
    assert b.m.octaves[1] == [2] and b.check_cull([1], erase=False)["verdict"] == [1]
    b.set_bad(1, False)
    b.set_keyframe(1, [0, 0])                                                      # another length: level 0 again
    assert b.check_cull([1], erase=False)["verdict"] == [0]
    # a keyframe whose octaves were never set reads level 0, also in a slot that held another keyframe's octaves before mcs_covis_clear
    assert b.d.L.mcs_covis_clear(b.d.h) == 0
    b.d.slot_ids = []
    b.m = M.Store()
    b.m.octaves = {}
    for k in range(1, 7):
        b.set_keyframe(k, [0])
    assert b.check_cull([1])["verdict"] == [1]


def test_refusals_change_nothing(env):
    pkg, G = env
    st, octs = CM.random_cull_store(21, 20, 40)
    ids = sorted(st.rows)
    b = CullBoth.of(pkg, G, st, octs, False, max_pts=max_point(st) + 1)
    L, cap = pkg.lib(), pkg._capi
    o = np.zeros(64, np.int32)
    p = o.ctypes.data

    def call(lst):
        a = np.array(lst, np.int64)
        return L.mcs_covis_cull_keyframes(b.d.h, len(a), a.ctypes.data, None, 8, 0, p, p, p, p, p)
    assert call([ids[0], 999]) == cap.MCS_ERR_INVALID and call([ids[0], ids[1], ids[0]]) == cap.MCS_ERR_INVALID
    b.erase(ids[4])
    assert call([ids[4]]) == cap.MCS_ERR_INVALID                                   # an erased keyframe is not live
    pts = np.array([1, 1], np.int32)
    z4, z8 = np.ones(2, np.int32), np.zeros(2, np.int64)
    assert L.mcs_covis_cull_points(b.d.h, 5, 2, pts.ctypes.data, z4.ctypes.data, z4.ctypes.data, z8.ctypes.data, 0, p) == cap.MCS_ERR_INVALID   # a repeat
    pts[1] = max_point(st) + 1
    assert L.mcs_covis_cull_points(b.d.h, 5, 2, pts.ctypes.data, z4.ctypes.data, z4.ctypes.data, z8.ctypes.data, 0, p) == cap.MCS_ERR_INVALID
    assert L.mcs_covis_observations(b.d.h, pts.ctypes.data, 2, 0, p) == cap.MCS_ERR_INVALID
    assert L.mcs_ctx_set_async_search(G.ctx().h, 1) == 0
    try:
        assert call(ids[:2]) == cap.MCS_ERR_UNSUPPORTED
        pts[1] = 2
        assert L.mcs_covis_cull_points(b.d.h, 5, 2, pts.ctypes.data, z4.ctypes.data, z4.ctypes.data, z8.ctypes.data, 0, p) == cap.MCS_ERR_UNSUPPORTED
        assert L.mcs_covis_observations(b.d.h, pts.ctypes.data, 2, 0, p) == cap.MCS_ERR_UNSUPPORTED
    finally:
        assert L.mcs_ctx_set_async_search(G.ctx().h, 0) == 0
    assert call([]) == 0 and o[0] == 0                                              # an empty list: no bad points
    b.check_observations()
    CM.not_vacuous(b.check_cull(sorted(b.m.rows)))


# ---------------------------------------------------------------------------------------------- MapPointCulling
def recent_points(b, n, seed, cur):
    """n distinct recent points with counters and first keyframes around every boundary of the table"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(b.points())[:n].astype(np.int32)
    assert len(ids) == n
    visible = rng.integers(0, 9, n).astype(np.int32)
    found = np.minimum(rng.integers(0, 9, n), np.maximum(visible, 1)).astype(np.int32)
    first = (cur - rng.integers(-1, 5, n)).astype(np.int64)
    return ids, found, visible, first


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_cull_points(env, n, device):
    pkg, G = env
    st, octs = CM.random_cull_store(40 + n, 20, 150)
    b = CullBoth.of(pkg, G, st, octs, device, max_pts=max_point(st) + 1)
    b.set_points_bad(b.points()[::6])
    cur = sorted(st.rows)[-1]
    ids, found, visible, first = recent_points(b, n, n, cur)
    w = b.check_cull_points(cur, ids, found, visible, first)
    if n > 1:
        assert set(w["verdict"]) == {0, 1, 2, 3, 4}                                # all five branches in one call
        gone = [int(p) for p, v in zip(ids, w["verdict"]) if v in (1, 2, 3)]
        assert gone and b.d.observations(gone) == [0] * len(gone)                  # the flags are in the store
    # a second call on what remains: the first call's flags hold, its scratch is clean
    w2 = b.check_cull_points(cur + 1, w["remaining"] + [int(ids[0])], [1] * (len(w["remaining"]) + 1), [2] * (len(w["remaining"]) + 1),
                             [cur] * (len(w["remaining"]) + 1)) if w["remaining"] and int(ids[0]) not in w["remaining"] else None
    assert w2 is None or len(w2["verdict"]) == len(w["remaining"]) + 1
    b.check_reference(np.array(ids[:200], np.int32), (0, 0, 0))
    b.check_cull(sorted(b.m.rows))                                                 # and KeyFrameCulling sees the points that MapPointCulling made bad


def test_cull_points_hand_cases_and_repeats(env):
    pkg, G = env
    rows, bad, cur, pts = CM.point_cases()
    for device in KINDS:
        b = CullBoth.of(pkg, G, CM.store_of(rows, bad), {}, device)
        w = b.check_cull_points(cur, [p[0] for p in pts], [p[1] for p in pts], [p[2] for p in pts], [p[3] for p in pts])
        assert w["verdict"] == [p[4] for p in pts]
    # device kind: both copies of a repeated point get the verdict of the FIRST (here 2: found ratio), though the second copy's own counters say "stays"
    b = CullBoth.of(pkg, G, CM.store_of(rows, bad), {}, True)
    assert b.d.cull_points(cur, [3, 7, 3], [1, 5, 5], [10, 10, 10], [10, 10, 10]) == [2, 0, 2]
    assert b.d.observations([3, 7]) == [0, 3]
    # an id outside [0, max_points) reads as a bad point
    assert b.d.cull_points(cur, [7, 5000, -1], [5, 5, 5], [10, 10, 10], [10, 10, 10]) == [0, 1, 1] and b.d.observations([7, 5000, -1]) == [3, 0, 0]
