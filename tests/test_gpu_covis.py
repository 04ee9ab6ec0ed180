"""-m gpu: mcs_covis_update_reference / mcs_covis_update_connections (cTracking::UpdateReferenceKeyFrames + UpdateReferencePoints, src/cTracking.cpp:1024-1123;
cMultiKeyFrame::UpdateConnections, src/cMultiKeyFrame.cpp:406-500) against tests/covis_model.py, host-kind and device-kind, bit for bit: every output is an
integer except local_dist, which is + - * and sqrt only.  The shapes are the smallest at which the kernels can go wrong: rows around the wave (64) and the
16-byte load (4 entries), slots around the wave-per-slot grid (4 slots per workgroup) and the 64-slot ballot, point ids beyond 16 bits."""
import importlib

import numpy as np
import pytest

import covis_model as M
from covis_pack import Both, Dev

pytestmark = pytest.mark.gpu
KINDS = [False, True]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return importlib.import_module("multicol-slam_amd"), G


def voter(rng, store, n, n_points, lo=0):
    """a frame row of n features: points of the store's range, 30 % NULL, some repeated"""
    row = rng.integers(lo, max(n_points, lo + 1), n)
    row[rng.random(n) < 0.3] = -1
    rep = np.flatnonzero(rng.random(n) < 0.1)
    if len(rep):
        row[rep] = row[rng.integers(0, n, len(rep))]
    return row.astype(np.int32)


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n_feat", [1, 63, 64, 65, 255, 256, 1025])
def test_row_lengths(env, n_feat, device):
    pkg, G = env
    n_points = max(2, n_feat)
    st = M.random_store(100 + n_feat, 3, n_feat, n_points)
    b = Both.of(pkg, G, st, device, max_pts=n_points)
    rng = np.random.default_rng(n_feat)
    for nf in (n_feat, 2 * n_feat + 1):
        want = b.check_reference(voter(rng, st, nf, n_points), rng.normal(0, 1, 3), where="nf=%d" % nf)
    if n_feat >= 63:
        assert len(want["local_kfs"]) == 3 and len(want["local_points"]) > n_feat // 4
    b.check_connections(sorted(st.rows))
    # a shorter row replaces a longer one: the tail of the old row must not count
    b.set_keyframe(4, st.rows[4][:max(1, n_feat // 2)])
    b.check_reference(voter(rng, st, n_feat, n_points), (0, 0, 0))
    b.check_connections(sorted(st.rows))


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n_kf", [1, 2, 64, 65])
def test_slot_counts_with_holes_and_a_replaced_row(env, n_kf, device):
    pkg, G = env
    n_feat, n_points = 48, 40 + 12 * n_kf
    st = M.random_store(200 + n_kf, n_kf, n_feat, n_points, bad_frac=0.05)
    b = Both.of(pkg, G, st, device, max_pts=n_points)
    rng = np.random.default_rng(n_kf)
    ids = sorted(st.rows)
    if n_kf > 2:
        for k in ids[1::3]:
            b.erase(k)
        for k in sorted(b.m.rows)[::5]:
            b.set_bad(k)
    assert b.d.slots() == n_kf and b.d.size() == len(b.m.rows)
    last = sorted(b.m.rows)[-1]
    b.set_keyframe(last, voter(rng, st, n_feat - 5, n_points))            # replaced in place: no new slot
    assert b.d.slots() == n_kf
    for centre in (0.1, 0.5, 0.95):
        lo = max(0, int((n_points - 60) * centre))
        w = b.check_reference(voter(rng, st, 150, min(n_points, lo + 60), lo), rng.normal(0, 1, 3))
    b.check_connections(sorted(b.m.rows))
    if n_kf >= 64:
        assert len(w["local_kfs"]) >= 2
        # the last slot (slot 64 of 65: a second ballot word, a second workgroup of the slot-per-wave grids) can be local and the reference
        w = b.check_reference(np.array(b.m.rows[last] * 2, np.int32), (0, 0, 0))
        assert w["ref_kf"] == last or b.m.kf_bad[last]
    # erased ids cannot come back, lower ids cannot enter: refused, nothing changes
    if n_kf > 2:
        assert b.d.set_keyframe(ids[1], [0, 1]) == -1 and b.d.set_keyframe(0, [0, 1]) == -1
        assert b.d.slots() == n_kf and b.d.size() == len(b.m.rows)


@pytest.mark.parametrize("device", KINDS)
def test_one_point_and_ids_beyond_16_bits(env, device):
    pkg, G = env
    b = Both(pkg, G, 4, 8, 1, device)                                      # max_points = 1: the only id is 0
    b.set_keyframe(2, [0, -1, 0]); b.set_keyframe(5, [-1, 0]); b.set_keyframe(9, [-1])
    b.check_reference([0, 0, 0, 0, 0, -1], (1, 2, 3))
    b.check_connections([2, 5, 9])
    b.set_points_bad([0])
    w = b.check_reference([0, 0, 0, 0, 0, -1], (1, 2, 3))
    assert w["frame_points"] == [-1] * 6
    assert b.d.set_points_bad([1]) == (0 if device else -1)                # outside [0, max_points): refused (host) / ignored (device)
    # ---- 70 000 points: ids that need more than 16 bits
    rng = np.random.default_rng(7)
    b = Both(pkg, G, 6, 120, 70000, device)
    for k in range(6):
        b.set_keyframe(10 + k, rng.integers(69900 - 40 * k, 70000, 120))
    b.set_points_bad([69999, 69950, 65536])
    w = b.check_reference(rng.integers(69800, 70000, 200), (0.5, 0, 0))
    assert len(w["local_kfs"]) == 6 and max(w["local_points"]) > 65536
    b.check_connections([10, 12, 15])


@pytest.mark.parametrize("device", KINDS)
def test_degenerate_voters(env, device):
    pkg, G = env
    st = M.random_store(5, 5, 40, 60)
    st.pt_bad |= {3, 4, 5}
    b = Both.of(pkg, G, st, device, max_kf=9, max_feat=64, max_pts=60)
    w = b.check_reference([-1] * 70, (0, 0, 0))
    assert w["local_kfs"] == [] and w["ref_kf"] == -1 and w["local_points"] == []
    w = b.check_reference([3, 4, 5] * 20, (0, 0, 0))                        # all bad: all nulled, nobody votes
    assert w["frame_points"] == [-1] * 60 and w["local_kfs"] == []
    p = next(q for q in st.rows[1] if q >= 0 and q not in st.pt_bad)
    w = b.check_reference([p] * 70, (0, 0, 0))                              # one point 70 times: 70 votes for every keyframe that holds it
    assert w["weights"] and set(w["weights"]) == {70}
    b.check_reference([], (0, 0, 0))
    b.set_keyframe(40, [-1] * 64); b.set_keyframe(41, [3, 4, 5] * 21); b.set_keyframe(42, [p] * 64); b.set_keyframe(43, [])
    w = b.check_connections([40, 41, 42, 43])
    assert w[0]["ordered"] is None and w[1]["ordered"] is None and w[3]["ordered"] is None and set(w[2]["weights"]) == {64}
    # an empty store: every frame point that is bad is still nulled
    e = Both(pkg, G, 2, 4, 60, device)
    e.set_points_bad([3])
    assert e.check_reference([3, 2, -1], (0, 0, 0))["frame_points"] == [-1, 2, -1]


@pytest.mark.parametrize("case", M.HAND_CASES, ids=[c[0] for c in M.HAND_CASES])
def test_hand_cases(env, case):
    pkg, G = env
    name, rows, bad_pts, bad_kfs, poses, frames, queries = case
    for device in KINDS:
        st = M.Store()
        for k in sorted(rows):
            st.set_keyframe(k, rows[k])
        st.pt_bad = set(bad_pts)
        for k in bad_kfs:
            st.kf_bad[k] = True
        for k, t in poses.items():
            st.t[k] = t
        b = Both.of(pkg, G, st, device)
        for fp in frames:
            b.check_reference(fp, (1.0, 2.0, 3.0), where=name)
        b.check_connections(queries, where=name)


@pytest.fixture(scope="module")
def random_case():
    """40 keyframes x 300 features over 2 000 points, 5 % bad, 10 % repeats; expected values computed once"""
    st = M.random_store(2024, 40, 300, 2000, bad_frac=0.05, repeat_frac=0.10)
    rng = np.random.default_rng(11)
    frames = [voter(rng, st, 300, lo + 600, lo) for lo in (0, 700, 1400)]
    return st, frames


@pytest.mark.parametrize("device", KINDS)
def test_random_case(env, random_case, device):
    pkg, G = env
    st, frames = random_case
    b = Both.of(pkg, G, st, device, max_pts=2000)
    for k in (4, 31, 61):
        b.set_bad(k)
    b.erase(64)
    for fp in frames:
        w = b.check_reference(fp, (0.3, -0.2, 0.1))
        assert 3 <= len(w["local_kfs"]) < 39 and len(w["local_points"]) > 300 and (np.array(w["frame_points"]) != fp).any()
    w = b.check_connections(sorted(b.m.rows))
    assert any(len(x["ordered"]) > 3 for x in w) and any(len(set(x["weights"])) < len(x["weights"]) for x in w if x["ordered"])


@pytest.mark.parametrize("device", KINDS)
def test_cap_below_the_list_length(env, random_case, device):
    pkg, G = env
    st, frames = random_case
    b = Both.of(pkg, G, st, device, max_pts=2000)
    full = len(M.update_reference(st, frames[1], (0, 0, 0))["local_points"])
    assert full > 100
    for cap in (full, full - 1, 7, 0):
        got = b.check_reference(frames[1], (0, 0, 0), cap=cap)             # n_points reports the FULL count, the first cap entries are written
        assert len(got["local_points"]) == full


@pytest.mark.parametrize("device", KINDS)
def test_calls_in_a_row_and_batches(env, random_case, device):
    pkg, G = env
    st, frames = random_case
    b = Both.of(pkg, G, st, device, max_pts=2000)
    ids = sorted(st.rows)
    for _ in range(2):                                                     # the scratch (mult, keys) is clean again after every call
        b.check_reference(frames[0], (0, 0, 0))
        b.check_connections(ids[3:5])
        b.check_reference(frames[2], (0, 0, 0))
    three = [ids[2], ids[20], ids[39]]
    batch = b.d.update_connections(three)
    assert batch == [b.d.update_connections([k])[0] for k in three] == [M.update_connections(st, k) for k in three]
    assert b.d.update_connections([ids[5], ids[5]])[0] == b.d.update_connections([ids[5]])[0]


@pytest.mark.parametrize("device", KINDS)
def test_capacity_errors_leave_the_store_unchanged(env, device):
    pkg, G = env
    st = M.random_store(9, 3, 20, 50)
    b = Both.of(pkg, G, st, device, max_kf=3, max_feat=20, max_pts=50)
    fp = voter(np.random.default_rng(1), st, 60, 50)
    before = (b.d.update_reference(fp, (0, 0, 0), 50), b.d.update_connections(sorted(st.rows)))
    CAP = pkg._capi.MCS_ERR_CAPACITY
    assert b.d.set_keyframe(100, list(range(20))) == CAP                   # a fourth keyframe
    assert b.d.set_keyframe(7, list(range(21))) == CAP                     # a replaced row longer than max_features
    assert b.d.slots() == 3 and b.d.size() == 3 and b.d.slot_ids == sorted(st.rows)
    assert (b.d.update_reference(fp, (0, 0, 0), 50), b.d.update_connections(sorted(st.rows))) == before
    b.check_reference(fp, (0, 0, 0))
    if not device:                                                         # host-kind calls validate what they can see
        assert b.d.set_keyframe(7, [50]) == -1 and b.d.set_keyframe(7, [-2]) == -1
        b.check_reference(fp, (0, 0, 0))
    q, o4, o8 = np.array([999], np.int64), np.zeros(8, np.int32), np.zeros(8, np.int64)                   # a keyframe the store does not hold
    assert b.d.L.mcs_covis_update_connections(b.d.h, 1, q.ctypes.data, 0, o4.ctypes.data, o4.ctypes.data, o8.ctypes.data, o4.ctypes.data, o4.ctypes.data) == -1
    assert b.d.erase(999) == -1 and b.d.set_bad(999) == -1 and b.d.set_pose([999], [(0, 0, 0)]) == -1


def test_refused_while_deferred_searches_are_on(env):
    pkg, G = env
    b = Both.of(pkg, G, M.random_store(1, 2, 8, 20), False)
    L = pkg.lib()
    assert L.mcs_ctx_set_async_search(G.ctx().h, 1) == 0
    try:
        fp, t, o4, o8 = np.zeros(4, np.int32), np.zeros(3), np.zeros(8, np.int32), np.zeros(8, np.int64)
        rc = L.mcs_covis_update_reference(b.d.h, fp.ctypes.data, 4, t.ctypes.data, 4, 0, o8.ctypes.data, o4.ctypes.data, np.zeros(8).ctypes.data, o4.ctypes.data,
                                          o8.ctypes.data, o4.ctypes.data, o4.ctypes.data)
        assert rc == pkg._capi.MCS_ERR_UNSUPPORTED
        q = np.array([1], np.int64)
        assert L.mcs_covis_update_connections(b.d.h, 1, q.ctypes.data, 0, o4.ctypes.data, o4.ctypes.data, o8.ctypes.data, o4.ctypes.data,
                                              o4.ctypes.data) == pkg._capi.MCS_ERR_UNSUPPORTED
    finally:
        assert L.mcs_ctx_set_async_search(G.ctx().h, 0) == 0
    b.check_reference([0, 1, 2], (0, 0, 0))
