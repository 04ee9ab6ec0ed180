"""-m gpu: mcs_covis_* on stores of more than 1024 keyframe slots and lists of more than 128 keyframes (tests/covis_tiles.py), against tests/covis_model.py and
tests/cull_model.py, host kind and device kind, bit for bit: everything compared is an integer except local_dist, which is + - * and sqrt only and is compared
by bytes.  What runs here and nowhere else in the suite: the second and later 1024-slot steps of k_covis_local (base, wtot[16] and the atomicMax of the
reference keyframe carried across steps, the tail from n on) and of k_covis_scan, the strided loops of k_covis_order with ties in every step, the second and
later 128-entry chunks of the culling list, and the wave-per-slot grids beyond 256 workgroups.

Every case is first held to what it is there for on the MODEL's output (covis_tiles.assert_*; tests/test_covis_tiles_cpu.py runs the same without a GPU).
Each (S, kind) hub store is built once per module, by S mcs_covis_set_keyframe calls, and shared by the checks that follow; none of them changes it."""
import importlib
import itertools

import numpy as np
import pytest

import cull_model as CM
import covis_tiles as T
from cull_pack import CullBoth

pytestmark = pytest.mark.gpu
KINDS = [False, True]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return importlib.import_module("multicol-slam_amd"), G


def same_reference(got, want, cap, where):
    """what covis_pack.Both.check_reference asserts, against a result of the model that was computed before"""
    full = len(want["local_points"])
    assert got["frame_points"] == want["frame_points"], where
    assert got["local_kfs"] == want["local_kfs"] and got["weights"] == want["weights"] and got["ref_kf"] == want["ref_kf"], where
    assert np.array(got["dists"]).tobytes() == np.array(want["dists"]).tobytes(), where
    assert got["n_points"] == full and got["local_points"] == want["local_points"][:cap], (where, got["n_points"], full)


# ---------------------------------------------------------------------------------------------- 1. hub stores of S slots
@pytest.fixture(scope="module", params=list(itertools.product(T.SIZES, KINDS)), ids=lambda p: "%d-%s" % (p[0], "device" if p[1] else "host"))
def hub(request, env):
    S, device = request.param
    c = T.tile_case(S)
    T.assert_tile_case_does_its_job(c)                             # on the model, before the device is asked
    b = T.both_of(c, *env, device)
    assert b.d.slots() == S and b.d.size() == S - len(c.erased)
    return c, b


def test_local_map_across_steps(hub):
    c, b = hub
    want = b.check_reference(c.frame, c.frame_t, where="S=%d" % c.S)   # the Both's own model, kept in step call by call
    assert want == c.ref
    got = b.d.update_reference(c.frame, c.frame_t, c.full + 3)
    assert got["ref_kf"] == T.kid_of(100) and len(got["local_kfs"]) == len(c.ref["local_kfs"])
    if T.steps(c.S) > 1:
        assert c.stray_point in got["local_points"]
    # a second frame whose votes reach no keyframe, then the first again: rankOf, cnt and off of the longer call do not linger
    none = b.check_reference([-1, T.HUB - 1, -1], c.frame_t)
    assert none["local_kfs"] == [] and none["ref_kf"] == -1
    same_reference(b.d.update_reference(c.frame, c.frame_t, c.full), c.ref, c.full, "again")


def test_cap_around_the_offset_of_step_one(hub):
    c, b = hub
    for cap in c.caps:
        got = b.d.update_reference(c.frame, c.frame_t, cap)        # n_points stays the full count; exactly the first cap entries are written
        same_reference(got, c.ref, cap, "S=%d cap=%d" % (c.S, cap))
        assert got["n_points"] == c.full and len(got["local_points"]) == cap


def test_connections_of_a_query_in_every_step(hub):
    c, b = hub
    for q in c.queries:
        got = b.d.update_connections([q])[0]
        assert got == c.conn[q], ("S=%d query slot %d" % (c.S, T.slot_of(q)))
    assert b.check_connections([c.queries[-1]])[0] == c.conn[c.queries[-1]]


def test_a_batch_from_different_steps_equals_the_single_calls(hub):
    c, b = hub
    batch = b.d.update_connections(c.batch)
    assert batch == [b.d.update_connections([q])[0] for q in c.batch]
    assert batch == [c.conn[q] for q in c.batch]


# ---------------------------------------------------------------------------------------------- 2. pinned slots, S = 2049
@pytest.mark.parametrize("device", KINDS)
def test_pinned_slots(env, device):
    """one store, the calls in a row; the erasure of slot 7 comes last.  Every expectation is stated in covis_tiles (PINNED_FRAMES, ALL_POINTS,
    pinned_connections) and the model is compared as well."""
    c = T.pinned_case()
    b = T.both_of(c, *env, device)
    S = T.PIN_S
    for name, frame, want in T.PINNED_FRAMES:
        w = b.check_reference(frame, (0.5, 0.25, -1.0), where=name)
        got = b.d.update_reference(frame, (0.5, 0.25, -1.0), 8)
        for k, v in want.items():
            assert w[k] == v and got[k] == v, (name, k, got[k], v)
    # only the last slot is local: Dev.update_reference has asserted -1 / 0 / 0 from index n_local on; here that n_local is 1
    got = b.d.update_reference(T.PINNED_FRAMES[4][1], (0, 0, 0), 8)
    assert got["local_kfs"] == [T.kid_of(S - 1)] and got["n_points"] == 3
    # every slot local
    b.set_bad(T.kid_of(T.PIN_BAD), False)
    w = b.check_reference(T.ALL_FRAME, (0, 0, 0), where="all")
    got = b.d.update_reference(T.ALL_FRAME, (0, 0, 0), len(T.ALL_POINTS))
    assert got["local_kfs"] == [T.kid_of(k) for k in range(S)] and got["weights"] == [5] * S and got["ref_kf"] == T.kid_of(0)
    assert got["local_points"] == T.ALL_POINTS == w["local_points"]
    b.set_bad(T.kid_of(T.PIN_BAD), True)
    # update_connections
    for erased in (False, True):
        if erased:
            b.erase(T.kid_of(7))
        want = T.pinned_connections(sorted(b.m.rows))
        slots = sorted(want)
        got = b.check_connections([T.kid_of(k) for k in slots], where="erased=%s" % erased)
        for k, g in zip(slots, got):
            assert (g["ordered"], g["weights"]) == want[k], (k, erased)
        if not erased:
            # a query whose counter is empty, in place of a row that voted before; the old row comes back afterwards
            old = list(b.m.rows[T.kid_of(T.QEMPTY)])
            b.set_keyframe(T.kid_of(T.QEMPTY), T.EMPTY_ROW)
            g = b.check_connections([T.kid_of(T.QEMPTY), T.kid_of(T.Q29)])
            assert g[0] == dict(counter={}, ordered=None, weights=None) and g[1]["ordered"] == [T.kid_of(0)]
            b.set_keyframe(T.kid_of(T.QEMPTY), old)
    assert b.d.slots() == S and b.d.size() == S - 1


# ---------------------------------------------------------------------------------------------- 3. culling at size
def max_point(st):
    return max([p for r in st.rows.values() for p in r] + list(st.pt_bad) + [0])


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n_list", T.CULL_LIST_LENGTHS)
def test_cull_lists_around_the_chunk(env, n_list, device):
    c = T.cull_list_case(n_list)
    T.assert_cull_list_case_does_its_job(c)
    b = CullBoth.of(*env, c.store, c.octaves, device, max_pts=max_point(c.store) + 1)
    w = b.check_cull(c.ids, c.not_erase, where="n=%d" % n_list)
    assert w["verdict"] == c.want["verdict"] and w["bad_points"] == c.want["bad_points"]
    # a second call on what is left, the list reversed: the list buffer of the first call does not linger
    rest = [k for k in c.ids[::-1] if k in b.m.rows]
    b.check_cull(rest, where="second")


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("S", [1100, 2049])
def test_cull_every_keyframe_of_a_store_beyond_one_step(env, S, device):
    c = T.cull_tile_case(S)
    T.assert_cull_tile_case_does_its_job(c)
    b = CullBoth.of(*env, c.store, c.octaves, device, max_pts=max_point(c.store) + 1)
    for k in c.erased:
        b.erase(k)
    for k in c.bad_kfs:
        b.set_bad(k)
    b.set_points_bad(c.bad_points)
    assert b.d.slots() == S and b.d.size() == len(c.ids)
    w = b.check_cull(c.ids, c.not_erase, where="S=%d" % S)           # with its read-back: observations before and after the erasures, update_reference
    assert w["verdict"] == c.want["verdict"] and w["bad_points"] == c.want["bad_points"]
    assert b.d.size() == len(c.ids) - len(w["culled"])


@pytest.mark.parametrize("max_kf", [1100, 65536])
def test_both_halves_of_a_packed_counter_word(env, max_kf):
    """1100 observers at level 0 and 1100 at level 1: the two 16-bit halves of one word (max_kf = 1100), or two 32-bit counters (max_kf = 65536)"""
    rows, octs, listed, n_culled = T.packed_halves_case()
    st = CM.store_of(rows)
    for device in KINDS:
        b = CullBoth.of(*env, st, octs, device, max_kf=max_kf, max_feat=4, max_pts=2200)
        assert b.d.observations([0, 1, 2, 3, 1000, 2199]) == [1100, 1100, 1100, 550, 1, 0]
        w = b.check_cull(listed, erase=False)
        assert w["verdict"].count(1) == n_culled
        assert b.d.observations([0, 1, 3]) == [1100, 1100, 550]     # a culled keyframe's row still counts until the caller erases it
        for k in w["culled"]:
            b.erase(k)
        assert b.d.observations([0, 1, 3]) == [1100 - n_culled, 1100 - n_culled, 550 - n_culled]
        b.check_observations()
