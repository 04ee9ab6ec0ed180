"""tests/covis_model.py and tests/cull_model.py on the stores of tests/covis_tiles.py (more than 1024 keyframe slots, lists of more than 128 keyframes), without a
GPU.  Two things: every case does what it is there for (asserted on the model's output, so that a case that misses its purpose fails here), and covis_model
agrees with a second, independent numpy statement that has no loops over keyframes and no steps of 1024: an incidence matrix A[k, p] (point p occurs in row
k), v[p] = the voter's entries equal to p with p not bad, count = A @ v; local keyframes = ascending ids with count > 4 that are not bad; the reference
keyframe = the first argmax among them; ordered = lexsort by (-weight, -id) over count >= 30, else the first argmax; local points = first occurrences over
the concatenated local rows.  This guards the generators and the model's ordering rules where ties run in the thousands."""
import numpy as np
import pytest

import covis_model as M
import cull_model as CM
import covis_tiles as T


class Incidence:
    def __init__(self, st, n_points):
        self.ids = np.array(sorted(st.rows), np.int64)
        self.A = np.zeros((len(self.ids), n_points), np.int16)              # counts stay below 46 * 46
        for i, k in enumerate(self.ids):
            r = np.array(st.rows[k], np.int64)
            self.A[i, r[r >= 0]] = 1
        self.good = np.ones(n_points, bool)
        self.good[sorted(st.pt_bad)] = False
        self.kf_bad = np.array([st.kf_bad[k] for k in self.ids], bool)
        self.st = st

    def votes(self, row):
        r = np.array(row, np.int64)
        return (np.bincount(r[r >= 0], minlength=self.A.shape[1]) * self.good).astype(np.int16)

    def reference(self, frame):
        fp = np.array(frame, np.int64)
        fp[(fp >= 0) & ~self.good[np.maximum(fp, 0)]] = -1
        count = (self.A @ self.votes(frame)).astype(np.int64)
        loc = np.flatnonzero((count > 4) & ~self.kf_bad)
        ref = int(self.ids[loc[np.argmax(count[loc])]]) if len(loc) else -1
        cat = np.concatenate([np.array(self.st.rows[k], np.int64) for k in self.ids[loc]] + [np.zeros(0, np.int64)])
        cat = cat[(cat >= 0) & self.good[np.maximum(cat, 0)]]
        _, first = np.unique(cat, return_index=True)
        return dict(frame_points=fp.tolist(), local_kfs=self.ids[loc].tolist(), weights=count[loc].tolist(), ref_kf=ref, local_points=cat[np.sort(first)].tolist())

    def connections(self, kid):
        count = (self.A @ self.votes(self.st.rows[kid])).astype(np.int64)
        count[self.ids == kid] = 0
        if not count.any():
            return dict(counter={}, ordered=None, weights=None)
        sel = np.flatnonzero(count >= 30)
        if len(sel) == 0:
            sel = np.array([np.argmax(count)])
        sel = sel[np.lexsort((-self.ids[sel], -count[sel]))]
        return dict(counter={int(self.ids[i]): int(count[i]) for i in np.flatnonzero(count)}, ordered=self.ids[sel].tolist(), weights=count[sel].tolist())


def same_reference(got, want):
    for k in ("frame_points", "local_kfs", "weights", "ref_kf", "local_points"):
        assert got[k] == want[k], k


@pytest.mark.parametrize("S", T.SIZES)
def test_hub_stores_reach_every_step_and_the_model_agrees_with_numpy(S):
    c = T.tile_case(S)
    T.assert_tile_case_does_its_job(c)
    st = T.model_of(c)
    inc = Incidence(st, c.max_pts)
    same_reference(c.ref, inc.reference(c.frame))
    for q in c.queries:
        assert c.conn[q] == inc.connections(q), q
    # cap never changes what the model computes: the values the device test asks for are distinct and inside [0, full]
    assert len(set(c.caps)) == len(c.caps) and all(0 <= v <= c.full for v in c.caps)


def test_pinned_slots_the_model_gives_what_the_cases_state():
    c = T.pinned_case()
    st = T.model_of(c)
    inc = Incidence(st, c.max_pts)
    obs = st.observers()
    for name, frame, want in T.PINNED_FRAMES:
        got = M.update_reference(st, frame, (0, 0, 0), obs)
        for k, v in want.items():
            assert got[k] == v, (name, k)
        same_reference(got, inc.reference(frame))
    st.kf_bad[T.kid_of(T.PIN_BAD)] = False
    inc_all = Incidence(st, c.max_pts)
    got = M.update_reference(st, T.ALL_FRAME, (0, 0, 0), obs)
    assert got["local_kfs"] == [T.kid_of(k) for k in range(T.PIN_S)] and got["weights"] == [5] * T.PIN_S and got["ref_kf"] == T.kid_of(0)
    assert got["local_points"] == T.ALL_POINTS
    same_reference(got, inc_all.reference(T.ALL_FRAME))
    st.kf_bad[T.kid_of(T.PIN_BAD)] = True
    for erased in (False, True):
        if erased:
            st.erase(T.kid_of(7))
            inc, obs = Incidence(st, c.max_pts), st.observers()
        want = T.pinned_connections(sorted(st.rows))
        for slot, (ordered, weights) in want.items():
            got = M.update_connections(st, T.kid_of(slot), obs)
            assert got["ordered"] == ordered and got["weights"] == weights, (slot, erased)
            assert got == inc.connections(T.kid_of(slot))
    assert len(want[T.Q30][0]) == T.PIN_S - 2
    st.set_keyframe(T.kid_of(T.QEMPTY), T.EMPTY_ROW)
    got = M.update_connections(st, T.kid_of(T.QEMPTY))
    assert got == dict(counter={}, ordered=None, weights=None) == Incidence(st, c.max_pts).connections(T.kid_of(T.QEMPTY))


@pytest.mark.parametrize("n_list", T.CULL_LIST_LENGTHS)
def test_cull_lists_beyond_one_chunk_do_their_job(n_list):
    c = T.cull_list_case(n_list)
    assert len(c.ids) == n_list == len(set(c.ids)) and sum(c.not_erase) == n_list // 5
    T.assert_cull_list_case_does_its_job(c)


@pytest.mark.parametrize("S", [1100, 2049])
def test_cull_stores_beyond_one_step_do_their_job(S):
    c = T.cull_tile_case(S)
    assert len(c.store.rows) == S and max(len(r) for r in c.store.rows.values()) == 16
    T.assert_cull_tile_case_does_its_job(c)


def test_packed_halves_case():
    rows, octs, listed, n_culled = T.packed_halves_case()
    st = CM.store_of(rows)
    assert CM.observations(st, [0, 1]) == [1100, 1100]
    w = CM.keyframe_culling(st, octs, listed)
    assert w["verdict"].count(1) == n_culled and w["verdict"].count(0) == len(listed) - n_culled and w["bad_points"] == []
    assert w["n_redundant"][:2] == [3, 4] and w["n_mps"][:2] == [4, 4]
    assert CM.observations(CM.erase_culled(w["store"], w["culled"]), [0, 1]) == [1100 - n_culled] * 2
    assert min(T.slot_of(k) for k in listed) < T.STEP < max(T.slot_of(k) for k in listed) and len(listed) > T.CHUNK
