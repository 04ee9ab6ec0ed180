"""The hostile keyframe databases of tests/hostile_kfdb.py are what they claim to be: asserted on the model (tests/kfdb_model.py) alone, without a GPU.
Where a case exists to pin one line of a kernel, the model is also mutated the way that line could be wrong, and the expected output must change: a case
that no mutation moves would pass on a wrong kernel too.  tests/test_gpu_hostile_kfdb.py runs the same scripts on the device."""
import math
import struct

import numpy as np
import pytest

import hostile_kfdb as H
import kfdb_model as M
import kfdb_pack as P

INT_MAX = 0x7FFFFFFF


def run(script, n_words=64, mut=None):
    """-> per query operation, per query: (candidate ids, trace with doubles as bits)"""
    out = []
    for r in P.check(script, n_words, mut=mut)[1]:
        if r and isinstance(r[0], tuple):
            r = [(c, P.trace_key(t)) for c, t in r]
        out.append(r)   # (a score operation's result stays a list of doubles, or None where the call is refused)
    return out


def ids(trace):
    return [row[0] for row in trace]


def f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# ------------------------------------------------------------------ 1. geometry

def list_order(kfs_in_add_order, query_words, minw):
    """the list order the device builds: (smallest shared word by `minw`, add sequence) over the keyframes that share a word.  The model has no smallest
    shared word to mutate (its order falls out of the walk over the inverted lists), so the two minw mutations act on this restatement, one step removed
    from kfdb_model, unlike every other mutation of this file: it is first held equal to the model's trace order under `minw_true`, then mutated."""
    q = set(query_words)
    keyed = [(minw(row, q), seq, i) for seq, (i, row, _) in enumerate(kfs_in_add_order) if q & set(row)]
    return [i for _, _, i in sorted(keyed)]


def minw_true(row, q):
    return min(w for w in row if w in q)


def minw_first_pass_only(row, q):   # mutation: the lanes' second pass (index >= 64) never reaches the minimum
    return min([w for k, w in enumerate(row) if w in q and k < 64], default=INT_MAX)


def minw_lane0_wins(row, q):        # mutation: no reduction across lanes: lane 0's own minimum is written
    return min([w for k, w in enumerate(row) if w in q and k % 64 == 0], default=INT_MAX)


@pytest.mark.parametrize("n_words", [n for n in H.GEOMETRY_WORDS if n >= 6999])
def test_geometry_placements_decide_the_order(n_words):
    script, order = H.geometry(n_words)
    kfs = [op for op in script if op[0] == "add"][0][1]
    batch = [op for op in script if op[0] == "reloc"][0][1]
    res = run(script, n_words)[0]
    by = {n: k for k, n in reversed(list(enumerate(order)))}   # first occurrence of each query
    for name in "ABCEF":
        cands, trace = res[by[name]]
        assert ids(trace) == list_order(kfs, batch[by[name]][1], minw_true), name   # every keyframe sharing a word is scored in these queries
    assert ids(res[by["A"]][1]) == [1, 2] and ids(res[by["C"]][1]) == [2, 1] and ids(res[by["B"]][1]) == [3, 4]   # both orders occur
    assert list_order(kfs, batch[by["A"]][1], minw_first_pass_only) == [2, 1]
    assert list_order(kfs, batch[by["B"]][1], minw_lane0_wins) == [4, 3]
    assert list_order(kfs, batch[by["B"]][1], minw_first_pass_only) == [3, 4]   # index 63 is still in the first pass: only the lane mutation moves B
    rows = {i: r for i, r, _ in kfs}
    assert rows[1].index(164) == 64 and len(rows[1]) == 129 and rows[3].index(1126) == 63 and rows[3].index(1128) == 64 and len(rows[3]) == 128
    assert [len(rows[i]) for i in (6, 7, 8, 9, 10)] == [0, 1, 63, 64, 65]
    assert ids(res[by["E"]][1]) == [8, 9, 10] and ids(res[by["D"]][1]) == [5] and ids(res[by["F"]][1]) == [8, 9, 10]
    assert res[by["G"]] == ([], []) and res[by["H"]] == ([], [])
    assert len(batch[by["F"]][1]) > 256 and len(batch) == 17
    assert 16 * ((24576 + 31) // 32) * 4 == 48 * 1024 and 16 * ((24577 + 31) // 32) * 4 > 48 * 1024


@pytest.mark.parametrize("n_words", [n for n in H.GEOMETRY_WORDS if n < 6999])
def test_geometry_small_vocabularies(n_words):
    script, order = H.geometry(n_words)
    res = run(script, n_words)[0]
    kfs = [op for op in script if op[0] == "add"][0][1]
    assert set(ids(res[order.index("C")][1])) <= {i for i, r, _ in kfs if r} and len(res[order.index("C")][1]) >= 1
    assert res[order.index("G")] == ([], [])
    assert all(c == [] and t == [] for r in run(H.geometry_all_empty(n_words), n_words) for c, t in r)


# ------------------------------------------------------------------ 2. slots and batches

@pytest.mark.parametrize("nq,S", [b for b in H.BATCHES if b[0] >= 2] + [(3, S) for S in H.SLOT_COUNTS if S >= 2])
def test_batches_read_scores_written_earlier_in_the_batch(nq, S):
    script = H.slots(S, nq)
    good, mutant = run(script), run(script, mut={"no_carry": True})
    assert good[0][-1] != mutant[0][-1], "relocalisation: the last query reads no score of the batch"
    assert good[0][-1][1][0][0] == 1 and good[0][0][1][0][0] == 2   # the first query lists kf 2, the last lists kf 1 first (word 0 is the smallest)
    qid = [q[0] for q in script[-2][1]]
    if nq >= 15:
        assert 0 in qid and len(set(qid)) < len(qid)


def test_slot_counts_have_ghosts_and_erased():
    for S in H.SLOT_COUNTS:
        script = H.slots(S, 3)
        mod, _ = P.check(script, 64)
        assert len(mod.kf) == S, S
        if S >= 4:
            assert 0 < len(mod.active) < S - max(1, S // 8) + 1 and any(op[0] == "erase" for op in script)


# ------------------------------------------------------------------ 3. reallocation

def test_reallocation_rounds_carry_state():
    script = H.realloc()
    good = run(script)
    assert len(good) == 8   # four rounds, relocalisation then loop
    # (round, hook, state lost from this id on, the queries 0..2 of the round's batch that must change per form).  Query 0 = the repeated id (trap (b) and the
    # stale score behind it), 1 = trap (a) in slots 0 / 1, 2 = trap (a) in slots past 256 (kf 291 has a score only from round 2 on); the loop form cannot
    # read a stale score through (a), only through query 0
    for r, hook, from_id, moved in ((2, "grow2", 0, ({0, 1}, {0})), (3, "grow3", 0, ({0, 1, 2}, {0})), (3, "grow3", 257, ({0, 2}, {0}))):
        mutant = run(script, mut={"hook": {hook: H.zero_state(from_id)}})
        assert mutant[:2 * r] == good[:2 * r]
        for form in (0, 1):
            g, m = good[2 * r + form], mutant[2 * r + form]
            assert {k for k in (0, 1, 2) if g[k] != m[k]} == moved[form], (r, hook, from_id, form)
            # trap (b): kf 3 is never appended again, kf 292 once (it is new in round 2); the mutants append them
            assert ids(g[0][1]) == ([293, 4, 292] if r == 2 else [293, 4]) and (3 in ids(m[0][1])) == (from_id == 0) and 292 in ids(m[0][1])
            acc = {row[0]: f64(row[3]) for row in g[0][1]}
            score = {row[0]: f64(row[2]) for row in g[0][1]}
            assert acc[4] > score[4] and (acc[293] > score[293]) == (r == 3)   # the stale scores of kf 2 / kf 291 (scored from round 2 on) are in
    # the two forms keep separate state: dropping the loop queries leaves the relocalisation results as they are
    assert run([op for op in script if op[0] != "loop"]) == good[0::2]
    slots = np.cumsum([len(op[1]) for op in script if op[0] == "add"]).tolist()
    assert slots == list(H.REALLOC_BLOCKS) and slots[1] <= 256 < slots[2] <= 600 < slots[3] and slots[3] > 514


# ------------------------------------------------------------------ 4. long lists

@pytest.mark.parametrize("n", H.LONG_COUNTS)
def test_long_lists(n):
    order = [i for i in range(1, n + 1) if i not in H.LONG_READDED(n)] + H.LONG_READDED(n)
    res = run(H.long_list(n, "mixed") + H.long_queries(n), 8)
    cands, trace = res[0][0]
    assert ids(trace) == order and cands == [i for i in order if i % 4 == 3]
    assert {f64(row[2]) for row in trace} == {0.75} and {f64(row[3]) for row in trace} == {0.75, 1.5, 2.25, 8.25}
    assert all(row[4] == row[0] for row in trace)   # equal scores: every entry stays its own best
    assert len(res[1][0][0]) > 3 and len(res[2][0][1]) > 100   # the caps of the two refused calls are below the counts
    assert res[3][0] == ([], [])   # the first id again: nothing appended, because the refused calls committed nothing
    assert res[6][0][0] == cands and res[6][1] == ([], [])   # loop form: min score equal to the common score, and one ulp above
    cands, trace = run(H.long_list(n, "common") + [("reloc", [(7000, *H.LONG_QUERY)])], 8)[0][0]
    assert cands == [1] and ids(trace) == order and {row[4] for row in trace} == {1}


def test_count_only_call_commits():
    script = H.count_only()
    good = run(script, 16)
    assert good[0] == [([], [])]
    mutant = run(script, 16, mut={"hook": {"after_count_only": H.zero_state()}})
    assert good[1] != mutant[1] and f64(good[1][0][1][0][3]) == 2.0 and f64(mutant[1][0][1][0][3]) == 1.0


# ------------------------------------------------------------------ 5. thresholds and ties

def test_retention_boundary(monkeypatch):
    good = run(H.retention(), 4)
    for form in (0, 1):
        cands, trace = good[form][0]
        assert [f64(row[2]) for row in trace] == [1.0, 0.75, np.nextafter(0.75, 1.0)] and cands == [1, 3]

    def retain_ge(accs, best):
        seen, out = set(), []
        for acc, k in accs:
            if acc >= 0.75 * best and id(k) not in seen:
                seen.add(id(k))
                out.append(k)
        return out

    monkeypatch.setattr(M, "_retain", retain_ge)
    assert run(H.retention(), 4)[0][0][0] == [1, 2, 3]


def test_best_neighbour_ties():
    for form in run(H.best_neighbour(), 8):
        cands, trace = form[0]
        best = {row[0]: row[4] for row in trace}
        assert best[1] == 3 and best[4] == 4 and best[6] == 6


@pytest.mark.parametrize("m", sorted(H.MIN_COMMON))
def test_min_common_words(m):
    assert H.MIN_COMMON[m] == int(m * 0.8)
    for form in run(H.min_common(m), 32):
        assert ids(form[0][1]) == [1, 3] and [row[1] for row in form[0][1]] == [m, H.MIN_COMMON[m] + 1]


def test_loop_min_scores():
    res = run(H.loop_min_scores(), 8)
    single = [r[0] for r in res[:7]]
    listed = [sorted(ids(t)) for _, t in single]
    assert listed == [[1, 2, 3], [2], [1, 2, 3], [], [], [2], []]
    assert np.nextafter(H.LOOP_SCORE, 1.0) == H.LOOP_SCORE + H.ULP_075 and math.isnan(H.loop_min_scores()[7][1][0][3])


def test_connected_sets():
    res = run(H.connected_sets(), 8)
    assert 2 not in ids(res[1][0][1]) and not {4, 5} & set(ids(res[2][0][1]))
    row3 = [row for row in res[3][0][1] if row[0] == 3][0]
    assert f64(row3[3]) == 2.25 and not {4, 5} & set(ids(res[3][0][1]))   # kf 4 / kf 5 are not appended, but counted by kf 3 with counters of 3


# ------------------------------------------------------------------ 6. ids

def test_wide_ids():
    res = run(H.wide_ids(), 8)
    assert {1, H.BIG} <= set(ids(res[0][0][1])) and (H.BIG & 0xFFFFFFFF) == 1
    assert {H.INT64_MIN, H.INT64_MAX, -1} <= {i for q in res[0] for i in ids(q[1])}
    res = run(H.erased_best(), 8)
    assert res[1][0][0] == [2] and ids(res[1][0][1]) == [1] and res[2][0][0] == [1]


# ------------------------------------------------------------------ 7. add / score (the model side of the scripts runs)

def test_add_and_score_scripts_run_on_the_model():
    assert len(run(H.add_calls(), 40)) == 2 and run(H.bad_queries(), 40)
    for n in H.SCORE_COUNTS:
        res = run(H.score_calls(n))
        assert len(res[0]) == n and (n < 2 or res[0][1] == 0.0) and all(x == 0.0 for x in res[1])


def test_slab_growth_has_rows_behind_each_reallocation():
    script = H.slab_growth()
    adds = [op for op in script if op[0] == "add"]
    assert len(adds) == H.SLAB_ADDS and all(len(op[1]) == 1 and len(op[1][0][1]) == H.SLAB_ROW for op in adds)
    used = np.cumsum([len(op[1][0][1]) for op in adds]).tolist()   # slab elements in use after each add; capacities 64 -> 128 -> 256 (max(need, 2 * cap, 64))
    for cap in (64, 128):
        k = [i for i in range(1, len(used)) if used[i - 1] <= cap < used[i]]
        assert len(k) == 1 and used[k[0] - 1] > 0, cap   # one add crosses the capacity, with rows in the slab before it
    assert 128 < used[-1] <= 256
    assert all(max(op[1][0][1]) < H.SLAB_WORDS for op in adds)
    scores, reloc = run(script, H.SLAB_WORDS)
    assert len(scores) == H.SLAB_ADDS and all(0.0 < s < 1.0 for s in scores) and len(set(scores)) > 1   # rows differ: a shifted row shows
    assert sorted(ids(reloc[0][1])) == [1, H.SLAB_ADDS]   # the query meets the first row and the last, nothing between


# ------------------------------------------------------------------ 8. BowVectors

def test_bow_vector_preconditions():
    _, child_off, child_idx, word, weight = H.vocabulary()
    N = H.VOC_LEAVES
    assert len(set(word[1:].tolist())) == N and child_off[1] == N and (child_off[1:] == N).all() and child_idx.tolist() == list(range(1, N + 1))
    w = float(weight[1234])
    assert w > 0 and weight[4001] > 0
    for n in (4096, 4097):
        s = 0.0
        for _ in range(n):
            s += w
        assert s != n * w   # n sequential additions are not one product
    assert weight[weight > 0].max() / weight[weight > 0].min() > 2.0 ** 59
    leaf = H.leaves(4097, "distinct")
    items = M.bow_vector(word[leaf].tolist(), weight[leaf].tolist())
    raw = {int(word[x]): float(weight[x]) for x in leaf if weight[x] > 0}
    up = down = 0.0
    for k in sorted(raw):
        up += abs(raw[k])
    for k in sorted(raw, reverse=True):
        down += abs(raw[k])
    assert up != down and len(items) == len(raw) < 4097   # the order of the norm's sum shows, and stop words are dropped
    assert P.model_bow_vector(word, weight, H.leaves(1025, "zeros")) == [] and (weight[H.leaves(1025, "zeros")] == 0).all()
    assert P.model_bow_vector(word, weight, H.leaves(4097, "same")) == [(int(word[1234]), P.bits(1.0))]
    two = P.model_bow_vector(word, weight, H.leaves(4097, "same_plus_one"))
    s = 0.0
    for _ in range(4096):
        s += w
    assert len(two) == 2 and dict(two)[int(word[1234])] != P.bits(4096 * w / (4096 * w + float(weight[4001]))) and \
        dict(two)[int(word[1234])] == P.bits(s / (s + float(weight[4001])) if word[1234] < word[4001] else s / (float(weight[4001]) + s))
    mixed = H.leaves(1024, "stop_mixed")
    assert (weight[mixed] == 0).any() and (weight[mixed] > 0).any() and len(set(mixed.tolist())) < 100
