"""-m gpu: the device keyframe database (csrc/mcs_kfdb.hip: k_qbitmap, k_count, k_walk, k_maxc, k_score, k_carry, k_final, k_score_list) and the device
BowVector (k_bow_vector, csrc/mcs_bow.hip) on the hostile cases of tests/hostile_kfdb.py, against the model of tests/kfdb_model.py through tests/kfdb_pack.py.

Every comparison is exact: ids, word counters, counts and orders as equal values, doubles as equal bits; nothing has a tolerance.  In both memory kinds only
the first cand_count[q] candidate ids and the first diag.count[q] diagnostic rows of a query are compared (the first `cap` of them where a call is refused
for its capacity): the rows past them are copied from the call's scratch and are unspecified.  tests/test_kfdb_hostile_cpu.py shows on the model that each
case is what it claims to be and which mutation of the model moves its expected output."""
import pytest

import hostile_kfdb as H
import kfdb_pack as P

pytestmark = pytest.mark.gpu
KINDS = [pytest.param(False, id="host"), pytest.param(True, id="device")]


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return G.mcs, G


def check(env, script, n_words, device, batched=True):
    pkg, G = env
    return P.check(script, n_words, dev=P.DeviceSide(pkg, G, n_words, device), batched=batched)[1]


# ------------------------------------------------------------------ 1. row and bitmap geometry (k_qbitmap, k_count)

@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n_words", H.GEOMETRY_WORDS)
def test_row_and_bitmap_geometry(env, n_words, device):
    """bit 0 / 31 of a bitmap word and the last word of the vocabulary; rows of 0, 1, 63, 64, 65, 128, 129 words; the only shared word at index 64; the
    smallest shared word at lane 63 against a larger one at lane 0; 16 + 1 queries; bitmaps of exactly 48 KB in LDS (24 576 words) and the first size read
    from global memory (24 577)"""
    script, _ = H.geometry(n_words)
    check(env, script, n_words, device)
    check(env, script, n_words, device, batched=False)


@pytest.mark.parametrize("device", KINDS)
def test_all_rows_empty(env, device):
    check(env, H.geometry_all_empty(33), 33, device)


# ------------------------------------------------------------------ 2. slot and query counts

@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("S", H.SLOT_COUNTS)
def test_slot_counts(env, S, device):
    """1, 3, 4, 5 slots around k_count's four per workgroup, 255, 256, 257 around the 256-thread blocks of k_walk / k_maxc / k_score / k_carry; ghosts, erased"""
    check(env, H.slots(S, 3), H.SLOT_WORDS, device)


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("nq,S", H.BATCHES)
def test_batch_sizes(env, nq, S, device):
    """1, 15, 16, 17, 32, 33 queries around KF_QG = 16, with fresh ids, an id repeated inside the batch and id 0; the batch against the model's sequential
    calls, and the same queries one call each"""
    check(env, H.slots(S, nq), H.SLOT_WORDS, device)
    check(env, H.slots(S, nq), H.SLOT_WORDS, device, batched=False)


# ------------------------------------------------------------------ 3. state across reallocation

@pytest.mark.parametrize("device", KINDS)
def test_state_survives_reallocation(env, device):
    """query ids, counters and scores of both forms across the growth of the state arrays from 256 to 600 and from 600 to 1240 slots (traps (a) and (b))"""
    check(env, H.realloc(), 64, device)


# ------------------------------------------------------------------ 4. long lists through k_final

@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n", H.LONG_COUNTS)
def test_long_lists(env, n, device):
    """every keyframe in the list: 1 023, 1 024, 1 025, 2 049 entries through k_final's 1024-thread strides; add order with the re-added ones last; covisibility
    lists of none, itself, one neighbour twice and ten; cand cap and diagnostics cap below the counts (MCS_ERR_CAPACITY, full counts, state unchanged)"""
    check(env, H.long_list(n, "mixed") + H.long_queries(n), 8, device)


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("n", (1025, 2049))
def test_long_list_with_one_common_best(env, n, device):
    res = check(env, H.long_list(n, "common") + [("reloc", [(7000, *H.LONG_QUERY)]), ("loop", H.q_loop(7001, 0.0))], 8, device)
    assert res[0][0][0] == [1] and res[1][0][0] == [1]


@pytest.mark.parametrize("device", KINDS)
def test_count_only_call_commits(env, device):
    """cap = 0 with null cand_ids succeeds when no query has a candidate, and its state is committed"""
    check(env, H.count_only(), 16, device)


# ------------------------------------------------------------------ 5. thresholds and ties

@pytest.mark.parametrize("device", KINDS)
def test_retention_boundary(env, device):
    res = check(env, H.retention(), 4, device)
    assert res[0][0][0] == [1, 3] and res[1][0][0] == [1, 3]


@pytest.mark.parametrize("device", KINDS)
def test_best_neighbour_ties(env, device):
    check(env, H.best_neighbour(), 8, device)


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("m", sorted(H.MIN_COMMON))
def test_min_common_words(env, m, device):
    check(env, H.min_common(m), 32, device)


@pytest.mark.parametrize("device", KINDS)
def test_loop_min_scores(env, device):
    """a score equal to min_score passes, a min_score one ulp above the score drops it; -inf, +inf; NaN gives what the model gives: no candidate"""
    res = check(env, H.loop_min_scores(), 8, device)
    assert res[4] == [([], [])]


@pytest.mark.parametrize("device", KINDS)
def test_connected_sets(env, device):
    check(env, H.connected_sets(), 8, device)


# ------------------------------------------------------------------ 6. ids

@pytest.mark.parametrize("device", KINDS)
def test_wide_ids(env, device):
    """keyframe ids 1 and 2^32 + 1 are two slots and come back with all 64 bits; query ids 1, 2^32 + 1, -1, INT64_MIN, INT64_MAX"""
    check(env, H.wide_ids(), 8, device)


@pytest.mark.parametrize("device", KINDS)
def test_erased_best_keyframe(env, device):
    res = check(env, H.erased_best(), 8, device)
    assert res[1][0][0] == [2]


# ------------------------------------------------------------------ 7. mcs_kfdb_add and mcs_kfdb_score

@pytest.mark.parametrize("device", KINDS)
def test_add_calls_and_refusals(env, device):
    """a batched add with empty rows in the middle; every refusal by code and text (the bad offsets among them, refused before anything is sized by them);
    size() and a following query equal the model after each"""
    check(env, H.add_calls(), 40, device)


@pytest.mark.parametrize("device", KINDS)
def test_slab_grows_behind_rows(env, device):
    """40 adds of one 5-word row each: the slab is reallocated at 64 and at 128 elements with rows in it; every row's score and a query over the first and
    the last row"""
    check(env, H.slab_growth(), H.SLAB_WORDS, device)


@pytest.mark.parametrize("device", KINDS)
def test_bad_queries_leave_the_state(env, device):
    check(env, H.bad_queries(), 40, device)


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("nkf", H.SCORE_COUNTS)
def test_score(env, nkf, device):
    check(env, H.score_calls(nkf), 64, device)


# ------------------------------------------------------------------ 8. mcs_bow_vector on a root with 4 200 leaves

DUPLICATE = "two nodes with a weight > 0 carry the same word id (every word has one leaf)"


@pytest.fixture(scope="module")
def voc(env):
    pkg, G = env
    node_desc, child_off, child_idx, word, weight = H.vocabulary()
    v = P.Vocab(pkg, G, node_desc, child_off, child_idx)
    assert v.set_words(word, weight) == (0, "")
    return v, word, weight


@pytest.mark.parametrize("device", KINDS)
@pytest.mark.parametrize("pattern", H.BOW_PATTERNS)
@pytest.mark.parametrize("n", H.BOW_COUNTS)
def test_bow_vector(voc, n, pattern, device):
    """0, 1, 1 023, 1 024, 1 025, 4 097 leaves through k_bow_vector's 1024-thread strides: one word n times (n sequential additions), that word next to a
    second one, distinct words, stop words only (no word, norm 0), stop words mixed in; weights from 2^-40 to 2^20"""
    v, word, weight = voc
    leaf = H.leaves(n, pattern)
    rc, got = v.bow_vector(leaf, device)
    assert rc == 0
    assert got == P.model_bow_vector(word, weight, leaf)


@pytest.mark.parametrize("device", KINDS)
def test_bow_vector_after_a_refused_call(voc, device):
    """a leaf id out of range is refused, and the histogram is zero again: the same good call gives the same bits as before"""
    v, word, weight = voc
    good = H.leaves(1025, "stop_mixed")
    want = P.model_bow_vector(word, weight, good)
    assert v.bow_vector(good, device) == (0, want)
    for bad_id in (H.VOC_LEAVES + 1, -1):
        bad = good.copy()
        bad[700] = bad_id
        assert v.bow_vector(bad, device)[0] == P.INVALID
        assert v.L_.mcs_last_error().decode() == "mcs_bow_vector: leaf node id out of range"
        assert v.bow_vector(good, device) == (0, want)


def test_duplicate_word_ids_are_refused(voc):
    """two nodes of weight > 0 with one word id are refused (the word's weight would be whichever node reached the histogram first), the previous table stays
    usable; nodes of weight 0 may share an id"""
    v, word, weight = voc
    leaf = H.leaves(1024, "distinct")
    want = P.model_bow_vector(word, weight, leaf)
    dup = word.copy()
    dup[10] = dup[20]
    assert weight[10] > 0 and weight[20] > 0
    assert v.set_words(dup, weight) == (P.INVALID, DUPLICATE)
    assert v.bow_vector(leaf, False) == (0, want)
    shared = word.copy()
    shared[7], shared[14] = shared[21], shared[10]   # nodes 7, 14, 21 are stop words (weight 0): 7 shares 21's id, 14 shares the id of weighted node 10
    assert weight[7] == weight[14] == weight[21] == 0
    assert v.set_words(shared, weight) == (0, "")
    assert v.bow_vector(leaf, True) == (0, P.model_bow_vector(shared, weight, leaf))
    assert v.set_words(word, weight) == (0, "")
