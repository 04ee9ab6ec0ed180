"""Hostile keyframe databases, covisibility lists and query batches for the device keyframe database (csrc/mcs_kfdb.hip), as scripts of operations that
tests/kfdb_pack.py runs on the model and on the library, and hostile leaf lists for mcs_bow_vector.  Pure Python / NumPy; nothing of the library is
imported.  Every builder names the launch shape it is aimed at:

    k_qbitmap   workgroup per query, 256 lanes striding the query's words, bit w & 31 of word w >> 5
    k_count     4 slots per workgroup (one wave each), lanes stride a row by 64, 16 queries per workgroup, bitmaps in LDS up to 48 KB (16 queries x
                24 576 words), else read from global memory
    k_walk / k_score / k_carry   256-thread blocks over the slots
    k_final / k_bow_vector       1024-thread strides over the list / the leaves
    state arrays                 capacity max(2 * slots, 256) at the first query that finds it too small, the old contents copied
    slab of rows                 capacity max(need, 2 * capacity, 64) elements at the first add that finds it too small, the rows in use copied

Values are plain doubles; nothing needs them normalised (the library and the model do the same arithmetic on whatever they are given)."""
import math

import numpy as np

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
ULP_075 = 2.0 ** -53   # 0.75 + 2^-53 is the next double above 0.75


def uni(words):
    """a row with the same value 1 / len for every word"""
    words = [int(w) for w in words]
    return words, [1.0 / len(words)] * len(words)


# ------------------------------------------------------------------ 1. row and bitmap geometry (k_qbitmap, k_count)

GEOMETRY_WORDS = (1, 32, 33, 6999, 24576, 24577)
# keyframe ids of the two placements (big vocabularies)
KF_IDX64, KF_AFTER_IDX64, KF_LANE63, KF_AFTER_LANE63 = 1, 2, 3, 4


def geometry(n_words):
    """-> (script, notes).  One batch of 17 queries (16 fill one k_count workgroup and, at 24 576 words, exactly 48 KB of LDS; the 17th starts a second one).

    Big vocabularies (>= 6 999 words):
      kf 1  129 words 100..228; the only word it shares with query A (164) sits at index 64: lane 0's second pass.
      kf 2  [50, 400], added BEFORE kf 1.  Query A = {164, 400}: kf 1 (smallest shared word 164) precedes kf 2 (400) although it was added later; a minw
            of kf 1 that missed index 64 (INT_MAX) would put it last.  Query C = {50, 164}: kf 2 (50) precedes kf 1: both orders occur.
      kf 3  128 even words 1000..1254: it shares 1126 (index 63, lane 63) and 1128 (index 64, lane 0 again) with query B.
      kf 4  [1127, 3000], added BEFORE kf 3.  Query B = {1126, 1127, 1128, 3000}: kf 3 (1126) precedes kf 4 (1127); if lane 0's 1128 won, kf 4 would lead.
      kf 5  [0, 31, 32, n_words - 1]: first / last bit of a bitmap word, last word of the vocabulary; query D is the same set.
      kf 6  empty row; kf 7 one word; kf 8 / 9 / 10: 63 / 64 / 65 words, query E shares only the LAST word of each (indices 62, 63, 64).
      Query F holds 301 words (k_qbitmap's lanes take a second pass) covering kf 8..10 whole.  Query G is empty, query H shares a word with nothing.
    Small vocabularies (1, 32, 33 words): rows [0], [], all words, [n - 1], [0, 31], [31, 32] as far as they fit, and queries over the same sets."""
    nw = n_words
    if nw >= 6999:
        kfs = [(2, *uni([50, 400])), (1, *uni(range(100, 229))), (4, *uni([1127, 3000])), (3, *uni(range(1000, 1256, 2))), (5, *uni([0, 31, 32, nw - 1])),
               (6, [], []), (7, *uni([nw - 1])), (8, *uni(range(5000, 5063))), (9, *uni(range(5100, 5164))), (10, *uni(range(5200, 5265)))]
        qs = {"A": uni([164, 400]), "B": uni([1126, 1127, 1128, 3000]), "C": uni([50, 164]), "D": uni([0, 31, 32, nw - 1]), "E": uni([5062, 5163, 5264]),
              "F": uni(range(5000, 5301)), "G": ([], []), "H": uni([4000])}
    else:
        rows = [[0], [], list(range(nw)), [nw - 1]] + ([[0, 31]] if nw >= 32 else []) + ([[31, 32]] if nw >= 33 else [])
        kfs = [(i + 1, *(uni(r) if r else ([], []))) for i, r in enumerate(rows)]
        qs = {"A": uni([0]), "B": uni([nw - 1]), "C": uni(range(nw)), "G": ([], [])}
        if nw >= 32:
            qs["D"] = uni([0, 31])
        if nw >= 33:
            qs["E"] = uni([32])
            qs["F"] = uni([31, 32])
    names = sorted(qs)
    batch, order = [], []
    for k in range(17):
        n = names[k % len(names)]
        batch.append((1000 + k, *qs[n]))
        order.append(n)
    script = [("covis", 1, [2, 3]), ("covis", 3, [4]), ("add", kfs), ("reloc", batch)]
    return script, order


def geometry_all_empty(n_words):
    """a database whose rows are all empty: nothing shares a word with anything"""
    return [("add", [(i, [], []) for i in range(1, 7)]), ("reloc", [(50, *uni([0, n_words - 1])), (51, [], [])]),
            ("loop", [(1, [], [], 0.0, []), (52, *uni([0]), 0.0, [2])])]


# ------------------------------------------------------------------ 2. slot and query counts (k_count's 4 slots, the 256-thread blocks, KF_QG = 16)

SLOT_COUNTS = (1, 3, 4, 5, 255, 256, 257)
BATCHES = [(nq, S) for S in (5, 257) for nq in (1, 15, 16, 17, 32, 33)]
SLOT_WORDS = 64
TRAP_FIRST, TRAP_LAST = uni([0, 10]), uni(range(6))


def slots(S, nq, seed=0):
    """S slots over 64 words: keyframes 1 .. S - ghosts are added in one call, the last ids are ghosts (named as neighbours only), every 7th added keyframe
    from 3 on is erased.  Rows are 2..6 words of 32..63, except kf 1 = [0..5] and kf 2 = [0, 10] with kf 2 the neighbour of kf 1.
    Batch: the first query {0, 10} scores kf 2 (2 shared words; kf 1 with 1 is below minCommonWords = 1), the LAST query {0..5} scores kf 1 and visits kf 2
    without scoring it (1 shared word, minCommonWords = 4), so kf 1's accumulated score reads what the first query of the batch wrote (trap (c)).  Between
    them: fresh ids, an id repeated inside the batch, id 0, over random words of 32..63 (and word 0 now and then, which revisits kf 1 and kf 2)."""
    rng = np.random.default_rng(1000 * S + nq + seed)
    nghost = 0 if S < 3 else max(1, S // 8)
    added = list(range(1, S - nghost + 1))
    everyone = list(range(1, S + 1))
    script = []
    kfs = []
    for i in added:
        if i == 1:
            kfs.append((1, *TRAP_LAST))
        elif i == 2:
            kfs.append((2, *TRAP_FIRST))
        else:
            kfs.append((i, *uni(sorted(rng.choice(np.arange(32, 64), int(rng.integers(2, 7)), replace=False).tolist()))))
    for i in added[2::3] + everyone[len(added):][:1]:   # some covisibility lists before the add: their slots (ghosts among them) come first
        script.append(("covis", i, [int(x) for x in rng.choice(everyone, min(3, S), replace=False)]))
    script.append(("add", kfs))
    ghosts = everyone[len(added):-1]   # the last one is named by kf 1 below; the others ten at a time by the last keyframes that stay in the database
    hosts = [i for k, i in enumerate(added) if k > 2 and (k - 2) % 7][::-1]
    for j in range(0, len(ghosts), 10):
        script.append(("covis", hosts[j // 10], ghosts[j:j + 10]))
    if S >= 2:
        script.append(("covis", 1, [2] + ([S] if S >= 3 else [])))
    erased = added[2::7] if S >= 4 else []
    if erased:
        script.append(("erase", erased))
    qs = [(100, *TRAP_FIRST)]
    for k in range(1, nq - 1):
        words = sorted(rng.choice(np.arange(32, 64), int(rng.integers(3, 9)), replace=False).tolist())
        if k % 4 == 0:
            words = [0] + words
        qid = 0 if k % 5 == 3 else (qs[-1][0] if k % 5 == 1 and k > 1 else 100 + k)
        qs.append((qid, *uni(words)))
    if nq >= 2:
        qs.append((100 + nq, *TRAP_LAST))
    script.append(("reloc", qs))
    script.append(("loop", [(q[0], q[1], q[2], 0.0, [int(x) for x in rng.choice(everyone, min(2, S), replace=False)] if k % 3 == 1 else [])
                            for k, q in enumerate(qs)]))
    return script


# ------------------------------------------------------------------ 3. state across reallocation

REALLOC_BLOCKS = (100, 200, 300, 620)   # slots after each round's add: the state arrays hold 256 after round 0, 600 after round 2, 1240 after round 3


def realloc():
    """Four rounds; round r adds keyframes up to REALLOC_BLOCKS[r] slots and then queries in both forms with EQUAL query ids, relocalisation first.  The state
    arrays get their first capacity (256) at round 0, stay through round 1 (200 slots: the round that leaves counters, query ids and scores behind) and are
    reallocated at round 2 (300 slots -> 600) and at round 3 (620 slots -> 1240); the hook "grow<r>" marks the moment before the reallocating query.

    Two pairs carry the scores: kf 1 = [0..5] with neighbour kf 2 = [0, 10] (slots 0, 1) and kf 290 = [20..25] with neighbour kf 291 = [20, 30] (slots 289,
    290: past 256, added in round 2).  kf 3 = [15, 16] and kf 292 = [15, 17] carry a query id; kf 4 = [14, 18] names kf 2 and kf 293 = [13, 19] names kf 291.
    Each round's batch, ids 1000 + 10 r + k unless said otherwise:
      k = 0  under the id of the PREVIOUS round's k = 3 query, {13..19}: kf 3 and kf 292 still store that id, so their counters continue and they are not
             appended (trap (b)); kf 4 and kf 293 are appended and scored, and their neighbours kf 2 / kf 291, not visited, still store that id with the
             counter (2 > minCommonWords = 1) and the score of the previous round: both forms add that stale score (the loop form's only way to one)
      k = 1  {0..5}: scores kf 1, visits kf 2 without scoring it: relocalisation adds the score kf 2 got in the PREVIOUS round (trap (a)); the loop form
             skips it (1 word, minCommonWords = 4)
      k = 2  {20..25}: the same for kf 290 / kf 291
      k = 3  {0, 10, 15, 20, 30}: scores kf 2 and kf 291 (what the next round reads) and leaves its id in kf 3 and kf 292 (one shared word each: visited,
             not above minCommonWords = 1)
      k = 4  six random words of 32..63 (the bulk: every other keyframe's state moves)
    The loop batch repeats ids and words with min score 0 and, for k = 4, a connected set."""
    rng = np.random.default_rng(77)
    script, have = [], 0

    def row(i):
        special = {1: list(range(6)), 2: [0, 10], 3: [15, 16], 4: [14, 18], 290: list(range(20, 26)), 291: [20, 30], 292: [15, 17], 293: [13, 19]}
        return (i, *uni(special.get(i) or sorted(rng.choice(np.arange(32, 64), int(rng.integers(2, 7)), replace=False).tolist())))

    for r, upto in enumerate(REALLOC_BLOCKS):
        script.append(("add", [row(i) for i in range(have + 1, upto + 1)]))
        for i in range(have + 1, upto + 1, 9):
            script.append(("covis", i, [int(x) for x in rng.choice(np.arange(1, upto + 1), 4, replace=False) if x != i]))
        script += [("covis", 1, [2]), ("covis", 4, [2])]
        if upto >= 293:
            script += [("covis", 290, [291]), ("covis", 293, [291])]
        have = upto
        script.append(("hook", "grow%d" % r))
        base = 1000 + 10 * r
        qs = [(base - 10 + 3, *uni(range(13, 20))), (base + 1, *uni(range(6))), (base + 2, *uni(range(20, 26))), (base + 3, *uni([0, 10, 15, 20, 30])),
              (base + 4, *uni(sorted(rng.choice(np.arange(32, 64), 6, replace=False).tolist())))]
        script.append(("reloc", qs))
        script.append(("loop", [(q[0], q[1], q[2], 0.0, [5, 6, 290] if k == 4 else []) for k, q in enumerate(qs)]))
    return script


def zero_state(from_id=0):
    """mutation for the hooks of realloc(): the state of keyframes with id >= from_id is lost (ids are slots + 1 in that script)"""
    def f(mod):
        for i, k in mod.kf.items():
            if i >= from_id:
                k.mnRelocQuery = k.mnRelocWords = k.mnLoopQuery = k.mnLoopWords = 0
                k.mRelocScore = k.mLoopScore = 0.0
    return f


# ------------------------------------------------------------------ 4. long lists through k_final

LONG_COUNTS = (1023, 1024, 1025, 2049)
LONG_QUERY = ([1, 2], [0.75, 0.25])
LONG_ROW = ([1, 2], [0.5, 0.5])      # scores 0.75 against LONG_QUERY; a row equal to the query scores 1.0
LONG_READDED = lambda n: [3, n // 2, n]   # noqa: E731


def long_list(n, pattern):
    """n keyframes with the same two-word row, so every one is in the list and the order is add order alone; kf 3, n // 2 and n are erased and added again, so they
    go last, in that order.  pattern "mixed": covisibility by id % 4: none / itself / the same neighbour twice / ten neighbours; all scores are equal, so
    every entry stays its own best and only the ten-neighbour entries are retained (accumulated 8.25 against 0.75, 1.5, 2.25): about n / 4 candidates.
    pattern "common": kf 1's row equals the query (score 1.0) and every other keyframe names it: every other entry's best is kf 1, and dedup returns [1]."""
    kfs = [(i, *(LONG_QUERY if pattern == "common" and i == 1 else LONG_ROW)) for i in range(1, n + 1)]
    script = [("add", kfs)]
    for i in range(1, n + 1):
        if pattern == "common":
            nb = [1] if i != 1 else []
        else:
            nb = [[], [i], [i % n + 1, i % n + 1], [(i + k) % n + 1 for k in range(10)]][i % 4]
        if nb:
            script.append(("covis", i, nb))
    re = LONG_READDED(n)
    script += [("erase", re), ("add", [kfs[i - 1] for i in re])]
    return script


def long_queries(n):
    """the calls on the mixed list: a full one, the caller's cap below the count, the diagnostics cap below the list length, then the FIRST id again: the
    refused calls left the state alone, so every keyframe still stores that id, nothing is appended and there is no candidate (had a refused call been
    committed, everything would be appended again); then fresh ids, a batch of two, and the loop form at and one ulp above the common score"""
    q = lambda i: [(i, *LONG_QUERY)]   # noqa: E731
    return [("reloc", q(7000)), ("reloc", q(7001), {"cap": 3, "expect": "capacity"}), ("reloc", q(7002), {"dcap": 100, "expect": "capacity"}), ("reloc", q(7000)),
            ("reloc", q(7003) + q(7004)), ("loop", q_loop(7005, 0.0)), ("loop", q_loop(7006, 0.75) + q_loop(7007, 0.7500000000000001)),
            host_score(LONG_QUERY, [1, 2, n])]


def host_score(query, ids):
    """the last operation of a script with refused calls: a score call in HOST memory whatever the kind of the run, so it stages its arrays in the context's
    block; a refused call that had kept its claim on the block would make it fail"""
    return ("score", *query, list(ids), {"host": True})


def q_loop(i, min_score, conn=()):
    return [(i, *LONG_QUERY, min_score, list(conn))]


def count_only():
    """cap = 0 with null cand_ids.  Loop form: kf 2 = [8, 9], kf 4 = [5] with kf 2 as its neighbour.  Call 1: query id 7 over {8, 9} with min score +inf and no
    room for candidates: kf 2 is appended and scored (its loop query id, counter and score are state now), nothing passes +inf, so no query has a candidate,
    the call succeeds and commits.  Call 2: id 7 again over {5}: kf 4 is appended and scored (minCommonWords = 0); its neighbour kf 2 is not visited but
    still stores id 7 with 2 words, so the score of call 1 is added to kf 4's.  Had call 1 not committed, kf 2 would store id 0 and add nothing."""
    return [("add", [(2, *uni([8, 9])), (4, *uni([5]))]), ("covis", 4, [2]),
            ("loop", [(7, *uni([8, 9]), math.inf, [])], {"cap": 0, "null_cands": True}), ("hook", "after_count_only"),
            ("loop", [(7, *uni([5]), 0.0, [])]), ("reloc", [(7, *uni([5, 8]))]), host_score(uni([5, 8]), [2, 4])]


# ------------------------------------------------------------------ 5. thresholds and ties

def retention():
    """query {1: 1.0}: kf 1 {1: 1.0} scores 1.0 (kept), kf 2 {1: 0.75, 2: 0.25} exactly 0.75 = 0.75 * best (dropped: the test is >), kf 3 one ulp above (kept)"""
    return [("add", [(1, [1], [1.0]), (2, [1, 2], [0.75, 0.25]), (3, [1, 2], [0.75 + ULP_075, 0.25 - ULP_075])]), ("reloc", [(10, [1], [1.0])]),
            ("loop", [(11, [1], [1.0], 0.0, [])])]


def best_neighbour():
    """query = LONG_QUERY.  kf 1, 4, 5 score 0.75 (LONG_ROW), kf 2 and 3 score 1.0.  kf 1's neighbours are [3, 2]: equal higher scores, the first (3) wins.
    kf 4's neighbour is kf 5 with a score equal to its own: kf 4 stays its own best.  kf 6 (score 1.0) has the neighbours [2, 3]: equal to its own, it stays."""
    return [("add", [(1, *LONG_ROW), (2, *LONG_QUERY), (3, *LONG_QUERY), (4, *LONG_ROW), (5, *LONG_ROW), (6, *LONG_QUERY)]),
            ("covis", 1, [3, 2]), ("covis", 4, [5]), ("covis", 6, [2, 3]), ("reloc", [(10, *LONG_QUERY)]), ("loop", [(11, *LONG_QUERY, 0.0, [])])]


MIN_COMMON = {4: 3, 5: 4, 9: 7, 10: 8}   # maxCommonWords -> static_cast<int>(max * 0.8)


def min_common(m):
    """kf 1 shares m words with the query, kf 2 exactly minCommonWords (not scored: the test is >), kf 3 one more (scored)"""
    t = MIN_COMMON[m]
    return [("add", [(1, *uni(range(m))), (2, *uni(list(range(t)) + [20])), (3, *uni(list(range(t + 1)) + [21]))]), ("reloc", [(10, *uni(range(m)))]),
            ("loop", [(11, *uni(range(m)), 0.0, [])])]


LOOP_SCORE = 0.75   # LONG_ROW against LONG_QUERY


def loop_min_scores():
    """loop form over two keyframes that score 0.75 and one that scores 1.0: min score equal to 0.75 (all pass: >=), one ulp above (only the 1.0 one), -inf,
    +inf (nothing), NaN (si >= NaN is false: nothing), each under a fresh id"""
    mins = [LOOP_SCORE, LOOP_SCORE + ULP_075, -math.inf, math.inf, math.nan, 1.0, 1.0 + 2.0 ** -52]
    return [("add", [(1, *LONG_ROW), (2, *LONG_QUERY), (3, *LONG_ROW)]), ("covis", 1, [2, 3]), ("covis", 3, [1])] + \
           [("loop", q_loop(20 + k, m)) for k, m in enumerate(mins)] + [("loop", [q_loop(40 + k, m)[0] for k, m in enumerate(mins)])]


def connected_sets():
    """loop form over five keyframes that score 0.75 and kf 6 that scores 1.0; kf 3 names kf 4 and kf 5.  Connected sets (a) of ids the database never saw,
    (b) with the query keyframe itself, (c) with duplicates: kf 4 and kf 5 keep query id 2 and end with counter 1, (d) query id 2 AGAIN with kf 4 connected:
    its stored id already equals the query's, so trap (b) wins over the connected-set reset: the counter continues to 3, and kf 3's accumulated score takes
    the stale scores of kf 4 and kf 5 (3 > minCommonWords = 1; a reset counter of 1 would not pass).  Then a batch of the same kinds."""
    return [("add", [(i, *LONG_ROW) for i in range(1, 6)] + [(6, *LONG_QUERY)]), ("covis", 1, [2, 3, 6]), ("covis", 2, [1, 6]), ("covis", 3, [4, 5]),
            ("loop", q_loop(1, 0.0, [900, 901])), ("loop", q_loop(2, 0.0, [2])), ("loop", q_loop(3, 0.0, [4, 4, 5, 4])), ("loop", q_loop(2, 0.0, [4])),
            ("loop", q_loop(1, 0.0, [2, 3]) + q_loop(4, 0.0, [1, 1, 900, 4]) + q_loop(4, 0.0, [6]))]


# ------------------------------------------------------------------ 6. ids

BIG = 2 ** 32 + 1


def wide_ids():
    """keyframes 1 and 2^32 + 1 are two slots with different rows; the same pair and -1, INT64_MIN, INT64_MAX as query ids"""
    return [("add", [(1, *LONG_ROW), (BIG, *LONG_QUERY), (INT64_MAX, *uni([1, 3])), (INT64_MIN, *uni([2, 3])), (-1, *uni([1, 2]))]),
            ("covis", 1, [BIG, INT64_MIN]), ("covis", BIG, [1]), ("covis", -1, [INT64_MAX, 1]),
            ("reloc", [(1, *LONG_QUERY), (BIG, *LONG_QUERY), (1, *uni([1, 3])), (-1, *LONG_QUERY), (INT64_MIN, *LONG_QUERY), (INT64_MAX, *uni([2, 3]))]),
            ("loop", [(BIG, *LONG_QUERY, 0.0, [1]), (1, *LONG_QUERY, 0.0, [BIG]), (INT64_MIN, *uni([1, 3]), 0.0, [-1, INT64_MAX]), (-1, *uni([1]), 0.0, [])])]


def erased_best():
    """kf 2 (score 1.0) is scored by query id 9 and then erased; kf 1 (score 0.75) is added afterwards with kf 2 as its neighbour; query id 9 AGAIN: kf 2 is
    not visited, but still stores id 9 and its score, so it is kf 1's best keyframe and the candidate returned is the erased kf 2"""
    return [("add", [(2, *LONG_QUERY)]), ("reloc", [(9, *LONG_QUERY)]), ("erase", [2]), ("add", [(1, *LONG_ROW)]), ("covis", 1, [2]),
            ("reloc", [(9, *LONG_QUERY)]), ("reloc", [(10, *LONG_QUERY)])]


# ------------------------------------------------------------------ 7. mcs_kfdb_add and mcs_kfdb_score

INVALID = -1
ADD = "mcs_kfdb_add: "
T_RANGE, T_ORDER = ADD + "word id out of range", ADD + "word ids of a BowVector must be strictly ascending"
T_MONOTONE, T_FIRST = ADD + "offsets must be non-decreasing", "offsets[0] must be 0"
T_QUERY_RANGE, T_QUERY_ORDER = "query BowVector: word id out of range", "query BowVector: word ids must be strictly ascending"   # device kind: found by k_qbitmap


def add_calls(n_words=40):
    """a batched add with empty rows in the middle, then every refusal (code and text), each followed by the size check kfdb_pack.check makes after an add,
    and a query at the end that must still equal the model: a refused call has touched nothing, a batch whose second id is present has added nothing"""
    nw = n_words
    good = [(1, *uni([0, 5, 31, 32, nw - 1])), (2, [], []), (3, [], []), (4, *uni([5, 6])), (5, [], []), (6, *uni([nw - 1]))]
    refuse = lambda t: {"expect": (INVALID, t)}   # noqa: E731
    return [("add", good),
            ("add", [(10, *uni([1, nw]))], refuse(T_RANGE)), ("add", [(10, *uni([1, 2])), (11, [-1], [1.0])], refuse(T_RANGE)),
            ("add", [(10, [3, 3], [0.5, 0.5])], refuse(T_ORDER)), ("add", [(10, [4, 3], [0.5, 0.5])], refuse(T_ORDER)),
            ("add", [(10, *uni([1])), (11, *uni([2])), (10, *uni([3]))], refuse(ADD + "keyframe 10 appears twice in one call")),
            ("add", [(10, *uni([1])), (4, *uni([2]))], refuse(ADD + "keyframe 4 is already in the database")),
            ("add_raw", [10, 11], [0, 10, 4], [1, 2, 3, 4], [0.25] * 4, refuse(T_MONOTONE)),
            ("add_raw", [10], [0, -1], [1], [1.0], refuse(T_MONOTONE)),
            ("add_raw", [10, 11], [1, 2, 3], [1, 2, 3], [1.0] * 3, refuse(T_FIRST)),
            ("reloc", [(50, *uni([5, 6, nw - 1])), (51, *uni([1, 2, 3]))]),
            ("add", [(10, *uni([1, 2])), (11, [], []), (12, *uni([3]))]),
            ("reloc", [(52, *uni([1, 2, 3, 5]))])]


def bad_queries(n_words=40):
    """a detection query with a word out of range and one with descending words, each in a batch behind a good query (whose state change must not stay), in
    both forms; then a host-memory score call (host_score), then the good query alone.  Host kind: the guard's texts; device kind: k_qbitmap's."""
    nw = n_words
    good, later = (60, *uni([5, 6])), (61, *uni([5, 6, 31]))
    r = lambda form, host, dev: {"refuse": {False: (INVALID, "mcs_kfdb_detect_%s: %s" % (form, host)), True: (INVALID, dev)}}   # noqa: E731
    rel, lp = r("relocalisation", "word id out of range", T_QUERY_RANGE), r("loop", "word id out of range", T_QUERY_RANGE)
    rel2 = r("relocalisation", "word ids of a BowVector must be strictly ascending", T_QUERY_ORDER)
    lp2 = r("loop", "word ids of a BowVector must be strictly ascending", T_QUERY_ORDER)
    lq = lambda q: (*q, 0.0, [])   # noqa: E731
    return [("add", [(1, *uni([5, 6, 31])), (2, *uni([5, 32])), (3, *uni([6, nw - 1]))]), ("covis", 1, [2, 3]), ("covis", 2, [1]),
            ("reloc", [good, (62, [5, nw], [0.5, 0.5])], rel), ("reloc", [good, (62, [6, 5], [0.5, 0.5])], rel2), ("reloc", [good, (62, [5, 5], [0.5, 0.5])], rel2),
            ("loop", [lq(good), lq((62, [-1, 5], [0.5, 0.5]))], lp), ("loop", [lq(good), lq((62, [31, 6], [0.5, 0.5]))], lp2),
            host_score(uni([5, 6]), [1, 2, 3]), ("reloc", [later, good]), ("loop", [lq(later), lq(good)])]


SCORE_COUNTS = (0, 1, 255, 256, 257)


def score_calls(nkf):
    """mcs_kfdb_score against nkf stored keyframes (k_score_list: 256-thread blocks), kf 2 with an empty row, then with an empty query, then naming an erased
    id (refused; nothing is written)"""
    rng = np.random.default_rng(nkf)
    kfs = [(i, *(([], []) if i == 2 else uni(sorted(rng.choice(64, int(rng.integers(1, 9)), replace=False).tolist())))) for i in range(1, nkf + 1)]
    ids = list(range(1, nkf + 1))
    q = uni(sorted(rng.choice(64, 12, replace=False).tolist()))
    script = ([("add", kfs)] if kfs else []) + [("score", *q, ids), ("score", [], [], ids)]
    if nkf >= 2:
        script += [("erase", [nkf]), ("score", *q, ids, {"expect": (INVALID, "mcs_kfdb_score: keyframe %d is not in the database" % nkf)}), ("score", *q, ids[:-1])]
    return script


SLAB_ADDS, SLAB_ROW, SLAB_WORDS = 40, 5, 256


def slab_growth():
    """40 add calls of one keyframe each, 5 words per row, into a database created without a capacity hint: the slab holds 64 elements from the first add,
    128 from the 13th (60 elements of 12 rows behind it) and 256 from the 26th (125 elements of 25 rows).  Row i (keyframe i + 1) = words i, 40 + i, ...,
    160 + i with values that differ from row to row, so a row lost or shifted by a reallocation shows in its score.  Then one score call over all 40
    keyframes against every word, and one relocalisation query {0, 39} that shares a word with the first row and with the last."""
    def row(i):
        raw = [1.0 + (i + 3 * k) % 7 for k in range(SLAB_ROW)]
        return (i + 1, [i + SLAB_ADDS * k for k in range(SLAB_ROW)], [x / sum(raw) for x in raw])

    return [("add", [row(i)]) for i in range(SLAB_ADDS)] + \
           [("score", *uni(range(SLAB_ADDS * SLAB_ROW)), list(range(1, SLAB_ADDS + 1))), ("reloc", [(500, *uni([0, SLAB_ADDS - 1]))])]


# ------------------------------------------------------------------ 8. mcs_bow_vector: a root with N leaf children

VOC_LEAVES = 4200
BOW_COUNTS = (0, 1, 1023, 1024, 1025, 4097)
BOW_PATTERNS = ("same", "same_plus_one", "distinct", "zeros", "stop_mixed")


def vocabulary():
    """-> (node_desc, child_off, child_idx, word id per node, weight per node) of a root (node 0) with VOC_LEAVES leaves.  word = node * 37 mod VOC_LEAVES (a
    bijection: rank order differs from node order); weight 0 for every 7th node (stop words), else (1 + (node % 5) / 8 + node / 10 000) * 2^e with e running from -40 to 20
    (a full mantissa: k additions of it are not k times it)."""
    N = VOC_LEAVES
    nodes = np.arange(1, N + 1)
    word = np.concatenate([[-1], (nodes * 37) % N]).astype(np.int32)
    e = -40.0 + 60.0 * (nodes - 1) / (N - 1)
    wt = np.where(nodes % 7 == 0, 0.0, (1.0 + (nodes % 5) / 8.0 + 1e-4 * nodes) * np.exp2(np.round(e)))
    weight = np.concatenate([[0.0], wt]).astype(np.float64)
    child_off = np.concatenate([[0], np.full(N + 1, N)]).astype(np.int32)
    return np.zeros((N + 1, 32), np.uint8), child_off, nodes.astype(np.int32), word, weight


def leaves(n, pattern):
    """n leaf node ids.  same: one weighted node n times; same_plus_one: that node n - 1 times, then another (a lone word normalises to 1.0 whatever its
    sum was; with a second word the sum shows); distinct: n different nodes, shuffled, stop words among them; zeros: stop words only; stop_mixed: 80 nodes,
    stop words among them, drawn with repetition"""
    rng = np.random.default_rng(n)
    if pattern == "same":
        return np.full(n, 1234, np.int32)
    if pattern == "same_plus_one":
        return np.array([1234] * (n - 1) + [4001][:n], np.int32)
    if pattern == "distinct":
        return rng.permutation(np.arange(1, VOC_LEAVES + 1))[:n].astype(np.int32)
    if pattern == "zeros":
        return (7 * rng.integers(1, VOC_LEAVES // 7, n)).astype(np.int32)
    if pattern == "stop_mixed":
        return rng.choice(np.arange(1, VOC_LEAVES + 1, 53), n).astype(np.int32) if n else np.zeros(0, np.int32)
    raise ValueError(pattern)
