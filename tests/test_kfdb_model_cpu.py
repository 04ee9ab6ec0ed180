"""Known answers, derived by hand from src/cMultiKeyFrameDatabase.cpp, for the keyframe-database model (tests/kfdb_model.py) the device
database is checked against: one case at least per trap of DESIGN.md section 7."""
import kfdb_model as M


def kf(i, words, val=0.1, neighbours=()):
    return M.KF(i, [(w, val) for w in words], neighbours)


def db_with(*kfs, n_words=32):
    db = M.Database(n_words)
    for k in kfs:
        db.add(k)
    return db


def trace_ids(db, qid, words):
    t = []
    db.DetectRelocalisationCandidates(qid, [(w, 0.1) for w in words], trace=t)
    return [e[0] for e in t]


def test_list_order_smallest_shared_word_then_add_order():
    A, B, C = kf(1, [5, 9]), kf(2, [3, 9]), kf(3, [9])
    db = db_with(A, B, C)
    # word 3 appends B, word 5 appends A, word 9 appends C; counts B 2, A 2, C 1; min = int(1.6) = 1 -> C is not scored
    assert trace_ids(db, 10, [3, 5, 9]) == [2, 1]
    assert (A.mnRelocWords, B.mnRelocWords, C.mnRelocWords) == (2, 2, 1)


def test_readd_moves_a_keyframe_last():
    A, B = kf(1, [4]), kf(2, [4])
    db = db_with(A, B)
    assert trace_ids(db, 10, [4]) == [1, 2]
    db.erase(A)
    assert trace_ids(db, 11, [4]) == [2]
    db.add(A)
    assert trace_ids(db, 12, [4]) == [2, 1]


def test_min_common_words_truncates_and_is_strict():
    A, B = kf(1, [1, 2, 3, 4]), kf(2, [1, 2, 3])
    db = db_with(A, B)
    t = []
    db.DetectRelocalisationCandidates(10, [(w, 0.25) for w in (1, 2, 3, 4)], trace=t)
    assert [e[:2] for e in t] == [(1, 4)]            # max 4 -> int(3.2) = 3; B shares 3, needs > 3
    C = kf(3, [1, 2, 3, 4, 5])
    db.add(C)
    t = []
    db.DetectRelocalisationCandidates(11, [(w, 0.2) for w in (1, 2, 3, 4, 5)], trace=t)
    assert [e[:2] for e in t] == [(3, 5)]            # max 5 -> int(4.0) = 4; A shares 4, needs > 4


def test_l1_score_depends_on_summation_order():
    x = 2.0 ** -54
    v = [(1, 1.0), (2, x), (3, x), (4, x)]
    # terms in ascending word order: -2, then three times -2^-53, each a quarter ulp of 2 -> the sum stays -2
    assert M.l1_score(v, v) == 1.0
    s = 0.0
    for _, a in reversed(v):                         # the same terms the other way round: -3 * 2^-53 first, then -2 rounds away
        s += abs(a - a) - abs(a) - abs(a)
    assert -s / 2.0 == 1.0 + 2.0 ** -52


def test_l1_score_takes_vi_from_the_first_vector():
    v = [(0, 0.04808522976722815), (1, 0.08469778693977133), (2, 0.0002340059279011881), (3, 0.04948746600608905), (4, 0.0801711147045314),
         (5, 0.02541802458560585), (6, 0.10503007728376915), (7, 0.10015860640127595), (8, 0.0033988870037281707)]
    w = [(0, 0.0028273178881623113), (1, 0.06015694142149962), (2, 0.10434990697539007), (3, 0.04235602640980138), (4, 0.024066599681179263),
         (5, 0.046901841731413034), (6, 0.003226754174985327), (7, 0.02463240736367056), (8, 0.04865417707228578)]
    assert M.l1_score(v, w) == 0.18631696445653367 and M.l1_score(w, v) == 0.18631696445653365


def test_unscored_neighbour_reads_its_stale_score_or_zero():
    N = kf(3, [1, 2, 3, 4, 5])
    A = kf(1, [1, 2, 3, 4, 5, 6, 7, 8, 9, 10], 0.1, [N])
    db = db_with(A, N)
    q1 = [(w, 0.2) for w in (1, 2, 3, 4, 5)]
    t = []
    db.DetectRelocalisationCandidates(10, q1, trace=t)    # both share 5 words: both scored
    stale = N.mRelocScore
    assert [e[0] for e in t] == [1, 3] and stale > 0
    # query 2 shares 10 words with A, 5 with N: N is visited (mnRelocQuery = 11) but not scored (5 <= int(8.0)) -> A adds N's score of query 1
    q2 = [(w, 0.1) for w in range(1, 11)]
    t = []
    out = db.DetectRelocalisationCandidates(11, q2, trace=t)
    sA = M.l1_score(q2, A.bow)
    assert t == [(1, 10, sA, sA + stale, 1 if sA >= stale else 3)]
    assert N.mRelocScore == stale and [k.mnId for k in out] == [t[0][4]]
    # a neighbour never scored reads 0.0
    N2 = kf(4, [1, 2])
    B = kf(2, list(range(1, 11)), 0.1, [N2])
    db2 = db_with(B, N2)
    t = []
    db2.DetectRelocalisationCandidates(12, q2, trace=t)
    sB = M.l1_score(q2, B.bow)
    assert t == [(2, 10, sB, sB + 0.0, 2)] and N2.mnRelocQuery == 12 and N2.mRelocScore == 0.0


def test_loop_connected_keyframe_counter_quirk():
    Cn, A = kf(2, [1, 2, 3]), kf(3, [1, 2, 3])
    db = db_with(Cn, A)
    Q = kf(9, [1, 2, 3])
    out = db.DetectLoopCandidates(Q, 0.0, connected=[Cn])
    assert [k.mnId for k in out] == [3]
    assert Cn.mnLoopWords == 1 and Cn.mnLoopQuery == 0      # reset to 0 on every visit, query id never set
    assert A.mnLoopWords == 3 and A.mnLoopQuery == 9


def test_loop_neighbour_needs_the_word_count():
    N = kf(3, [1])
    A = kf(1, [1, 2, 3, 4, 5], 0.2, [N])
    db = db_with(A, N)
    Q = kf(9, [1, 2, 3, 4, 5], 0.2)
    t = []
    db.DetectLoopCandidates(Q, 0.0, trace=t)
    sA = M.l1_score(Q.bow, A.bow)
    assert N.mnLoopQuery == 9 and N.mnLoopWords == 1 and t == [(1, 5, sA, sA, 1)]   # N has the query id but 1 <= int(4.0)


def test_best_acc_score_start_and_zero_scores():
    # a score of exactly 0.0 (values of opposite sign): relocalisation starts at 0 and 0 > 0.75 * 0 fails -> no candidate
    A = M.KF(1, [(1, -0.5)])
    db = db_with(A)
    assert db.DetectRelocalisationCandidates(10, [(1, 0.5)]) == []
    # the loop form drops scores below minScore before accumulating, and starts at minScore
    B = kf(2, [1, 2], 0.5)
    db = db_with(B)
    Q = kf(9, [1, 2], 0.5)
    assert db.DetectLoopCandidates(Q, 1.0) == [B]          # score 1.0 >= 1.0 and 1.0 > 0.75
    assert db.DetectLoopCandidates(kf(10, [1, 2], 0.5), 1.0 + 2 ** -52) == []
    assert B.mLoopScore == 1.0                              # written although below minScore


def test_dedup_of_a_best_keyframe_reached_twice():
    C = kf(3, [1, 2, 3, 4], 0.25)
    A = kf(1, [1, 2, 3, 4, 7], 0.2, [C])
    B = kf(2, [1, 2, 3, 4, 8], 0.2, [C])
    db = db_with(A, B, C)
    q = [(w, 0.25) for w in (1, 2, 3, 4)]
    t = []
    out = db.DetectRelocalisationCandidates(10, q, trace=t)
    assert [e[4] for e in t] == [3, 3, 3] and [k.mnId for k in out] == [3]   # C scores 1.0: best of A, B and itself


def test_query_id_reuse_and_id_zero():
    A = kf(1, [1, 2])
    db = db_with(A)
    assert db.DetectRelocalisationCandidates(0, [(1, 0.5), (2, 0.5)]) == []   # never-queried keyframes already hold query id 0
    assert A.mnRelocWords == 2 and A.mnRelocQuery == 0
    assert db.DetectRelocalisationCandidates(5, [(1, 0.5), (2, 0.5)]) == [A]
    assert db.DetectRelocalisationCandidates(5, [(1, 0.5), (2, 0.5)]) == []   # same id again: not appended, counter continues
    assert A.mnRelocWords == 4


def test_query_keyframe_in_the_database_finds_itself():
    P = kf(4, [1, 2, 3], 1 / 3)
    O = kf(5, [1, 9], 0.5)
    db = db_with(P, O)
    t = []
    out = db.DetectLoopCandidates(P, 0.0, trace=t)
    assert out == [P] and t[0][:3] == (4, 3, 1.0)


def test_empty_database_and_empty_query():
    db = M.Database(8)
    assert db.DetectRelocalisationCandidates(1, [(1, 1.0)]) == []
    assert db.DetectLoopCandidates(kf(2, [1]), 0.0) == []
    db.add(kf(1, [1]))
    assert db.DetectRelocalisationCandidates(3, []) == []


def test_bow_vector_accumulates_then_normalises_in_word_order():
    words = [7, 3, 7, 7, 5, 3]
    weights = [0.1, 0.3, 0.1, 0.1, 0.0, 0.3]          # word 5 has weight 0 and drops out
    got = M.bow_vector(words, weights)
    v3, v7 = 0.3 + 0.3, (0.1 + 0.1) + 0.1
    norm = 0.0 + v3 + v7
    assert got == [(3, v3 / norm), (7, v7 / norm)]
