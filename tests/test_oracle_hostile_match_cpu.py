"""CPU: the oracle's three brute-force searches against the independent definition of tests/hostile_descriptors.py on every hostile case, for 16-, 32- and 64-byte
descriptors, masked and unmasked — and the conditions that keep those cases from passing vacuously: every class of boundary decision is present (counted from the
definition's own bookkeeping and printed), the tag code of layout (b) keeps foreign rows out of every decision, the triangulation rays stay clear of the epipolar
bound, and the layout wrappers give back the rows they were given.  Integer results: tolerance 0."""
import numpy as np
import pytest

import hostile_descriptors as H


@pytest.fixture(scope="module")
def O(oracle):
    return oracle


def same(O, S, ratio, define=H.define_search, book=None, **kw):
    dn, dm = define(S, ratio, book, **kw)
    on, om = H.oracle_search(O, S, ratio)
    assert np.array_equal(dn, on) and np.array_equal(dm, om), (S.mode, S.dim, S.masked, ratio, int((dm != om).sum()))
    return dn


@pytest.mark.parametrize("mode,dim,masked", H.CELLS)
def test_decision_table_oracle_equals_definition_and_is_not_vacuous(O, mode, dim, masked, capsys):
    counts = {}
    for ratio in H.RATIOS:
        for kind in ("decision", "contention"):
            for S in H.table(mode, dim, masked, "a", kind):
                book = []
                same(O, S, ratio, H.define_tiny, book)
                if kind == "decision":
                    H.classify(S, ratio, book, counts)
    for kind in ("decision", "contention"):
        for S in H.table(mode, dim, masked, "b", kind):
            keep = {}
            for ratio in H.ratios_b(dim, masked):
                same(O, S, ratio, keep=keep)
    ncases = H.table(mode, dim, masked, "a")[0].meta["nblocks"], H.table(mode, dim, masked, "a", "contention")[0].meta["nblocks"]
    with capsys.disabled():
        print("\n[hostile match] mode %d dim %d masked %d: %d table cases + %d contention cases; classes: %s"
              % (mode, dim, masked, ncases[0], ncases[1], " ".join("%s=%d" % kv for kv in sorted(counts.items()))))
    need = ["accept@TH-1", "accept@TH" if mode == 1 else "reject@TH", "reject@TH+1", "lone-accept", "ratio-equal@0.5", "ratio-equal@0.75", "ratio-equal@1"]
    if masked:
        need += ["odd-%s-%s@1" % (side, what) for side in ("within", "beyond") for what in ("TH", "cap")] + ["even-beyond-cap@1"]   # totals 2 cap + 1 | + 3 | + 2
    assert all(counts.get(k, 0) > 0 for k in need), [k for k in need if counts.get(k, 0) == 0]
    assert ("reject@TH" if mode == 1 else "accept@TH") not in counts   # strict in KF,KF, inclusive in KF,F


@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("masked", [False, True])
def test_layout_b_keeps_foreign_rows_out(dim, masked):
    """a condition, not a measurement: every row of another block lies beyond the largest row of the tables and beyond the list cap of every ratio layout (b) runs with"""
    th = H.th_low(dim, masked)
    caps = [H.list_cap(dim, masked, r) for r in H.ratios_b(dim, masked)]
    assert len(caps) >= 3 and {1.0, 1.25} <= set(H.ratios_b(dim, masked))
    for mode in (0, 1):   # (the tables of the two modes come from different random streams: each is checked, not the construction)
        for kind in ("decision", "contention"):
            S = H.table(mode, dim, masked, "b", kind)[0]
            assert H.min_cross(S) > max([th + 3] + caps), (mode, kind, H.min_cross(S), th + 3, caps)
    for grouped in (True, False):
        assert H.min_cross(H.tri_sets(dim, masked, grouped)) > th + 3   # the triangulation search collects nothing beyond TH_LOW


def test_list_caps():
    """the small ratios push the cap to its 8 * dim ceiling, 1.25 pins it at TH_LOW"""
    for dim in H.DIMS:
        for masked in (False, True):
            assert H.list_cap(dim, masked, 0.1) == 8 * dim and H.list_cap(dim, masked, 1.25) == H.th_low(dim, masked) == H.list_cap(dim, masked, 1.0)
            assert H.list_cap(dim, masked, 0.5) == 2 * H.th_low(dim, masked)


def test_exact_distance_builder():
    """(a, b) -> raw total a unmasked, 2 a + b masked"""
    for dim in H.DIMS:
        for masked in (False, True):
            th = H.th_low(dim, masked)
            blocks = [{"q": [(0, 0)], "t": [(a, b)]} for a in range(th + 4) for b in ((0, 1) if masked else (0,))]
            S = H.assemble_tiny(0, dim, masked, blocks)
            tot = np.array([H.raw_totals(S.dq[s], S.mq[s] if masked else None, S.dt[s], S.mt[s] if masked else None)[0, 0] for s in range(S.nsets)])
            want = np.array([(2 * a + b) if masked else a for a in range(th + 4) for b in ((0, 1) if masked else (0,))])
            assert np.array_equal(tot, want)


@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("masked", [False, True])
def test_triangulation_cases(O, dim, masked):
    th = H.th_low(dim, masked)
    for grouped in (True, False):
        S0 = H.tri_sets(dim, masked, grouped)
        E3 = H.tri_E(S0.nr_cams, np.random.default_rng(3), 3)
        for S in (S0, H.with_E(S0, E3)):
            book = []
            nm = same(O, S, 0.0, book=book)
            # margin: no tested pair within a factor of 2 of the 1e-2 bound; zero matrices give den == 0 (dsqr None)
            dsq = [e[5] for e in book if e[5] is not None]
            assert dsq and all(d < 0.5e-2 or d > 2e-2 for d in dsq), sorted(dsq)[:5]
            if S.nsets == 3:
                assert nm[1] == 0 and nm[0] == nm[2] > 0 and any(e[5] is None for e in book)
            seen = {(e[3], e[4]) for e in book if e[0] == 0}   # (distance, BestDist) of tested candidates of pair 0
            assert (0, 0) in seen and (2, 1) in seen and (th, th) in seen and (6, 3) in seen
            assert not any(d > 2 * b or d > th for d, b in seen)
    # the all-fail-then-pass query: 35 candidates tested, the last one taken
    S = H.tri_sets(dim, masked, True)
    book = []
    H.define_search(S, book=book)
    per_q = {}
    for e in book:
        per_q[e[1]] = per_q.get(e[1], 0) + 1
    assert max(per_q.values()) == 35


def clear_of_the_bound(S):
    """the triangulation margin condition on EVERY pair of one camera: no dsqr within a factor of 2 of 1e-2"""
    dsq = H.tri_margins(S)
    assert all(d < 0.5e-2 or d > 2e-2 for d in dsq), sorted(dsq, key=lambda d: abs(np.log(d / 1e-2)))[:3]
    return len(dsq)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dim,masked", [(dim, masked) for dim in H.DIMS for masked in (False, True)])
def test_degenerate_sets_and_chains(O, mode, dim, masked):
    """the lists tests/test_gpu_hostile_match.py walks (H.degenerate_cases, H.chain_cases): every cell, every K"""
    assert (mode, dim, masked) in H.DEGENERATE_CELLS and len(H.DEGENERATE_CELLS) == 18
    seen = set()
    for K, name, S in H.degenerate_cases(mode, dim, masked):
        nm = same(O, S, H.DEGENERATE_RATIO)
        seen.add(name)
        if mode == 2:
            clear_of_the_bound(S)
        if name in ("queries-invalid", "train-invalid"):
            assert nm.sum() == 0
        if name == "zero-masks" and mode != 2:
            assert nm[0] == 0    # every distance 0: 0 < ratio * 0 never holds (the triangulation search takes rows in index order instead)
    assert {"all-equal", "ones-vs-zeros", "nt=1", "nt=2", "nt=33", "queries-invalid", "train-invalid"} <= seen and (not masked or "zero-masks" in seen)
    assert mode != 2 or {"camera-without-rows", "one-camera"} <= seen
    if (dim, masked) in H.CHAIN_CELLS:
        for K in H.CHAIN_KS:
            for m, ratios, S in H.chain_cases(dim, masked, K):
                for ratio in (ratios if m == mode else ()):
                    assert same(O, S, ratio).sum() > 0


@pytest.mark.parametrize("dim,masked", H.RING_CELLS)
def test_ring_frames(O, dim, masked):
    """every pair the ring calls of the device test compute, pair 0 of (first 0, count 5) against the LAST frame"""
    d, m, v, n, pitch = H.ring_frames(dim, masked)
    for first, count in H.RING_RANGES:
        S = H.ring_sets(dim, masked, first, count)
        assert S.nsets == count and np.array_equal(S.dq[0], d[first, :n]) and np.array_equal(S.dt[0], d[(first - 1) % 5, :n])
        assert (same(O, S, H.RING_RATIO) > 0).all()
    assert np.array_equal(H.ring_sets(dim, masked, 0, 5).dt[0], d[4, :n])


@pytest.mark.parametrize("mode", [0, 1])
def test_claim_table_boundary_sets(O, mode):
    for nt in (16384, 16385):
        assert same(O, H.claim_sets(mode, nt), 0.9).sum() > 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_bait_rows_would_change_the_outcome(mode):
    """the rows a laid-out set does not own (block gaps, pitch tail) are copies of a query the search leaves unmatched: taken for a train row, one of them
    matches that query — shown with the definition on every set of the device's layout test, by appending the row"""
    for dim, masked in H.LAYOUT_CELLS:
        for S in [H.layout_case(mode, dim, masked)] + ([H.tri_sets(dim, masked, False)] if mode == 2 else []):
            desc, ray, pick = H.bait_for(S)
            assert pick is not None and S.vq[pick]
            k, i = pick
            for ratio in H.LAYOUT_RATIOS[mode]:
                n0, m0 = H.define_search(H.one_set(S, k), ratio)
                n1, m1 = H.define_search(H.with_bait_row(S, k), ratio)
                if mode == 1:
                    assert i not in m0[0] and m1[0, S.nt] == i
                else:
                    assert m0[0, i] == -1 and m1[0, i] == S.nt
                assert n1[0] == n0[0] + 1
            if mode == 2:   # the bait's ray passes for ITS query, clearly (no other query comes within TH_LOW of the bait: the tags)
                assert H.epipolar(S.raysq[pick], ray, S.E_of(k)[0])[1] < 0.5e-2
            S2, q, t = H.lay(S, "blocks")
            for L in (q, t):
                owned = np.zeros(L.pitch, bool)
                owned[L.phys] = True
                assert (L.desc[:, ~owned, :S.dim] == desc).all() and (L.rays is None or (L.rays[:, ~owned] == ray).all())


@pytest.mark.parametrize("how", ("plain",) + H.LAYOUTS)
def test_layout_wrappers_round_trip(how):
    for S0 in (H.table(0, 32, True, "b")[0], H.tri_sets(16, False), H.table(1, 64, False, "a")[2]):
        S, q, t = H.lay(S0, how)
        for L, arrs in ((q, (S.dq, S.mq if S.masked else None, S.vq, S.camq, S.raysq)), (t, (S.dt, S.mt if S.masked else None, S.vt, S.camt, S.rayst))):
            for got, want in zip(H.read_side(L), arrs):
                assert (got is None) == (want is None) and (got is None or np.array_equal(got, want))
            assert L.stride >= S.dim and L.stride % 4 == 0 and L.pitch > (L.phys.max() if L.n else -1)
            if how in ("stride4", "stride16"):
                assert (L.desc[:, :, S.dim:] == 0xA5).all()
            if how == "blocks" and L.n >= 3:
                assert L.block_pitch > L.block_rows and L.n % L.block_rows == 0
                owned = np.zeros(L.pitch, bool)
                owned[L.phys] = True
                assert (~owned).sum() >= 5 and (L.valid[:, ~owned] == 1).all()   # bait rows between the blocks
        assert S.nq >= S0.nq and np.array_equal(S.dq[:, :S0.nq], S0.dq)
