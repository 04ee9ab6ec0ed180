"""-m gpu: the search stage (top-K Hamming lists of mcs_match.hip / mcs_match_mfma.hip, the greedy resolution of mcs_greedy.hip, the C ABI of mcs_capi_match.hip)
on the hostile descriptor sets of tests/hostile_descriptors.py, against the oracle, bit for bit: match indices, match counts, and the fallback counter where a case
is built to force exact rescans.  tests/test_oracle_hostile_match_cpu.py shows the oracle equal to an independent definition on the same cases and that every
boundary class is present.

Which form of the greedy pass a call takes follows from its shape (launch_dw / launch_spec_kd of mcs_greedy.hip):
  layout (a) tables     hundreds to thousands of tiny set pairs in one call      -> k_greedy_spec, 4 waves (nsets >= 512) or 8 waves
  layout (b) tables     9 .. 21 set pairs (unmasked) / 2 .. 12 (masked)           -> k_greedy_spec, 8 waves; the first 8 pairs alone and every call of <= 8 pairs: k_greedy_jacobi
  degenerate, chains    one set pair                                              -> k_greedy_jacobi
  triangulation         with camera groups -> k_greedy_spec (TRI); without -> k_greedy
  nt = 16385            -> k_greedy (the claim table of the speculative form ends at 16384 rows)
and the lists: 16 / 32-byte rows without camera groups -> the matrix-core form, 64-byte rows and grouped calls -> the VALU form (all of them under MCS_MATCH_VALU=1)."""
import ctypes as C
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import hostile_descriptors as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = H.KS


@pytest.fixture(scope="module")
def G():
    import gpu_common
    return gpu_common


@pytest.fixture(scope="module")
def cap():
    return importlib.import_module("multicol-slam_amd._capi")


def P(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Pinned:
    """page-locked int32 output arrays (mcs_host_alloc) out of one allocation that grows on demand: a host-kind search whose outputs lie in such memory
    writes them with the output kernel (launch_search_out) instead of three copies"""

    def __init__(self, G):
        self.G, self.p, self.n = G, None, 0

    def take(self, *shapes):
        G = self.G
        sizes = [max(int(np.prod(sh)), 1) * 4 for sh in shapes]
        need = sum((n + 63) // 64 * 64 for n in sizes)
        if need > self.n:
            self.close()
            p = C.c_void_p()
            G.mcs.check(G.mcs.lib().mcs_host_alloc(G.ctx().h, 2 * need, C.byref(p)))
            self.p, self.n = p, 2 * need
        out, at = [], 0
        for sh, n in zip(shapes, sizes):
            a = np.frombuffer((C.c_uint8 * n).from_address(self.p.value + at), np.int32)[:int(np.prod(sh))].reshape(sh)
            a[...] = -7
            out.append((C.c_void_p(self.p.value + at), a))
            at += (n + 63) // 64 * 64
        return out

    def close(self):
        if self.p is not None:
            self.G.mcs.check(self.G.mcs.lib().mcs_host_free(self.G.ctx().h, self.p))
        self.p, self.n = None, 0


@pytest.fixture(scope="module")
def pin(G):
    p = Pinned(G)
    yield p
    p.close()


SWEEPS_1 = os.environ.get("MCS_JACOBI_MAX_SWEEPS") == "1"     # (the third child of test_other_code_paths_agree_on_the_tables)


_expected = {}


def expected(G, S, ratio=0.0):
    key = (id(S), ratio)
    if key not in _expected:
        _expected[key] = (S,) + H.oracle_search(G.O, S, ratio)   # (S kept alive: the key is its id)
    return _expected[key][1:]


class Call:
    """one laid-out Sets on the device's side of the C ABI, host kind and (buffers made on first use) device kind"""

    def __init__(self, G, cap, S, how="plain", groups=True):
        self.G, self.cap = G, cap
        self.S, self.q, self.t = H.lay(S, how)
        self.groups = groups and S.mode == 2
        self.dev = None

    def _sets(self, kind):
        cap, G = self.cap, self.G
        sides = []
        if kind == cap.MEM_DEVICE and self.dev is None:
            self.dev = [[None if a is None else G.DevBuf(a) for a in (L.desc, L.mask, L.valid, L.group, L.rays)] for L in (self.q, self.t)]
            self.devE = None if self.S.E is None else G.DevBuf(np.ascontiguousarray(self.S.E))
        for k, L in enumerate((self.q, self.t)):
            if kind == cap.MEM_HOST:
                adr = [None if a is None else a.ctypes.data for a in (L.desc, L.mask, L.valid, L.group, L.rays)]
            else:
                adr = [None if b is None else b.ptr.value for b in self.dev[k]]
            if L.inter:
                adr[1] = adr[0] + L.dim
            if not self.groups:
                adr[3] = None
            sides.append((cap.DescSet(adr[0], adr[1], adr[2], adr[3], L.n, L.stride, L.block_rows, L.block_pitch), adr[4]))
        return sides

    def run(self, K, ratio, kind, pin=None):
        """-> (match [nsets, n], nmatches [nsets], fallbacks [nsets]); pin: host-kind outputs in page-locked arrays"""
        cap, G, S = self.cap, self.G, self.S
        lib, ctx = G.mcs.lib(), G.ctx()
        (q, rq), (t, rt) = self._sets(kind)
        shape = (S.nsets, self.t.n if S.mode == 1 else self.q.n)
        m, nm, fb = np.full(shape, -7, np.int32), np.full(S.nsets, -7, np.int32), np.full(S.nsets, -7, np.int32)
        if kind == cap.MEM_DEVICE:
            bufs = [G.DevBuf(a) for a in (m, nm, fb)]
            pm, pn, pf = (b.ptr for b in bufs)
        elif pin is not None:
            (pm, m), (pn, nm), (pf, fb) = pin.take(shape, (S.nsets,), (S.nsets,))
        else:
            pm, pn, pf = P(m), P(nm), P(fb)
        if S.mode == 2:
            E = np.ascontiguousarray(S.E)
            pE = C.c_void_p(self.devE.ptr.value) if kind == cap.MEM_DEVICE else P(E)
            nc = S.nr_cams
            if len(E) > 1:
                assert len(E) == S.nsets
                cap.check(lib.mcs_search_triangulation_sweep(ctx.h, S.nsets, C.byref(q), self.q.pitch, C.byref(t), self.t.pitch, rq, rt, pE, nc * nc * 9, nc, S.dim, K,
                                                             kind, pm, pn, pf))
            else:
                cap.check(lib.mcs_search_triangulation(ctx.h, S.nsets, C.byref(q), self.q.pitch, C.byref(t), self.t.pitch, rq, rt, pE, nc, S.dim, K, kind, pm, pn, pf))
        else:
            fn = lib.mcs_search_kf_kf if S.mode == 0 else lib.mcs_search_kf_f
            cap.check(fn(ctx.h, S.nsets, C.byref(q), self.q.pitch, C.byref(t), self.t.pitch, S.dim, ratio, K, kind, pm, pn, pf))
        if kind == cap.MEM_DEVICE:
            ctx.synchronize()
            m, nm, fb = (b.read() for b in bufs)
        elif pin is not None:
            m, nm, fb = m.copy(), nm.copy(), fb.copy()
        return m, nm, fb

    def check(self, K, ratio, kinds, what="", pin=None):
        """device == oracle for every memory kind; -> the fallback counters of the last run"""
        en, em = expected(self.G, self.S, ratio)
        for kind in kinds:
            m, nm, fb = self.run(K, ratio, kind, pin)
            S = self.S
            assert self.G.first_diff(nm, en) is None and self.G.first_diff(m, em) is None, \
                (what, "mode %d dim %d masked %d" % (S.mode, S.dim, S.masked), "K %d ratio %g kind %d" % (K, ratio, kind),
                 self.G.first_diff(nm, en), self.G.first_diff(m, em))
            assert (fb >= 0).all()
            if SWEEPS_1 and S.mode != 2 and S.nsets <= 8:
                # the fixpoint form serves this call, and its budget is one sweep: wherever that sweep changed an outcome (any set pair with a match) the loop
                # is given up and the in-order pass reports every query
                assert (fb[en > 0] == self.q.n).all(), (what, K, ratio, fb, en)
                Call.given_up += int((en > 0).sum())
        return fb

    given_up = 0


def head(S, n):
    """the first n set pairs of S"""
    cut = lambda a: None if a is None else a[:n]
    return H.Sets(S.mode, S.dim, S.masked, cut(S.dq), cut(S.mq), cut(S.vq), cut(S.dt), cut(S.mt), cut(S.vt), meta=dict(S.meta))


# ------------------------------------------------------------------------------------------------------------------- decision tables
@pytest.mark.parametrize("mode,dim,masked", H.CELLS)
def test_table_layout_a_many_tiny_pairs(G, cap, pin, mode, dim, masked):
    """one set pair per table entry (nq = 1 or 2, nt = 0 .. 3): every ratio, every K, host memory (page-locked outputs: the output kernel) and device memory"""
    most = 0
    for kind_ in ("decision", "contention"):
        for S in H.table(mode, dim, masked, "a", kind_):
            call = Call(G, cap, S)
            most = max(most, S.nsets)
            for ratio in H.RATIOS:
                for K in KS:
                    fb = call.check(K, ratio, (cap.MEM_HOST, cap.MEM_DEVICE), "a/" + kind_, pin)
                    if kind_ == "contention" and K == 1:
                        assert fb.sum() > 0, "K = 1: the upper query's only entry is taken whenever the lower one matched"
    assert most >= 512    # the 4-wave speculative form


@pytest.mark.parametrize("mode,dim,masked", H.CELLS)
def test_table_layout_b_tagged_blocks(G, cap, pin, mode, dim, masked):
    """all table entries in a few set pairs, kept apart by their tags; the first 8 pairs again on their own (the fixpoint form takes calls of up to 8 pairs).
    Layout (b) runs the ratios whose list cap the tag code can out-distance (H.ratios_b: 0.9, 1.0, 1.25 unmasked, 0.5 and above masked)"""
    before = Call.given_up
    for kind_ in ("decision", "contention"):
        S = H.table(mode, dim, masked, "b", kind_)[0]
        calls = [Call(G, cap, S)] + ([Call(G, cap, _head8(S))] if S.nsets > 8 else [])
        for call in calls:
            for ratio in H.ratios_b(dim, masked):
                for K in KS:
                    fb = call.check(K, ratio, (cap.MEM_HOST, cap.MEM_DEVICE), "b/" + kind_, pin)
                    if kind_ == "contention" and K == 1:
                        assert fb.sum() > 0
    assert not SWEEPS_1 or Call.given_up > before     # (every cell has a call of at most 8 pairs)


_heads = {}


def _head8(S):
    if id(S) not in _heads:
        _heads[id(S)] = (S, head(S, 8))
    return _heads[id(S)][1]


# ------------------------------------------------------------------------------------------------------------------- degenerate sets
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("masked", [False, True])
def test_degenerate_sets_and_nt_around_K(G, cap, mode, dim, masked):
    assert (mode, dim, masked) in H.DEGENERATE_CELLS
    for K, name, S in H.degenerate_cases(mode, dim, masked):
        Call(G, cap, S).check(K, H.DEGENERATE_RATIO, (cap.MEM_HOST, cap.MEM_DEVICE), name)


# ------------------------------------------------------------------------------------------------------------------- triangulation
@pytest.mark.parametrize("dim", H.DIMS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("grouped", [True, False])
def test_triangulation_cases(G, cap, dim, masked, grouped):
    """with camera groups (the speculative form) and without (k_greedy: one camera, one matrix); one shared block of essential matrices, and one per pair
    (pair 1: all zero — den == 0, nothing passes)"""
    S0 = H.tri_sets(dim, masked, grouped)
    E3 = H.tri_E(S0.nr_cams, np.random.default_rng(3), 3)
    for S in (S0, _withE(S0, E3)):
        call = Call(G, cap, S, groups=grouped)
        for K in (1, 4, 32):
            fb = call.check(K, 0.0, (cap.MEM_HOST, cap.MEM_DEVICE), "tri grouped %d nE %d" % (grouped, len(S.E)))
            if K == 1:
                assert fb[0] > 0, "34 failing candidates in front of the passing one: a one-entry list must be rescanned"


_withEs = {}


def _withE(S, E):
    if id(S) not in _withEs:
        _withEs[id(S)] = (S, H.with_E(S, E))
    return _withEs[id(S)][1]


# ------------------------------------------------------------------------------------------------------------------- chains
@pytest.mark.parametrize("K", H.CHAIN_KS)
@pytest.mark.parametrize("dim,masked", H.CHAIN_CELLS)
def test_chains_in_the_cells_the_chain_test_lacks(G, cap, K, dim, masked):
    for mode, ratios, S in H.chain_cases(dim, masked, K):
        call = Call(G, cap, S)
        for ratio in ratios:
            fb = call.check(K, ratio, (cap.MEM_HOST,), "chains")
        if K == 1 and mode == 1:
            assert fb.sum() > 0, "K = 1 on clustered data must force exact rescans"


# ------------------------------------------------------------------------------------------------------------------- above the claim table
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("nt", [16384, 16385])
def test_k_greedy_above_the_claim_table(G, cap, mode, nt):
    S = H.claim_sets(mode, nt)
    call = Call(G, cap, S)
    for K in (1, 8):
        for ratio in (0.9, 1.0):
            call.check(K, ratio, (cap.MEM_HOST, cap.MEM_DEVICE), "nt %d" % nt)


# ------------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("how", H.LAYOUTS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_row_layouts(G, cap, mode, how):
    """stride > dim with 0xA5 in the gap, descriptor | mask interleaved in one row, block-structured sets with bait rows between the blocks and behind the last
    one (H.bait_for: read as a train row, a bait row matches a query that has no match)"""
    for dim, masked in H.LAYOUT_CELLS:
        if how == "inter" and not masked:
            continue
        call = Call(G, cap, H.layout_case(mode, dim, masked), how)
        for ratio in H.LAYOUT_RATIOS[mode]:
            for K in (2, 8):
                call.check(K, ratio, (cap.MEM_HOST, cap.MEM_DEVICE), how)


# ------------------------------------------------------------------------------------------------------------------- ring
@pytest.mark.parametrize("dim,masked", H.RING_CELLS)
def test_ring_form_wraps_to_the_last_frame(G, cap, dim, masked):
    """mcs_search_kf_kf_ring: frame f against frame f - 1 of a ring of 5; pair 0 of (first 0, count 5) reads the LAST frame.  Against per-pair oracle calls
    (H.ring_sets: the pairs as one batched Sets, the same the CPU test holds against the definition)"""
    d, m, v, n, pitch = H.ring_frames(dim, masked)
    nf = len(d)
    lib, ctx = G.mcs.lib(), G.ctx()
    bd, bm, bv = G.DevBuf(d), G.DevBuf(m), G.DevBuf(v)
    fr = cap.DescSet(bd.ptr.value, bm.ptr.value if masked else None, bv.ptr.value, None, n, dim, 0, 0)
    for first, count in H.RING_RANGES:
        en, em = expected(G, H.ring_sets(dim, masked, first, count), H.RING_RATIO)
        assert (en > 0).all()
        for K in (1, 4):
            o_m, o_n, o_f = G.DevBuf(np.full((count, n), -7, np.int32)), G.DevBuf(np.full(count, -7, np.int32)), G.DevBuf(np.zeros(count, np.int32))
            cap.check(lib.mcs_search_kf_kf_ring(ctx.h, nf, first, count, C.byref(fr), pitch, dim, H.RING_RATIO, K, cap.MEM_DEVICE, o_m.ptr, o_n.ptr, o_f.ptr))
            ctx.synchronize()
            assert G.first_diff(o_n.read(), en) is None and G.first_diff(o_m.read(), em) is None, (first, count, K, G.first_diff(o_n.read(), en), G.first_diff(o_m.read(), em))


# ------------------------------------------------------------------------------------------------------------------- the other code paths
def test_other_code_paths_agree_on_the_tables():
    """the table tests again, each time in a fresh process under one switch: the VALU lists for every shape; the chunked form where the fixpoint form would run;
    the fixpoint given up after one sweep (resolved in order by exact rescans: the child asserts that the rescan counter of every such set pair reports every
    query, SWEEPS_1 above); the page-locked outputs of the host-kind calls filled by the runtime's copies instead of the output kernel.  One child after the
    other; a child that dies on a signal or runs into its time limit ends the test at once — nothing more is started on the device"""
    for switch in ({"MCS_MATCH_VALU": "1"}, {"MCS_GREEDY_JACOBI": "0"}, {"MCS_JACOBI_MAX_SWEEPS": "1"}, {"MCS_OUT_KERNEL": "0"}):
        e = dict(os.environ, **switch)
        try:
            r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_gpu_hostile_match.py"), "-m", "gpu", "-q", "-x", "-k", "test_table_layout"],
                               env=e, capture_output=True, text=True, timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired as x:
            pytest.fail("%s: the child ran into its time limit\n%s" % (switch, str(x.stdout)[-1500:]), pytrace=False)
        if r.returncode < 0 or r.returncode > 128:
            pytest.fail("%s: the child died (status %d)\n%s" % (switch, r.returncode, r.stdout[-1500:] + r.stderr[-800:]), pytrace=False)
        assert r.returncode == 0, (switch, r.stdout[-2500:] + r.stderr[-800:])
