"""Hostile descriptor sets for the search stage (top-K Hamming lists + the greedy resolution of SearchByBoW(KF,KF), SearchByBoW(KF,F) and
SearchForTriangulationRaw): seeded numpy generators, an independent definition of the three searches, and the case table that
tests/test_oracle_hostile_match_cpu.py (oracle == definition, and the conditions that keep a case from passing vacuously) and
tests/test_gpu_hostile_match.py (device == oracle, bit for bit) both walk.  Plain module: numpy only, nothing of the device; the oracle library is
only ever passed in by the caller (oracle_search), the definition does not touch it.

How a row at a PRESCRIBED distance is made.  The bits of a row are split (by a seeded permutation, so that every 32-bit word holds some of each) into
  payload A   TH_LOW + 3 bits covered by both masks: a row "at a" has the first a of them flipped against its block's base row
  odd bit     (masked) one bit covered by the query's mask only: flipped, it adds ONE to the raw popcount total, which the masked distance halves once
  dead bits   (masked) eight bits no mask covers, random in every row: they must not count
  tag         the rest: one code word per block (layout b), equal for a block's queries and rows — rows of different blocks are at least the code's
              minimum distance apart, whatever their payload says
so the raw total of (query at 0, row at (a, b)) is a unmasked and 2a + b masked, distance a either way.

A BLOCK is a handful of queries and the rows meant for them; a case is a list of blocks, laid out either as
  (a) many tiny set pairs, one per block, batched with a set pitch (blocks of one call have the same nq and nt), or
  (b) set pairs that hold many blocks each, kept apart by the tag.  Plotkin's bound caps a code whose distance nears half its length at a few dozen words:
      unmasked TH_LOW is a quarter of the row, so the unmasked tables need several set pairs (they go into one call); min_cross() is what the tests check."""
import numpy as np

SEED = 20
DIMS = (16, 32, 64)
RATIOS = (0.1, 0.25, 0.5, 0.6, 0.7, 0.75, 0.8, 0.9, 1.0, 1.25)
KS = (1, 2, 8, 16, 32)
INT_MAX = 0x7FFFFFFF
CELLS = [(mode, dim, masked) for mode in (0, 1) for dim in DIMS for masked in (False, True)]
# layout (b): blocks per set pair, and the ratio whose list cap the tag code must exceed (see the module text)
CHUNK = {(16, False): 64, (32, False): 256, (64, False): 1024, (16, True): 256, (32, True): 1024, (64, True): 1024}
TAG_RATIO = {False: 0.9, True: 0.5}


def th_low(dim, masked):
    """TH_LOW_ of cORBmatcher::cORBmatcher (src/cORBmatcher.cpp:46-65)"""
    return dim if masked else 2 * dim


def list_cap(dim, masked, ratio):
    """the farthest row that can still change a SearchByBoW decision: best <= TH_LOW, and a second d decides the ratio test only while ratio * d <= TH_LOW"""
    th = th_low(dim, masked)
    return max([th] + [m for m in range(th, 8 * dim + 1) if ratio * float(m) <= float(th)])


# ------------------------------------------------------------------------------------------------------------------- the independent definition
def raw_totals(dq, mq, dt, mt):
    """[nq, nt] popcount totals from np.unpackbits: |q ^ t| unmasked, |(q ^ t) & mq| + |(q ^ t) & mt| masked (NOT yet halved)"""
    nq, nt = len(dq), len(dt)
    if nq == 0 or nt == 0:
        return np.zeros((nq, nt), np.int64)
    Q, T = np.unpackbits(dq, axis=1).astype(np.float32), np.unpackbits(dt, axis=1).astype(np.float32)
    if mq is None:
        return np.rint(Q @ (1 - T).T + (1 - Q) @ T.T).astype(np.int64)
    MQ, MT = np.unpackbits(mq, axis=1).astype(np.float32), np.unpackbits(mt, axis=1).astype(np.float32)
    return np.rint((MQ * Q) @ (1 - T).T + (MQ * (1 - Q)) @ T.T + Q @ (MT * (1 - T)).T + (1 - Q) @ (MT * T).T).astype(np.int64)   # (sums < 2^24: exact in float32)


def distances(dq, mq, dt, mt):
    """DescriptorDistance64 / DescriptorDistance64Masked (:2438-2474): the masked sum over the whole row is halved ONCE"""
    r = raw_totals(dq, mq, dt, mt)
    return r if mq is None else r // 2


def define_bow(mode, D, vq, vt, th, ratio, book=None):
    """SearchByBoW(KF,KF) (mode 0, :885-966) / SearchByBoW(KF,F) without the vocabulary restriction (mode 1, :179-323) as the sequential loop they are.
    D = distance matrix as nested lists.  -> (nmatches, match12[nq] | matchF[nt]); book collects (query, best, second, accepted)"""
    nq, nt = len(vq), len(vt)
    taken = [False] * nt
    out = [-1] * (nt if mode == 1 else nq)
    n = 0
    big = isinstance(D, np.ndarray)   # long rows: the same scan (first smallest, then the smallest of the rest) through numpy
    if big:
        free = np.array(vt, bool)
    for i in range(nq):
        if not vq[i]:
            continue
        best, besti, second = INT_MAX, -1, INT_MAX
        if big:
            d = np.where(free, D[i], INT_MAX)
            if nt and d.min() < INT_MAX:
                besti = int(d.argmin())          # the lowest index among equals, as the strict `<` of the loop below
                best = int(d[besti])
                d[besti] = INT_MAX
                second = int(d.min())
        else:
            row = D[i]
            for j in range(nt):
                if taken[j] or not vt[j]:
                    continue
                d = row[j]
                if d < best:
                    second, best, besti = best, d, j
                elif d < second:
                    second = d
        ok = (best <= th if mode == 1 else best < th) and float(best) < ratio * float(second)
        if book is not None:
            book.append((i, best, second, ok))
        if ok:
            taken[besti] = True
            if big:
                free[besti] = False
            if mode == 1:
                out[besti] = i
            else:
                out[i] = besti
            n += 1
    return n, out


def epipolar(r1, r2, E, thresh=1e-2):
    """CheckDistEpipolarLine (misc.cpp:53-69) -> (verdict, dsqr or None where den == 0)"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    nom = float(r2 @ E @ r1)
    a, b = E @ r1, E.T @ r2
    den = float(a @ a + b @ b)
    if den == 0.0:
        return False, None
    dsqr = nom * nom / den
    return dsqr < thresh, dsqr


def define_tri(D, mp1, cam1, rays1, mp2, cam2, rays2, E, nr_cams, th, book=None):
    """SearchForTriangulationRaw (:968-1155, mbCheckOrientation off): candidates of the same camera within TH_LOW sorted by (distance, index), DistTh = 2 * BestDist,
    the first one that passes the epipolar test wins"""
    n1, n2 = len(mp1), len(mp2)
    taken = [False] * n2
    out = [-1] * n1
    n = 0
    for i in range(n1):
        if mp1[i]:
            continue
        cand = sorted((D[i][j], j) for j in range(n2) if not taken[j] and not mp2[j] and cam1[i] == cam2[j] and D[i][j] <= th)
        if not cand:
            continue
        dist_th = 2 * cand[0][0]
        tested = 0
        for d, j in cand:
            if d > dist_th:
                break
            tested += 1
            ok, dsqr = epipolar(rays1[i], rays2[j], E[cam1[i] * nr_cams + cam2[j]])
            if book is not None:
                book.append((i, j, d, cand[0][0], dsqr))
            if ok:
                taken[j] = True
                out[i] = j
                n += 1
                break
    return n, out


# ------------------------------------------------------------------------------------------------------------------- sets
class Sets:
    """the arrays of one call: nsets (query set, train set) pairs of nq / nt rows.  dq [nsets, nq, dim] ... ; valid 1 = takes part (mode 2: has NO map point);
    triangulation adds cam [nsets, n] int32, rays [nsets, n, 3], E [nE, nc * nc, 9] (nE = 1: shared by all pairs) and nr_cams"""

    def __init__(self, mode, dim, masked, dq, mq, vq, dt, mt, vt, camq=None, camt=None, raysq=None, rayst=None, E=None, nr_cams=0, meta=None):
        self.mode, self.dim, self.masked = mode, dim, masked
        self.dq, self.mq, self.vq, self.dt, self.mt, self.vt = dq, mq, vq, dt, mt, vt
        self.camq, self.camt, self.raysq, self.rayst, self.E, self.nr_cams = camq, camt, raysq, rayst, E, nr_cams
        self.nsets, self.nq, self.nt = dq.shape[0], dq.shape[1], dt.shape[1]
        self.meta = meta or {}

    def E_of(self, s):
        return self.E[s if len(self.E) > 1 else 0]


def define_search(S, ratio=0.0, book=None, keep=None):
    """the definition on every set pair of S -> (nmatches [nsets], match [nsets, nq | nt]); book entries get the set index in front; keep: a dict of the caller's
    that holds the distance matrices from one ratio to the next"""
    th = th_low(S.dim, S.masked)
    nm = np.zeros(S.nsets, np.int32)
    out = np.full((S.nsets, S.nt if S.mode == 1 else S.nq), -1, np.int32)
    for s in range(S.nsets):
        if keep is not None and s in keep:
            D = keep[s]
        else:
            D = distances(S.dq[s], S.mq[s] if S.masked else None, S.dt[s], S.mt[s] if S.masked else None).astype(np.int32)
            if keep is not None:
                keep[s] = D
        b = None if book is None else []
        if S.mode == 2:
            nm[s], o = define_tri(D.tolist(), (1 - S.vq[s]).tolist(), S.camq[s].tolist(), S.raysq[s], (1 - S.vt[s]).tolist(), S.camt[s].tolist(), S.rayst[s],
                                  S.E_of(s), S.nr_cams, th, b)
        else:
            nm[s], o = define_bow(S.mode, D if S.nt > 8 else D.tolist(), S.vq[s].tolist(), S.vt[s].tolist(), th, ratio, b)
        out[s] = o
        if book is not None:
            book.extend((s,) + e for e in b)
    return nm, out


def tiny_totals(S):
    """[nsets, nq, nt] raw popcount totals of layout (a), all pairs in one go (kept with S)"""
    if "raw" not in S.meta:
        x = S.dq[:, :, None, :] ^ S.dt[:, None, :, :]
        if S.masked:
            S.meta["raw"] = (np.unpackbits(x & S.mq[:, :, None, :], axis=3).sum(axis=3, dtype=np.int64) +
                             np.unpackbits(x & S.mt[:, None, :, :], axis=3).sum(axis=3, dtype=np.int64))
        else:
            S.meta["raw"] = np.unpackbits(x, axis=3).sum(axis=3, dtype=np.int64)
    return S.meta["raw"]


def define_tiny(S, ratio, book=None):
    """define_search for layout (a), thousands of tiny set pairs: the distances of all pairs in one go, the loops per pair as above"""
    th = th_low(S.dim, S.masked)
    D = (tiny_totals(S) // 2 if S.masked else tiny_totals(S)).tolist()
    vq, vt = S.vq.tolist(), S.vt.tolist()
    nm = np.zeros(S.nsets, np.int32)
    out = []
    for s in range(S.nsets):
        b = None if book is None else []
        nm[s], o = define_bow(S.mode, D[s], vq[s], vt[s], th, ratio, b)
        out.append(o)
        if book is not None:
            book.extend((s,) + e for e in b)
    return nm, np.array(out, np.int32).reshape(S.nsets, S.nt if S.mode == 1 else S.nq)


def oracle_search(O, S, ratio=0.0):
    """the oracle on every set pair of S -> (nmatches [nsets], match [nsets, nq | nt]).  SearchByBoW(KF,F) has no flags on the frame side: invalid frame rows
    are padding, the oracle sees the frame without them"""
    L = O.lib()
    dim, nq, nt = S.dim, S.nq, S.nt
    nm = np.zeros(S.nsets, np.int32)
    out = np.full((S.nsets, nt if S.mode == 1 else nq), -1, np.int32)
    ones = np.full((max(nq, nt, 1), dim), 255, np.uint8)
    C = [np.ascontiguousarray(a) for a in (S.dq, S.mq if S.masked else S.dq, S.vq, S.dt, S.mt if S.masked else S.dt, S.vt)]
    adr = [a.ctypes.data for a in C]
    o_adr, a1 = out.ctypes.data, ones.ctypes.data
    if S.mode == 0 or (S.mode == 1 and nt > 0 and S.vt.all()):
        for s in range(S.nsets):
            q, t = s * nq * dim, s * nt * dim
            mq_, mt_ = (adr[1] + q, adr[4] + t) if S.masked else (a1, a1)
            if S.mode == 0:
                nm[s] = L.orc_search_kf_kf(adr[0] + q, mq_, adr[2] + s * nq, nq, adr[3] + t, mt_, adr[5] + s * nt, nt, dim, int(S.masked), ratio, o_adr + s * nq * 4)
            else:
                nm[s] = L.orc_search_kf_f(adr[0] + q, mq_, adr[2] + s * nq, nq, adr[3] + t, mt_, nt, dim, int(S.masked), ratio, o_adr + s * nt * 4)
        return nm, out
    for s in range(S.nsets):
        mq = C[1][s] if S.masked else ones[:nq]
        if S.mode == 1:
            keep = np.flatnonzero(S.vt[s])
            mt = np.ascontiguousarray(C[4][s][keep]) if S.masked else np.ascontiguousarray(ones[:len(keep)])
            nm[s], m = O.search_kf_f(C[0][s], mq, C[2][s], np.ascontiguousarray(C[3][s][keep]).reshape(len(keep), dim), mt, S.masked, ratio)
            out[s, keep] = m
        else:
            mt = C[4][s] if S.masked else ones[:nt]
            nc = S.nr_cams
            nm[s], out[s] = O.search_triangulation(C[0][s], mq, np.ascontiguousarray(1 - S.vq[s]).astype(np.uint8), np.ascontiguousarray(S.camq[s], np.int32),
                                                   np.ascontiguousarray(S.raysq[s]), C[3][s], mt, np.ascontiguousarray(1 - S.vt[s]).astype(np.uint8),
                                                   np.ascontiguousarray(S.camt[s], np.int32), np.ascontiguousarray(S.rayst[s]),
                                                   np.ascontiguousarray(S.E_of(s)).reshape(nc * nc, 9), nc, S.masked)
    return nm, out


# ------------------------------------------------------------------------------------------------------------------- exact-distance builder
class Regions:
    """the split of a row's bits (module text); seeded per (dim, masked)"""

    def __init__(self, dim, masked, seed=SEED):
        self.dim, self.masked, self.bits = dim, masked, 8 * dim
        rng = np.random.default_rng([seed, dim, int(masked)])
        perm = rng.permutation(self.bits)
        nA = th_low(dim, masked) + 3
        self.A = perm[:nA]
        self.odd = perm[nA:nA + 1] if masked else perm[:0]
        self.dead = perm[nA + 1:nA + 9] if masked else perm[:0]
        self.tag = perm[nA + (9 if masked else 0):]

    def row(self, base_bits, a, b=0):
        """base row with `a` payload bits (and the odd bit if b) flipped -> bit array"""
        assert 0 <= a <= len(self.A) and (b == 0 or self.masked)
        r = base_bits.copy()
        r[self.A[:a]] ^= 1
        if b:
            r[self.odd] ^= 1
        return r

    def masks(self):
        """(query mask bits, train mask bits): the odd bit is covered by the query's mask only, the dead bits by none"""
        mq = np.ones(self.bits, np.uint8)
        mq[self.dead] = 0
        mt = mq.copy()
        mt[self.odd] = 0
        return mq, mt


def tag_code(nbits, count, dmin, rng):
    """`count` words of nbits with pairwise distance >= dmin: random words, kept greedily"""
    kept = np.zeros((0, nbits), np.float32)
    for _ in range(4000):
        cand = (rng.random((256, nbits)) < 0.5).astype(np.float32)
        far = (kept @ (1 - cand).T + (1 - kept) @ cand.T).min(axis=0) >= dmin if len(kept) else np.ones(256, bool)
        dc = cand @ (1 - cand).T + (1 - cand) @ cand.T
        add = []
        for c in np.flatnonzero(far):
            if all(dc[c, c2] >= dmin for c2 in add):
                add.append(c)
        kept = np.concatenate([kept, cand[add]])[:count]
        if len(kept) >= count:
            return kept.astype(np.uint8)
    raise RuntimeError("no code of %d words, %d bits, distance %d" % (count, nbits, dmin))


# ------------------------------------------------------------------------------------------------------------------- blocks -> sets
def _rows_of(blocks, side):
    """(block index, a, b[, flag]) of every row of one side, in block order"""
    blk, a, b, f = [], [], [], []
    for i, bl in enumerate(blocks):
        for r in bl[side]:
            blk.append(i); a.append(r[0]); b.append(r[1]); f.append(r[2] if len(r) > 2 else 1)
    return np.array(blk, np.int64), np.array(a, np.int64), np.array(b, np.int64), np.array(f, np.int64)


def _build_rows(R, base_bits, blk, a, b, rng):
    """packed rows: base row of the row's block with a payload bits / the odd bit flipped, dead bits random"""
    bits = base_bits[blk].copy() if len(blk) else np.zeros((0, R.bits), np.uint8)
    if len(blk):
        sub = bits[:, R.A]
        sub ^= (np.arange(len(R.A))[None, :] < a[:, None]).astype(np.uint8)
        bits[:, R.A] = sub
        if R.masked:
            bits[:, R.odd] ^= b[:, None].astype(np.uint8)
            bits[:, R.dead] = rng.integers(0, 2, (len(blk), len(R.dead)), dtype=np.uint8)
    return np.packbits(bits, axis=1).reshape(len(blk), R.dim)


def assemble_tiny(mode, dim, masked, blocks, seed=SEED):
    """layout (a): one set pair per block; all blocks must have the same number of queries and of rows"""
    R = Regions(dim, masked)
    rng = np.random.default_rng([seed, 1, mode, dim, int(masked), len(blocks)])
    nq, nt, n = len(blocks[0]["q"]), len(blocks[0]["t"]), len(blocks)
    assert all(len(b["q"]) == nq and len(b["t"]) == nt for b in blocks)
    base = rng.integers(0, 2, (n, R.bits), dtype=np.uint8)
    qb, qa, qo, _ = _rows_of(blocks, "q")
    tb, ta, to, _ = _rows_of(blocks, "t")
    dq = _build_rows(R, base, qb, qa, qo, rng).reshape(n, nq, dim)
    dt = _build_rows(R, base, tb, ta, to, rng).reshape(n, nt, dim)
    mqb, mtb = R.masks()
    mq = np.broadcast_to(np.packbits(mqb), (n, nq, dim)).copy() if masked else None
    mt = np.broadcast_to(np.packbits(mtb), (n, nt, dim)).copy() if masked else None
    return Sets(mode, dim, masked, dq, mq, np.ones((n, nq), np.uint8), dt, mt, np.ones((n, nt), np.uint8), meta={"layout": "a"})


def tag_dmin(dim, masked):
    """what the tag code of layout (b) is built for: beyond the largest row of the tables (TH_LOW + 3) and the list cap of TAG_RATIO"""
    return max(th_low(dim, masked) + 3, list_cap(dim, masked, TAG_RATIO[masked])) + 1


def assemble_tagged(mode, dim, masked, blocks, chunk=None, seed=SEED, tri=None):
    """layout (b): `chunk` blocks per set pair, every block under its own tag word; short sets are padded with invalid rows.  meta: qblk / tblk = the global
    block index of every row (-1 padding).  tri = (nr_cams,): rows carry (a, b, passes the epipolar test), cameras and rays are added (see tri_geometry)"""
    R = Regions(dim, masked)
    chunk = chunk or CHUNK[(dim, masked)]
    rng = np.random.default_rng([seed, 2, mode, dim, int(masked), len(blocks)])
    code = tag_code(len(R.tag), min(chunk, len(blocks)), tag_dmin(dim, masked), np.random.default_rng([seed, 3, dim, int(masked)]))
    nsets = (len(blocks) + chunk - 1) // chunk
    base = rng.integers(0, 2, (len(blocks), R.bits), dtype=np.uint8)
    base[:, R.tag] = code[np.arange(len(blocks)) % chunk]
    qb, qa, qo, _ = _rows_of(blocks, "q")
    tb, ta, to, tf = _rows_of(blocks, "t")
    rq, rt = _build_rows(R, base, qb, qa, qo, rng), _build_rows(R, base, tb, ta, to, rng)
    nq = max(int(np.bincount(qb // chunk, minlength=nsets).max()), 1)
    nt = max(int(np.bincount(tb // chunk, minlength=nsets).max()), 1) if len(tb) else 1
    dq, dt = rng.integers(0, 256, (nsets, nq, dim), dtype=np.uint8), rng.integers(0, 256, (nsets, nt, dim), dtype=np.uint8)
    vq, vt = np.zeros((nsets, nq), np.uint8), np.zeros((nsets, nt), np.uint8)
    qblk, tblk = np.full((nsets, nq), -1, np.int64), np.full((nsets, nt), -1, np.int64)
    tflag = np.ones((nsets, nt), np.int64)
    for s in range(nsets):
        iq, it = np.flatnonzero(qb // chunk == s), np.flatnonzero(tb // chunk == s)
        dq[s, :len(iq)], vq[s, :len(iq)], qblk[s, :len(iq)] = rq[iq], 1, qb[iq]
        dt[s, :len(it)], vt[s, :len(it)], tblk[s, :len(it)], tflag[s, :len(it)] = rt[it], 1, tb[it], tf[it]
    mqb, mtb = R.masks()
    mq = np.broadcast_to(np.packbits(mqb), (nsets, nq, dim)).copy() if masked else None
    mt = np.broadcast_to(np.packbits(mtb), (nsets, nt, dim)).copy() if masked else None
    S = Sets(mode, dim, masked, dq, mq, vq, dt, mt, vt, meta={"layout": "b", "qblk": qblk, "tblk": tblk, "chunk": chunk})
    if tri is not None:
        tri_geometry(S, tflag, tri[0], rng)
    return S


def min_cross(S):
    """layout (b): the smallest distance between a query and a row of ANOTHER block of its set pair (what keeps foreign rows out of every decision)"""
    lo = INT_MAX
    for s in range(S.nsets):
        D = distances(S.dq[s], S.mq[s] if S.masked else None, S.dt[s], S.mt[s] if S.masked else None)
        qb, tb = S.meta["qblk"][s], S.meta["tblk"][s]
        other = (qb[:, None] != tb[None, :]) & (qb[:, None] >= 0) & (tb[None, :] >= 0)
        if other.any():
            lo = min(lo, int(D[other].min()))
    return lo


def ratios_b(dim, masked):
    """the ratios layout (b) runs with: those whose list cap stays below what the tag code guarantees"""
    return [r for r in RATIOS if list_cap(dim, masked, r) < tag_dmin(dim, masked)]


# ------------------------------------------------------------------------------------------------------------------- the decision table
def decision_blocks(dim, masked):
    """one query per (best, second), 0 <= best <= second <= TH_LOW + 2; masked: also with the odd totals 2 best + 1 / 2 second + 1; the best row comes first or
    second in index order; the same pairs with a third row that ties the second; lone rows; no row at all"""
    th = th_low(dim, masked)
    par = ((0, 0), (1, 0), (0, 1), (1, 1)) if masked else ((0, 0),)
    blocks = []
    for best in range(th + 3):
        for second in range(best, th + 3):
            for pb, ps in par:
                rows = [(best, pb), (second, ps)]
                blocks.append({"q": [(0, 0)], "t": rows[::-1] if (best + second) & 1 else rows})
            blocks.append({"q": [(0, 0)], "t": [(second, 0), (best, 0), (second, 0)]})
        for pb in ((0, 1) if masked else (0,)):
            blocks.append({"q": [(0, 0)], "t": [(best, pb)]})
    blocks.append({"q": [(0, 0)], "t": []})
    return blocks


def contention_blocks(dim, masked):
    """the same (best, second) pairs with TWO equal queries: the lower one looks at (best, second), and where it takes the best row the upper one is left with
    (second, third = second + 1).  With K = 1 or 2 the upper query's list holds nothing free: exact rescans"""
    th = th_low(dim, masked)
    blocks = []
    for best in range(th + 3):
        for second in range(best, th + 3):
            for ps in ((0, 1) if masked else (0,)):
                blocks.append({"q": [(0, 0), (0, 0)], "t": [(best, 0), (second, ps), (second + 1, 0)]})
    return blocks


def by_shape(blocks):
    """blocks grouped by (number of queries, number of rows): the calls of layout (a)"""
    groups = {}
    for b in blocks:
        groups.setdefault((len(b["q"]), len(b["t"])), []).append(b)
    return groups


_cache = {}


def table(mode, dim, masked, layout, kind="decision"):
    """-> list of Sets (cached, read-only): layout 'a': one per block shape; 'b': one, with CHUNK blocks per set pair"""
    key = (mode, dim, masked, layout, kind)
    if key not in _cache:
        blocks = decision_blocks(dim, masked) if kind == "decision" else contention_blocks(dim, masked)
        if layout == "a":
            _cache[key] = [assemble_tiny(mode, dim, masked, g) for _, g in sorted(by_shape(blocks).items())]
        else:
            _cache[key] = [assemble_tagged(mode, dim, masked, blocks)]
        for S in _cache[key]:
            S.meta["nblocks"] = len(blocks)
    return _cache[key]


def classify(S, ratio, book, counts):
    """the non-vacuity classes of one definition run (book of define_bow) into counts"""
    th, cap = th_low(S.dim, S.masked), list_cap(S.dim, S.masked, ratio)

    def add(k):
        counts[k] = counts.get(k, 0) + 1
    for s, i, best, second, ok in book:
        if best == INT_MAX:
            continue
        if float(best) < ratio * float(second):      # the threshold alone decides
            if best == th - 1 and ok:
                add("accept@TH-1")
            if best == th:
                add("accept@TH" if ok else "reject@TH")
            if best == th + 1 and not ok:
                add("reject@TH+1")
            if ok and second == INT_MAX:
                add("lone-accept")
        if second < INT_MAX and float(best) == ratio * float(second) and (best <= th if S.mode == 1 else best < th):
            add("ratio-equal@%g" % ratio)
    if S.masked and cap <= th + 1:   # (the rows of the table end at TH_LOW + 2: ratios 1.0 and 1.25 for every dim, 0.9 for 16-byte rows)
        # odd totals (halved once: 2 d + 1 -> d), counted from DECISIONS: the best row carries the odd total and sits at the last accepted / first rejected
        # distance; the second row is the only row at the list cap (total 2 cap + 1: in) or right behind it (2 cap + 2 and 2 cap + 3: out)
        tot = tiny_totals(S)
        lim = th - (0 if S.mode == 1 else 1)
        for s, i, best, second, ok in book:
            if best == INT_MAX or not best < second:
                continue
            t = tot[s, i]
            if float(best) < ratio * float(second):
                if ok and best == lim and (t == 2 * lim + 1).any():
                    add("odd-within-TH@%g" % ratio)
                if not ok and best == lim + 1 and (t == 2 * lim + 3).any():
                    add("odd-beyond-TH@%g" % ratio)
            for name, d, total in (("odd-within-cap", cap, 2 * cap + 1), ("even-beyond-cap", cap + 1, 2 * cap + 2), ("odd-beyond-cap", cap + 1, 2 * cap + 3)):
                if second == d and (t // 2 == d).sum() == 1 and (t == total).any():
                    add("%s@%g" % (name, ratio))
    return counts


# ------------------------------------------------------------------------------------------------------------------- triangulation
def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


def tri_E(nr_cams, rng, nE=1):
    """[nE, nc * nc, 9]: the same-camera blocks are translation skews (the only ones the search reads), the others noise; pair 1 of a per-pair array is ALL ZERO
    (den == 0: nothing passes), the further pairs are multiples of pair 0 (dsqr is scale-free)"""
    E = rng.normal(size=(nE, nr_cams, nr_cams, 3, 3))
    for k in range(nE):
        for c in range(nr_cams):
            E[k, c, c] = _skew(tri_t(c)) * (1.0 + 1.5 * k)
    if nE > 1:
        E[1] = 0.0
    return E.reshape(nE, nr_cams * nr_cams, 9)


def tri_t(c):
    return np.array([0.05, 0.01 * (c + 1), 0.002 * (c + 1)])


def tri_geometry(S, tflag, nr_cams, rng):
    """cameras (block index mod nr_cams), rays and E for a tagged Sets: a row flagged 1 lies in the epipolar plane of its block's query (ray2 = unit(ray1 + 0.3 t^):
    dsqr ~ 1e-33), a row flagged 0 along t x ray1 (dsqr ~ 0.5): both far from the 1e-2 bound"""
    qb, tb = S.meta["qblk"], S.meta["tblk"]
    S.nr_cams = nr_cams
    S.camq, S.camt = (np.maximum(qb, 0) % nr_cams).astype(np.int32), (np.maximum(tb, 0) % nr_cams).astype(np.int32)
    nblk = int(max(qb.max(), tb.max())) + 1
    r1 = _unit(rng.normal(size=(nblk, 3)) * [0.5, 0.5, 0.2] + [0, 0, 1.0])
    S.raysq = r1[np.maximum(qb, 0)]
    that = np.stack([_unit(tri_t(c)) for c in range(nr_cams)])[S.camt]
    base = r1[np.maximum(tb, 0)]
    S.rayst = np.where(tflag[..., None] != 0, _unit(base + 0.3 * that), _unit(np.cross(that, base)))
    S.E = tri_E(nr_cams, rng, 1)
    S.mode = 2


def tri_blocks(dim, masked):
    """rows are (a, b, passes): see the issue's list — BestDist = 0, 2 BestDist / + 1, TH_LOW / + 1, long runs of failing candidates, a best row taken by a lower query"""
    th = th_low(dim, masked)
    odd = 1 if masked else 0
    B = []
    q = [(0, 0)]
    B.append({"q": q, "t": [(0, 0, 0), (0, 0, 1), (1, 0, 1)]})          # BestDist 0: the second row at 0 wins
    B.append({"q": q, "t": [(0, odd, 0), (1, 0, 1)]})                    # BestDist 0, DistTh 0: the row at 1 is out of reach
    B.append({"q": q, "t": [(1, 0, 1), (0, 0, 0)]})                      # the same, index order reversed
    for b in (1, 3, th // 2):
        B.append({"q": q, "t": [(b, 0, 0), (2 * b, odd, 1)]})            # exactly 2 BestDist: taken
        if 2 * b + 1 <= th + 2:
            B.append({"q": q, "t": [(b, odd, 0), (2 * b + 1, 0, 1)]})    # 2 BestDist + 1: not
    B.append({"q": q, "t": [(th, odd, 1)]})                              # at TH_LOW: a candidate
    B.append({"q": q, "t": [(th + 1, 0, 1)]})                            # beyond: none
    B.append({"q": q, "t": [(th // 2, 0, 0), (th + 1, 0, 1), (th, 0, 1)]})
    for b in (0, 2):
        B.append({"q": q, "t": [(b, 0, 0)] * 34 + [(b, 0, 1)]})          # more failing candidates within DistTh than any list holds, then one that passes
        B.append({"q": q, "t": [(b, 0, 0)] * 34})                        # ... then none
        B.append({"q": q, "t": [(b, 0, 0)] * 20 + [(2 * b, 0, 0)] * 14 + [(2 * b + 1, 0, 1)]})
    B.append({"q": [(0, 0), (0, 0)], "t": [(2, 0, 1), (5, odd, 1)]})     # the best row goes to the lower query: the upper one's BestDist is 5, not 2
    B.append({"q": [(0, 0), (0, 0), (0, 0)], "t": [(1, 0, 1), (1, 0, 0), (3, 0, 1)]})
    return B


def tri_sets(dim, masked, grouped=True, nr_cams=3):
    """the triangulation cases in one tagged set pair; grouped False: every camera index 0 and one essential matrix (the call without camera groups)"""
    key = ("tri", dim, masked, grouped, nr_cams)
    if key not in _cache:
        _cache[key] = assemble_tagged(2, dim, masked, tri_blocks(dim, masked), chunk=64, tri=(nr_cams if grouped else 1,))
    return _cache[key]


def with_E(S, E):
    """S (one set pair) repeated once per matrix block of E [nE, nc * nc, 9]"""
    n = len(E)
    rep = lambda a: None if a is None else np.repeat(a, n, axis=0)
    return Sets(2, S.dim, S.masked, rep(S.dq), rep(S.mq), rep(S.vq), rep(S.dt), rep(S.mt), rep(S.vt), rep(S.camq), rep(S.camt), rep(S.raysq), rep(S.rayst),
                E, S.nr_cams, dict(S.meta))


# ------------------------------------------------------------------------------------------------------------------- degenerate sets, chains
def _masks(rng, shape, masked, p=0.9):
    return np.packbits(rng.random(shape[:-1] + (shape[-1] * 8,)) < p, axis=-1) if masked else None


def add_tri(S, rng, nr_cams=3, train_cams=None):
    """rays / cameras / E for any Sets: every train ray passes or fails clearly against EVERY query ray of its camera — all query rays are one ray"""
    S.mode, S.nr_cams = 2, nr_cams
    r1 = _unit(np.array([0.2, -0.1, 1.0]))
    S.camq = rng.integers(0, nr_cams, (S.nsets, S.nq)).astype(np.int32)
    S.camt = rng.integers(0, train_cams or nr_cams, (S.nsets, S.nt)).astype(np.int32)
    S.raysq = np.broadcast_to(r1, (S.nsets, S.nq, 3)).copy()
    that = np.stack([_unit(tri_t(c)) for c in range(nr_cams)])[S.camt]
    S.rayst = np.where(rng.random((S.nsets, S.nt, 1)) < 0.7, _unit(r1 + 0.3 * that), _unit(np.cross(that, r1)))
    S.E = tri_E(nr_cams, rng, 1)
    return S


def clustered(rng, n, centres, flips):
    d = centres[rng.integers(0, len(centres), n)].copy()
    bits = centres.shape[1] * 8
    for i in range(n):
        for b in rng.integers(0, bits, flips):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def degenerate_sets(mode, dim, masked, K):
    """-> [(name, Sets)] for one mode (2: with rays and cameras)"""
    rng = np.random.default_rng([SEED, 5, mode, dim, int(masked), K])
    nq, nt = 40, 37
    out = []

    def mk(name, dq, dt, mq=None, mt=None, vq=None, vt=None, **tri):
        if masked:
            mq = _masks(rng, dq.shape, True) if mq is None else mq
            mt = _masks(rng, dt.shape, True) if mt is None else mt
        else:
            mq = mt = None
        S = Sets(mode, dim, masked, dq[None], None if mq is None else mq[None], (np.ones(len(dq), np.uint8) if vq is None else vq)[None],
                 dt[None], None if mt is None else mt[None], (np.ones(len(dt), np.uint8) if vt is None else vt)[None])
        if mode == 2:
            add_tri(S, rng, **tri)
        out.append((name, S))

    one = rng.integers(0, 256, (1, dim), dtype=np.uint8)
    onem = _masks(rng, (1, dim), masked)
    rep = lambda a, n: None if a is None else np.repeat(a, n, axis=0)
    mk("all-equal", rep(one, nq), rep(one, nt), rep(onem, nq), rep(onem, nt))
    rq, rt = rng.integers(0, 256, (nq, dim), dtype=np.uint8), rng.integers(0, 256, (nt, dim), dtype=np.uint8)
    if masked:
        mk("zero-masks", rq, rt, np.zeros_like(rq), np.zeros_like(rt))
    mk("ones-vs-zeros", np.full((nq, dim), 255, np.uint8), np.zeros((nt, dim), np.uint8), np.full((nq, dim), 255, np.uint8), np.full((nt, dim), 255, np.uint8))
    centres = rng.integers(0, 256, (3, dim), dtype=np.uint8)
    for n in sorted({1, max(K - 1, 1), K, K + 1}):
        mk("nt=%d" % n, clustered(rng, 20, centres, 2), clustered(rng, n, centres, 2))
    cq, ct = clustered(rng, nq, centres, 2), clustered(rng, nt, centres, 2)
    mk("queries-invalid", cq, ct, vq=np.zeros(nq, np.uint8))
    mk("train-invalid", cq, ct, vt=np.zeros(nt, np.uint8))
    if mode == 2:
        mk("camera-without-rows", cq, ct, train_cams=2)
        mk("one-camera", cq, ct, nr_cams=1)
    return out


def chain_sets(mode, dim, masked, seed):
    """the clustered sets of the chain test at the smallest useful size: near-duplicates on both sides, every outcome hangs on a chain of earlier ones"""
    rng = np.random.default_rng([SEED, 6, dim, int(masked), seed])
    nq, nt, ncl = 300, 280, 2 + seed % 5
    centres = rng.integers(0, 256, (ncl, dim), dtype=np.uint8)
    dq, dt = clustered(rng, nq, centres, 3), clustered(rng, nt, centres, 3)
    vq = (rng.random(nq) < 0.9).astype(np.uint8)
    vt = (rng.random(nt) < 0.9).astype(np.uint8) if mode == 0 else np.ones(nt, np.uint8)
    mq, mt = _masks(rng, dq.shape, masked), _masks(rng, dt.shape, masked)
    return Sets(mode, dim, masked, dq[None], None if mq is None else mq[None], vq[None], dt[None], None if mt is None else mt[None], vt[None])


def claim_sets(mode, nt, dim=32):
    """40 clustered queries against nt clustered rows (the speculative form's claim table ends at 16384 rows)"""
    rng = np.random.default_rng([SEED, 7, mode])       # (the same rows for every nt: 16384 is 16385 without its last row)
    centres = rng.integers(0, 256, (8, dim), dtype=np.uint8)
    dq = clustered(rng, 40, centres, 3)
    pick = rng.integers(0, 8, 16385)
    noise = np.packbits(rng.random((16385, dim * 8)) < 3.0 / (dim * 8), axis=1)
    dt = (centres[pick] ^ noise)[:nt]
    return Sets(mode, dim, False, dq[None], None, np.ones((1, 40), np.uint8), np.ascontiguousarray(dt)[None], None, np.ones((1, nt), np.uint8))


# ------------------------------------------------------------------------------------------------------------------- layouts
LAYOUTS = ("stride4", "stride16", "inter", "blocks")


def pad_rows(S, mult):
    """S with both sides padded by invalid rows to a multiple of `mult` (indices of the real rows unchanged)"""
    def pad(a, n, fill):
        if a is None:
            return None
        extra = (-n) % mult
        return np.concatenate([a, np.full((a.shape[0], extra) + a.shape[2:], fill, a.dtype)], axis=1)
    P = Sets(S.mode, S.dim, S.masked, pad(S.dq, S.nq, 0x5A), pad(S.mq, S.nq, 0xFF), pad(S.vq, S.nq, 0), pad(S.dt, S.nt, 0x5A), pad(S.mt, S.nt, 0xFF), pad(S.vt, S.nt, 0),
             pad(S.camq, S.nq, 0), pad(S.camt, S.nt, 0), pad(S.raysq, S.nq, 1.0), pad(S.rayst, S.nt, 1.0), S.E, S.nr_cams, dict(S.meta))
    return P


class Side:
    """one side of a call as the C ABI takes it: desc / mask [nsets, pitch, stride] bytes (mask None: unmasked; inter: the mask sits at byte `dim` of the
    descriptor's row), valid / group [nsets, pitch], rays [nsets, pitch, 3]; phys = the array row of set row i"""


def lay_side(d, m, v, cam, rays, dim, how, bait, bait_ray):
    nsets, n = d.shape[:2]
    L = Side()
    L.n, L.dim, L.how = n, dim, how
    L.stride = {"plain": dim, "stride4": dim + 4, "stride16": dim + 16, "inter": 2 * dim if m is not None else dim, "blocks": dim}[how]
    L.inter = how == "inter" and m is not None
    L.block_rows = n // 3 if how == "blocks" and n >= 3 else 0
    assert L.block_rows == 0 or n % 3 == 0
    L.block_pitch = L.block_rows + 2 if L.block_rows else 0
    i = np.arange(n)
    L.phys = i if not L.block_rows else (i // L.block_rows) * L.block_pitch + i % L.block_rows
    span = n if not L.block_rows else 2 * L.block_pitch + L.block_rows
    L.pitch = span + 1
    # every array row the set does not own is BAIT (bait_for): valid, full mask, camera 0; the bytes between rows are 0xA5
    L.desc = np.full((nsets, L.pitch, L.stride), 0xA5, np.uint8)
    L.desc[:, :, :dim] = bait
    L.desc[:, L.phys, :dim] = d
    L.mask = None
    if L.inter:
        L.desc[:, :, dim:] = 0xFF
        L.desc[:, L.phys, dim:] = m
    elif m is not None:
        L.mask = np.full((nsets, L.pitch, L.stride), 0xA5, np.uint8)
        L.mask[:, :, :dim] = 0xFF
        L.mask[:, L.phys, :dim] = m
    L.valid = np.ones((nsets, L.pitch), np.uint8)
    L.valid[:, L.phys] = v
    L.group = L.rays = None
    if cam is not None:
        L.group = np.zeros((nsets, L.pitch), np.int32)
        L.group[:, L.phys] = cam
    if rays is not None:
        L.rays = np.broadcast_to(bait_ray, (nsets, L.pitch, 3)).copy()
        L.rays[:, L.phys] = rays
    return L


def read_side(L):
    """the set rows back out of the laid-out arrays -> (desc, mask, valid, group, rays)"""
    d = L.desc[:, L.phys, :L.dim]
    m = L.desc[:, L.phys, L.dim:2 * L.dim] if L.inter else (None if L.mask is None else L.mask[:, L.phys, :L.dim])
    return d, m, L.valid[:, L.phys], None if L.group is None else L.group[:, L.phys], None if L.rays is None else L.rays[:, L.phys]




def one_set(S, k=0):
    """set pair k of S on its own"""
    c = lambda a: None if a is None else a[k:k + 1]
    E = None if S.E is None else S.E[k:k + 1] if len(S.E) > 1 else S.E
    return Sets(S.mode, S.dim, S.masked, c(S.dq), c(S.mq), c(S.vq), c(S.dt), c(S.mt), c(S.vt), c(S.camq), c(S.camt), c(S.raysq), c(S.rayst), E, S.nr_cams)


def bait_for(S):
    """-> (descriptor, ray, (set, query) | None) of the bait row that fills every array row a set does not own.  The bait is a copy of a query (of one of the
    first 8 set pairs) that the search leaves WITHOUT a match although it has a row in reach (SearchByBoW: rejected at ratio 1.0 with best > 0, hence at every
    smaller ratio; triangulation: a query of camera 0 — the camera index of the rows between the blocks), with full masks and, for the triangulation search, a ray
    in that query's epipolar plane: a kernel that read one such row as a train row would find it at distance 0 and match the query.  None: the sets have no such
    query (the bait is a copy of query 0 then); tests/test_oracle_hostile_match_cpu.py asserts that the sets of the layout test have one and that the row,
    appended, changes the outcome"""
    if "bait" not in S.meta:
        desc = S.dq[0, 0] if S.nq else np.zeros(S.dim, np.uint8)
        ray, pick = np.array([0.0, 0.0, 1.0]), None
        for k in range(min(S.nsets, 8) if S.nq and S.nt else 0):
            book = []
            _, out = define_search(one_set(S, k), 1.0, book)
            if S.mode == 2:
                free = [i for i in range(S.nq) if S.vq[k, i] and S.camq[k, i] == 0 and out[0, i] < 0]
            else:
                free = [i for _, i, best, second, ok in book if not ok and 0 < best < INT_MAX]
            if free:
                pick = (k, free[0])
                desc = S.dq[pick]
                if S.mode == 2:
                    ray = _unit(S.raysq[pick] + 0.3 * _unit(tri_t(0)))
                break
        S.meta["bait"] = (desc.copy(), ray, pick)
    return S.meta["bait"]


def with_bait_row(S, k):
    """set pair k of S with the bait row appended to the train side as a row of its own (what a kernel that read one row too many would see)"""
    desc, ray, _ = bait_for(S)
    S0 = one_set(S, k)
    app = lambda a, v: None if a is None else np.concatenate([a, np.broadcast_to(np.asarray(v, a.dtype), (1, 1) + a.shape[2:])], axis=1)
    return Sets(S.mode, S.dim, S.masked, S0.dq, S0.mq, S0.vq, app(S0.dt, desc), app(S0.mt, 0xFF), app(S0.vt, 1), S0.camq, app(S0.camt, 0), S0.raysq, app(S0.rayst, ray),
                S0.E, S.nr_cams)


def lay(S, how="plain"):
    """-> (S or its padded form, query Side, train Side)"""
    bait, bait_ray, _ = bait_for(S)
    if how == "blocks":
        S = pad_rows(S, 3)
    q = lay_side(S.dq, S.mq if S.masked else None, S.vq, S.camq, S.raysq, S.dim, how, bait, bait_ray)
    t = lay_side(S.dt, S.mt if S.masked else None, S.vt, S.camt, S.rayst, S.dim, how, bait, bait_ray)
    return S, q, t


# ------------------------------------------------------------------------------------------------------------------- the lists both test files walk
DEGENERATE_CELLS = [(mode, dim, masked) for mode in (0, 1, 2) for dim in DIMS for masked in (False, True)]
DEGENERATE_KS = (1, 2, 4, 16, 32)
DEGENERATE_RATIO = 0.8
CHAIN_CELLS = [(16, False), (16, True), (32, True), (64, False), (64, True)]    # (the cells tests/test_gpu_greedy_chains.py lacks)
CHAIN_KS = (1, 4, 32)
CHAIN_RATIOS = ((0, (0.9, 1.0)), (1, (0.9,)))
LAYOUT_CELLS = ((32, True), (16, False))
LAYOUT_RATIOS = {0: (0.9, 1.0), 1: (0.9, 1.0), 2: (0.0,)}
RING_CELLS = [(32, True), (16, False), (64, True)]
RING_RANGES = ((0, 5), (3, 2))
RING_RATIO = 0.9


def degenerate_cases(mode, dim, masked):
    """-> [(K, name, Sets)] (cached)"""
    key = ("deg", mode, dim, masked)
    if key not in _cache:
        _cache[key] = [(K, name, S) for K in DEGENERATE_KS for name, S in degenerate_sets(mode, dim, masked, K)]
    return _cache[key]


def chain_cases(dim, masked, K):
    """-> [(mode, ratios, Sets)]: the chain sets are seeded with K"""
    key = ("chain", dim, masked, K)
    if key not in _cache:
        _cache[key] = [(mode, ratios, chain_sets(mode, dim, masked, K)) for mode, ratios in CHAIN_RATIOS]
    return _cache[key]


def layout_case(mode, dim, masked):
    """the set the layout wrappers are run on"""
    return tri_sets(dim, masked) if mode == 2 else table(mode, dim, masked, "b")[0]


def ring_frames(dim, masked):
    """5 tiny frames of one ring: (desc, mask, valid) [5, pitch, ...], rows per frame, frame pitch in rows"""
    key = ("ring", dim, masked)
    if key not in _cache:
        rng = np.random.default_rng([SEED, 8, dim, int(masked)])
        nf, n, pitch = 5, 61, 64
        centres = rng.integers(0, 256, (4, dim), dtype=np.uint8)
        d = np.full((nf, pitch, dim), 0x5A, np.uint8)
        m = np.full((nf, pitch, dim), 0xFF, np.uint8)
        v = np.ones((nf, pitch), np.uint8)
        for f in range(nf):
            d[f, :n] = clustered(rng, n, centres, 2 + f)
            v[f, :n] = rng.random(n) < 0.9
            if masked:
                m[f, :n] = np.packbits(rng.random((n, dim * 8)) < 0.9, axis=1)
        _cache[key] = (d, m, v, n, pitch)
    return _cache[key]


def ring_sets(dim, masked, first, count):
    """what mcs_search_kf_kf_ring(first, count) computes, as one Sets: pair s = frame first + s against the frame before it, frame 0 against the LAST frame"""
    key = ("ringsets", dim, masked, first, count)
    if key not in _cache:
        d, m, v, n, _ = ring_frames(dim, masked)
        f = np.arange(first, first + count)
        p = (f - 1) % len(d)
        c = np.ascontiguousarray
        _cache[key] = Sets(0, dim, masked, c(d[f, :n]), c(m[f, :n]) if masked else None, c(v[f, :n]), c(d[p, :n]), c(m[p, :n]) if masked else None, c(v[p, :n]))
    return _cache[key]


def tri_margins(S):
    """dsqr of EVERY (query, row) pair of one camera that takes part, whether a search tests it or not (den == 0 left out)"""
    out = []
    for s in range(S.nsets):
        for i in np.flatnonzero(S.vq[s]):
            for j in np.flatnonzero((S.vt[s] != 0) & (S.camt[s] == S.camq[s, i])):
                dsqr = epipolar(S.raysq[s, i], S.rayst[s, j], S.E_of(s)[S.camq[s, i] * S.nr_cams + S.camt[s, j]])[1]
                if dsqr is not None:
                    out.append(dsqr)
    return out
