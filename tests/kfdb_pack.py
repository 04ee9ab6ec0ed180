"""The raw C ABI of the keyframe database (mcs_kfdb_add / _erase / _set_covisibility / _detect_relocalisation / _detect_loop / _score) next to the model of
tests/kfdb_model.py, both driven by one script of operations (tests/hostile_kfdb.py builds them): host-kind calls on numpy arrays, device-kind calls on
hipMalloc'ed copies (gpu_common.DevBuf).  check(script, dev) steps the model and, when a device side is given, the library, and compares after every query:
candidate ids, counts, and the diagnostic rows (ids, word counters, best ids as equal values, scores and accumulated scores as equal bits).

Only the first cand_count[q] ids and the first diag.count[q] diagnostic rows of a query are compared, in both memory kinds: the rows past them are copied
from the call's scratch and are unspecified.

A script is a list of operations:
    ("add", [(id, words, values), ...], opts)            one mcs_kfdb_add call; opts: expect = (code, text) of a refusal (the model is then not stepped)
    ("erase", [ids])
    ("covis", id, [neighbour ids])
    ("reloc", [(query id, words, values), ...], opts)    one batch; opts: cap, dcap, null_cands, expect = "capacity" (counts compared, state unchanged)
    ("loop", [(query id, words, values, min score, [connected ids]), ...], opts)
                                                         opts of both: refuse = {device kind?: (code, text)}: a bad query batch, refused; no state moves
    ("add_raw", ids, offsets, words, values, opts)       an add by its raw CSR arrays (offsets that no list of rows gives); opts: expect = (code, text)
    ("score", words, values, [ids], opts)                mcs_kfdb_score, bits against the model's l1_score; opts: expect = (code, text), host = True: this
                                                         call's arrays in host memory whatever the kind of the run
    ("hook", name)                                      nothing; a place where a mutation of the model can act (tests/test_kfdb_hostile_cpu.py)
This module imports nothing of the library: the package and gpu_common are handed in."""
import ctypes as C
import struct

import numpy as np

import kfdb_model as M

OK, INVALID, CAPACITY = 0, -1, -3
STATE = ("mnRelocQuery", "mnRelocWords", "mRelocScore", "mnLoopQuery", "mnLoopWords", "mLoopScore")


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def trace_key(trace):
    """a model trace with its doubles as bit patterns: equal keys = equal values and equal bits"""
    return [(int(i), int(w), bits(s), bits(a), int(b)) for i, w, s, a, b in trace]


def bow(words, values):
    return list(zip([int(x) for x in words], [float(x) for x in values]))


def csr(rows):
    """[(words, values)] -> offsets, words, values"""
    off = np.zeros(len(rows) + 1, np.int32)
    off[1:] = np.cumsum([len(r[0]) for r in rows])
    w = np.array([x for r in rows for x in r[0]], np.int32)
    v = np.array([x for r in rows for x in r[1]], np.float64)
    return off, w, v


class ModelSide:
    """kfdb_model.Database with one KF object per keyframe id, as the device keeps one slot per id (ghosts: ids only ever named as neighbours)"""

    def __init__(self, n_words):
        self.db = M.Database(n_words)
        self.kf, self.active = {}, set()

    def get(self, i):
        if i not in self.kf:
            self.kf[i] = M.KF(i, [])
        return self.kf[i]

    def add(self, i, b):
        k = self.get(i)
        assert i not in self.active
        k.bow = b
        self.db.add(k)
        self.active.add(i)

    def erase(self, i):
        if i in self.active:
            self.db.erase(self.kf[i])
            self.active.remove(i)

    def covis(self, i, nbs):
        self.get(i).neighbours = [self.get(j) for j in nbs]

    def reloc(self, qid, b):
        t = []
        c = self.db.DetectRelocalisationCandidates(int(qid), b, trace=t)
        return [k.mnId for k in c], t

    def loop(self, qid, b, min_score, conn):
        t = []
        c = self.db.DetectLoopCandidates(M.KF(qid, b), float(min_score), [self.kf[x] for x in conn if x in self.kf], trace=t)
        return [k.mnId for k in c], t

    def score(self, b, ids):
        return [M.l1_score(b, self.kf[i].bow) for i in ids]

    def snapshot(self):
        return {i: tuple(getattr(k, f) for f in STATE) for i, k in self.kf.items()}

    def restore(self, snap):
        for i, k in self.kf.items():
            for f, x in zip(STATE, snap.get(i, (0, 0, 0.0, 0, 0, 0.0))):
                setattr(k, f, x)


class DeviceSide:
    """one mcs_kfdb through the C ABI; every array argument of a call in host memory (device=False) or in device memory"""

    def __init__(self, pkg, G, n_words, device=False):
        self.pkg, self.G, self.device, self.L = pkg, G, bool(device), pkg.lib()
        self.kind = pkg.MEM_DEVICE if device else pkg.MEM_HOST
        self.h = C.c_void_p()
        pkg.check(self.L.mcs_kfdb_create(G.ctx().h, int(n_words), 0, C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self.L.mcs_kfdb_destroy(self.h)
        except Exception:
            pass

    def _in(self, arr, keep):
        arr = np.ascontiguousarray(arr)
        if self.device:
            b = self.G.DevBuf(arr)
            keep.append(b)
            return b.ptr.value
        keep.append(arr)
        return arr.ctypes.data

    def _out(self, arr, keep):
        if self.device:
            b = self.G.DevBuf(arr)
            keep.append(b)
            return b.ptr.value, b.read
        keep.append(arr)
        return arr.ctypes.data, (lambda: arr)

    def error(self):
        return self.L.mcs_last_error().decode("utf-8", "replace")

    def add_raw(self, ids, off, w, v):
        keep = []
        return self.L.mcs_kfdb_add(self.h, len(ids), self._in(np.asarray(ids, np.int64), keep), self._in(np.asarray(off, np.int32), keep),
                                   self._in(np.asarray(w, np.int32), keep), self._in(np.asarray(v, np.float64), keep), self.kind)

    def add(self, items):
        off, w, v = csr([(x[1], x[2]) for x in items])
        return self.add_raw([x[0] for x in items], off, w, v)

    def erase(self, ids):
        a = np.asarray(ids, np.int64)
        self.pkg.check(self.L.mcs_kfdb_erase(self.h, len(a), a.ctypes.data))

    def covis(self, i, nbs):
        a, n = np.zeros(10, np.int64), np.array([len(nbs)], np.int32)
        a[:len(nbs)] = nbs
        self.pkg.check(self.L.mcs_kfdb_set_covisibility(self.h, 1, np.array([i], np.int64).ctypes.data, a.ctypes.data, n.ctypes.data))

    def size(self):
        n = C.c_int32()
        self.pkg.check(self.L.mcs_kfdb_size(self.h, C.byref(n)))
        return n.value

    def detect(self, loop, queries, cap, dcap, null_cands=False):
        """-> rc, counts [nq], candidates (first min(count, cap) ids per query), diagnostic counts [nq], traces (first min(count, dcap) rows per query)"""
        nq, keep = len(queries), []
        off, w, v = csr([(q[1], q[2]) for q in queries])
        qid = np.array([q[0] for q in queries], np.int64)
        pc, rc_ = self._out(np.full(max(nq, 1), -9, np.int32), keep)
        po, ro = (None, None) if null_cands else self._out(np.full(max(nq * cap, 1), -77, np.int64), keep)
        dn = max(nq * dcap, 1)
        pdc, rdc = self._out(np.full(max(nq, 1), -9, np.int32), keep)
        pid, rid = self._out(np.full(dn, -77, np.int64), keep)
        pw, rw = self._out(np.full(dn, -9, np.int32), keep)
        ps, rs = self._out(np.full(dn, -7.0), keep)
        pa, ra = self._out(np.full(dn, -7.0), keep)
        pb, rb = self._out(np.full(dn, -77, np.int64), keep)
        diag = self.pkg._capi.KfdbDiag(dcap, pdc, pid, pw, ps, pa, pb)
        a = [self.h, nq, self._in(qid, keep), self._in(off, keep), self._in(w, keep) if len(w) else None, self._in(v, keep) if len(v) else None]
        if loop:
            coff = np.zeros(nq + 1, np.int32)
            coff[1:] = np.cumsum([len(q[4]) for q in queries])
            cids = np.array([x for q in queries for x in q[4]], np.int64)
            a += [self._in(coff, keep), self._in(cids, keep) if len(cids) else None, self._in(np.array([q[3] for q in queries], np.float64), keep)]
        f = self.L.mcs_kfdb_detect_loop if loop else self.L.mcs_kfdb_detect_relocalisation
        rc = f(*a, self.kind, cap, pc, po, C.byref(diag))
        if rc not in (OK, CAPACITY):
            return rc, None, None, None, None
        cnt, dc = rc_()[:nq].tolist(), rdc()[:nq].tolist()
        o = None if null_cands else ro()
        cands = [[] if o is None else o[q * cap:q * cap + min(cnt[q], cap)].tolist() for q in range(nq)]
        i_, w_, s_, a_, b_ = rid(), rw(), rs(), ra(), rb()
        traces = []
        for q in range(nq):
            r = slice(q * dcap, q * dcap + min(dc[q], dcap))
            traces.append(list(zip(i_[r].tolist(), w_[r].tolist(), s_[r].view(np.uint64).tolist(), a_[r].view(np.uint64).tolist(), b_[r].tolist())))
        return rc, cnt, cands, dc, traces

    def score(self, w, v, ids, host=False):
        """host: the arrays in host memory for this one call, whatever the kind of the side"""
        keep, was = [], (self.device, self.kind)
        if host:
            self.device, self.kind = False, self.pkg.MEM_HOST
        try:
            po, ro = self._out(np.full(max(len(ids), 1), -7.0), keep)
            rc = self.L.mcs_kfdb_score(self.h, len(w), self._in(np.asarray(w, np.int32), keep) if len(w) else None,
                                       self._in(np.asarray(v, np.float64), keep) if len(w) else None, len(ids),
                                       self._in(np.asarray(ids, np.int64), keep) if len(ids) else None, self.kind, po)
            return rc, (ro()[:len(ids)] if rc == OK else None)
        finally:
            self.device, self.kind = was


class Vocab:
    """a hand-built vocabulary through mcs_vocabulary_create / mcs_vocabulary_set_words, and mcs_bow_vector on it in either memory kind"""

    def __init__(self, pkg, G, node_desc, child_off, child_idx, L=1):
        self.pkg, self.G, self.L_ = pkg, G, pkg.lib()
        self.h = C.c_void_p()
        self.keep = [np.ascontiguousarray(node_desc, np.uint8), np.ascontiguousarray(child_off, np.int32), np.ascontiguousarray(child_idx, np.int32)]
        pkg.check(self.L_.mcs_vocabulary_create(G.ctx().h, len(self.keep[0]), *[a.ctypes.data for a in self.keep], L, C.byref(self.h)))

    def __del__(self):
        try:
            if self.h:
                self.L_.mcs_vocabulary_destroy(self.h)
        except Exception:
            pass

    def set_words(self, word, weight):
        """-> (code, text)"""
        w, t = np.ascontiguousarray(word, np.int32), np.ascontiguousarray(weight, np.float64)
        rc = self.L_.mcs_vocabulary_set_words(self.h, w.ctypes.data, t.ctypes.data)
        return rc, (self.L_.mcs_last_error().decode("utf-8", "replace") if rc else "")

    def bow_vector(self, leaf, device):
        """-> (code, [(word, bits of the value)]) : the first nwords_out entries; the outputs hold max(n, 1) entries"""
        leaf = np.ascontiguousarray(leaf, np.int32)
        n = len(leaf)
        ow, ov, on = np.full(max(n, 1), -9, np.int32), np.full(max(n, 1), -7.0), np.full(1, -9, np.int32)
        if device:
            dl, dw, dv, dn = self.G.DevBuf(leaf), self.G.DevBuf(ow), self.G.DevBuf(ov), self.G.DevBuf(on)
            rc = self.L_.mcs_bow_vector(self.h, dl.ptr.value if n else None, n, self.pkg.MEM_DEVICE, dw.ptr.value, dv.ptr.value, dn.ptr.value)
            if rc:
                return rc, None
            ow, ov, on = dw.read(), dv.read(), dn.read()
        else:
            rc = self.L_.mcs_bow_vector(self.h, leaf.ctypes.data if n else None, n, self.pkg.MEM_HOST, ow.ctypes.data, ov.ctypes.data, on.ctypes.data)
            if rc:
                return rc, None
        k = int(on[0])
        assert 0 <= k <= n
        return rc, list(zip(ow[:k].tolist(), ov[:k].view(np.uint64).tolist()))


def model_bow_vector(word, weight, leaf):
    """kfdb_model.bow_vector over the leaves' words and weights -> [(word, bits of the value)]"""
    leaf = np.asarray(leaf, np.int64)
    return [(w, bits(v)) for w, v in M.bow_vector(np.asarray(word)[leaf].tolist(), np.asarray(weight)[leaf].tolist())]


def _model_queries(mod, kind, queries, mut):
    out, start = [], None
    if mut.get("no_carry"):   # mutation: a query of a batch does not see the scores the earlier queries of the batch wrote
        start = {i: (k.mRelocScore, k.mLoopScore) for i, k in mod.kf.items()}
    for q in queries:
        if start is not None and out:
            for i, k in mod.kf.items():
                k.mRelocScore, k.mLoopScore = start.get(i, (0.0, 0.0))
        b = bow(q[1], q[2])
        out.append(mod.reloc(q[0], b) if kind == "reloc" else mod.loop(q[0], b, q[3], q[4]))
    return out


def check(script, n_words, dev=None, batched=True, mut=None, mod=None):
    """Steps the model through the script and, with dev (a DeviceSide), the library next to it, comparing every query.  batched=False issues the queries
    of a batch one call each.  -> (model side, [per query operation: [(candidate ids, trace)] per query])."""
    mut = mut or {}
    mod = mod or ModelSide(n_words)
    results = []
    for op in script:
        kind = op[0]
        if kind == "add":
            opts = op[2] if len(op) > 2 else {}
            if dev is not None:
                rc = dev.add(op[1])
                if "expect" in opts:
                    assert (rc, dev.error()) == tuple(opts["expect"]), (rc, dev.error())
                else:
                    assert rc == OK, dev.error()
            if "expect" not in opts:
                for i, w, v in op[1]:
                    mod.add(i, bow(w, v))
            if dev is not None:
                assert dev.size() == len(mod.active)
        elif kind == "add_raw":   # a refusal by the offsets: nothing for the model to do
            if dev is not None:
                rc = dev.add_raw(*op[1:5])
                assert (rc, dev.error()) == tuple(op[5]["expect"]), (rc, dev.error())
                assert dev.size() == len(mod.active)
        elif kind == "score":
            opts = op[4] if len(op) > 4 else {}
            want = None if "expect" in opts else mod.score(bow(op[1], op[2]), op[3])
            results.append(want)
            if dev is not None:
                rc, got = dev.score(op[1], op[2], op[3], host=opts.get("host", False))
                if "expect" in opts:
                    assert (rc, dev.error()) == tuple(opts["expect"]), (rc, dev.error())
                else:
                    assert rc == OK, dev.error()
                    assert [bits(x) for x in got] == [bits(x) for x in want], "scores differ in bits"
        elif kind == "erase":
            for i in op[1]:
                mod.erase(i)
            if dev is not None:
                dev.erase(op[1])
        elif kind == "covis":
            mod.covis(op[1], op[2])
            if dev is not None:
                dev.covis(op[1], op[2])
        elif kind == "hook":
            if op[1] in mut.get("hook", {}):
                mut["hook"][op[1]](mod)
        elif kind in ("reloc", "loop"):
            queries = op[1]
            opts = op[2] if len(op) > 2 else {}
            if "refuse" in opts:   # a bad query: code and text by memory kind; neither side's state moves
                if dev is not None:
                    rc = dev.detect(kind == "loop", queries, 8, 8)[0]
                    assert (rc, dev.error()) == tuple(opts["refuse"][dev.device]), (rc, dev.error())
                continue
            snap = mod.snapshot() if opts.get("expect") == "capacity" else None
            want = _model_queries(mod, kind, queries, mut)
            results.append(want)
            if snap is not None:
                mod.restore(snap)   # the library leaves its state as it was
            if dev is None:
                continue
            longest = max([len(t) for _, t in want] + [1])
            cap, dcap = opts.get("cap", longest), opts.get("dcap", longest)
            groups = [queries] if batched or snap is not None else [[q] for q in queries]
            k = 0
            for g in groups:
                rc, cnt, cands, dc, traces = dev.detect(kind == "loop", g, cap, dcap, opts.get("null_cands", False))
                assert rc == (CAPACITY if snap is not None else OK), (rc, dev.error())
                for j in range(len(g)):
                    wc, wt = want[k]
                    label = "%s query %d (id %d)" % (kind, k, g[j][0])
                    assert cnt[j] == len(wc) and dc[j] == len(wt), "%s: counts %d / %d, model %d / %d" % (label, cnt[j], dc[j], len(wc), len(wt))
                    if not opts.get("null_cands"):
                        assert cands[j] == wc[:cap], "%s: candidates %s, model %s" % (label, cands[j][:8], wc[:8])
                    tk = trace_key(wt)[:dcap]
                    if traces[j] != tk:
                        bad = [i for i in range(len(tk)) if traces[j][i] != tk[i]][0]
                        raise AssertionError("%s: diagnostic row %d is %s, model %s" % (label, bad, traces[j][bad], tk[bad]))
                    k += 1
        else:
            raise ValueError(kind)
    return mod, results
