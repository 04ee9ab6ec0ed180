"""The raw C ABI of mcs_covis_* for the GPU tests: a device store kept in step with a tests/covis_model.py Store, every array argument in host memory
(kind 0) or in hipMalloc'ed memory (kind 1, gpu_common.DevBuf), results in the shape of the model's.  Every output array is one entry longer than the call
may write and carries a sentinel there."""
import ctypes as C

import numpy as np

import covis_model as M
from newpoints_pack import Mem

SENT = -77


class Dev:
    def __init__(self, pkg, G, max_kf, max_feat, max_pts, device):
        self.pkg, self.G, self.L, self.device, self.kind = pkg, G, pkg.lib(), device, 1 if device else 0
        self.h = C.c_void_p()
        pkg._capi.check(self.L.mcs_covis_create(G.ctx().h, max_kf, max_feat, max_pts, C.byref(self.h)))
        self.slot_ids = []

    def __del__(self):
        try:
            self.L.mcs_covis_destroy(self.h)
        except Exception:
            pass

    def _n(self, fn):
        n = C.c_int32(-1)
        assert fn(self.h, C.byref(n)) == 0
        return n.value

    def size(self):
        return self._n(self.L.mcs_covis_size)

    def slots(self):
        return self._n(self.L.mcs_covis_slots)

    def set_keyframe(self, kid, points):
        mem = Mem(self.G, self.device)
        pts = np.ascontiguousarray(points, np.int32)
        rc = self.L.mcs_covis_set_keyframe(self.h, int(kid), mem.p(pts), len(pts), self.kind)
        if rc == 0 and (not self.slot_ids or kid > self.slot_ids[-1]):
            self.slot_ids.append(int(kid))
        return rc

    def set_pose(self, ids, ts):
        mem = Mem(self.G, self.device)
        ids = np.ascontiguousarray(ids, np.int64)
        return self.L.mcs_covis_set_keyframe_pose(self.h, len(ids), ids.ctypes.data, mem.p(np.ascontiguousarray(ts, np.float64)), self.kind)

    def erase(self, kid):
        return self.L.mcs_covis_erase_keyframe(self.h, int(kid))

    def set_bad(self, kid, bad=True):
        return self.L.mcs_covis_set_keyframe_bad(self.h, int(kid), int(bad))

    def set_points_bad(self, ids, bad=True):
        mem = Mem(self.G, self.device)
        ids = np.ascontiguousarray(ids, np.int32)
        flags = np.ascontiguousarray(np.broadcast_to(np.asarray(bad, bool), ids.shape), np.uint8)
        return self.L.mcs_covis_set_points_bad(self.h, mem.p(ids), len(ids), mem.p(flags), self.kind)

    def update_reference(self, frame_points, frame_t, cap):
        """-> the model's dict + n_points (full count) and the padding of every output"""
        mem, S = Mem(self.G, self.device), self.slots()
        fp = mem.out(np.ascontiguousarray(frame_points, np.int32).copy())
        o = dict(kfs=mem.out(np.full(S + 1, SENT, np.int64)), w=mem.out(np.full(S + 1, SENT, np.int32)), d=mem.out(np.full(S + 1, float(SENT))),
                 nl=mem.out(np.full(2, SENT, np.int32)), ref=mem.out(np.full(2, SENT, np.int64)), lp=mem.out(np.full(cap + 1, SENT, np.int32)),
                 np=mem.out(np.full(2, SENT, np.int32)))
        rc = self.L.mcs_covis_update_reference(self.h, fp[0], len(frame_points), mem.p(np.ascontiguousarray(frame_t, np.float64)), cap, self.kind, o["kfs"][0],
                                               o["w"][0], o["d"][0], o["nl"][0], o["ref"][0], o["lp"][0], o["np"][0])
        assert rc == 0, self.L.mcs_last_error()
        r = {k: v[1]() for k, v in o.items()}
        for k in r:
            assert r[k][-1] == SENT, "%s: written past its end" % k
        n, npts = int(r["nl"][0]), int(r["np"][0])
        assert 0 <= n <= S and npts >= 0
        assert (r["kfs"][n:S] == -1).all() and (r["w"][n:S] == 0).all() and (r["d"][n:S] == 0).all()        # the rest of the per-slot outputs
        assert (r["lp"][min(npts, cap):cap] == -1).all()                                                  # local_points[n_points .. cap) reads -1
        return dict(frame_points=fp[1]().tolist(), local_kfs=r["kfs"][:n].tolist(), weights=r["w"][:n].tolist(), dists=r["d"][:n].tolist(), ref_kf=int(r["ref"][0]),
                    local_points=r["lp"][:min(npts, cap)].tolist(), n_points=npts)

    def update_connections(self, ids):
        mem, S, nq = Mem(self.G, self.device), self.slots(), len(ids)
        qid = np.ascontiguousarray(ids, np.int64)
        o = dict(cnt=mem.out(np.full(nq * S + 1, SENT, np.int32)), nc=mem.out(np.full(nq + 1, SENT, np.int32)), od=mem.out(np.full(nq * S + 1, SENT, np.int64)),
                 ow=mem.out(np.full(nq * S + 1, SENT, np.int32)), no=mem.out(np.full(nq + 1, SENT, np.int32)))
        rc = self.L.mcs_covis_update_connections(self.h, nq, qid.ctypes.data, self.kind, o["cnt"][0], o["nc"][0], o["od"][0], o["ow"][0], o["no"][0])
        assert rc == 0, self.L.mcs_last_error()
        r = {k: v[1]() for k, v in o.items()}
        for k in r:
            assert r[k][-1] == SENT, "%s: written past its end" % k
        out = []
        for q in range(nq):
            c, n = r["cnt"][q * S:(q + 1) * S], int(r["no"][q])
            counter = {self.slot_ids[int(k)]: int(c[k]) for k in np.flatnonzero(c)}
            assert (c >= 0).all() and len(counter) == int(r["nc"][q])
            m = max(n, 0)
            assert (r["od"][q * S + m:(q + 1) * S] == -1).all() and (r["ow"][q * S + m:(q + 1) * S] == 0).all()
            out.append(dict(counter=counter, ordered=None if n < 0 else r["od"][q * S:q * S + n].tolist(), weights=None if n < 0 else r["ow"][q * S:q * S + n].tolist()))
        return out


class Both:
    """a model Store and a device store that receive the same operations"""

    def __init__(self, pkg, G, max_kf, max_feat, max_pts, device):
        self.m, self.d = M.Store(), Dev(pkg, G, max_kf, max_feat, max_pts, device)

    @classmethod
    def of(cls, pkg, G, store, device, max_kf=None, max_feat=None, max_pts=None):
        """a pair holding what `store` (without holes) holds"""
        ids = sorted(store.rows)
        b = cls(pkg, G, max_kf or max(len(ids), 1), max_feat or max([len(store.rows[k]) for k in ids] + [1]),
                max_pts or max([p for k in ids for p in store.rows[k]] + list(store.pt_bad) + [0]) + 1, device)
        for k in ids:
            b.set_keyframe(k, store.rows[k])
        if ids:
            b.set_pose(ids, [store.t[k] for k in ids])
        for k in ids:
            if store.kf_bad[k]:
                b.set_bad(k)
        if store.pt_bad:
            b.set_points_bad(sorted(store.pt_bad))
        return b

    def set_keyframe(self, kid, points):
        self.m.set_keyframe(kid, points)
        assert self.d.set_keyframe(kid, points) == 0

    def set_pose(self, ids, ts):
        for k, t in zip(ids, ts):
            self.m.t[k] = tuple(float(v) for v in t)
        assert self.d.set_pose(ids, ts) == 0

    def erase(self, kid):
        self.m.erase(kid)
        assert self.d.erase(kid) == 0

    def set_bad(self, kid, bad=True):
        self.m.kf_bad[kid] = bool(bad)
        assert self.d.set_bad(kid, bad) == 0

    def set_points_bad(self, ids, bad=True):
        for p in ids:
            (self.m.pt_bad.add if bad else self.m.pt_bad.discard)(int(p))
        assert self.d.set_points_bad(ids, bad) == 0

    def check_reference(self, frame_points, frame_t, cap=None, where=""):
        want = M.update_reference(self.m, frame_points, frame_t)
        full = len(want["local_points"])
        cap = full + 3 if cap is None else cap
        got = self.d.update_reference(frame_points, frame_t, cap)
        assert got["frame_points"] == want["frame_points"], where
        assert got["local_kfs"] == want["local_kfs"] and got["weights"] == want["weights"] and got["ref_kf"] == want["ref_kf"], (where, got, want)
        assert np.array(got["dists"]).tobytes() == np.array(want["dists"]).tobytes(), (where, got["dists"], want["dists"])   # + - * sqrt only: bit for bit
        assert got["n_points"] == full and got["local_points"] == want["local_points"][:cap], (where, got["n_points"], full)
        return want

    def check_connections(self, ids, where=""):
        want = [M.update_connections(self.m, k) for k in ids]
        got = self.d.update_connections(ids)
        assert got == want, (where, got, want)
        return want
