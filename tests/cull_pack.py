"""The raw C ABI of mcs_covis_set_keyframe_octaves / _cull_keyframes / _observations / _cull_points for the GPU tests, on top of tests/covis_pack.py: a device
store kept in step with a covis_model.Store that carries `octaves`, every array argument in host memory (kind 0) or device memory (kind 1), every output one
entry longer than the call may write with a sentinel there."""
import numpy as np

import covis_model as M
import cull_model as CM
from covis_pack import SENT, Both, Dev
from newpoints_pack import Mem


class CullDev(Dev):
    def set_octaves(self, kid, octs):
        mem = Mem(self.G, self.device)
        o = np.ascontiguousarray(octs, np.uint8)
        return self.L.mcs_covis_set_keyframe_octaves(self.h, int(kid), mem.p(o if len(o) else np.zeros(1, np.uint8)), len(o), self.kind)

    def cull_keyframes(self, ids, not_erase, cap):
        mem, n = Mem(self.G, self.device), len(ids)
        kid = np.ascontiguousarray(ids, np.int64)
        ne = None if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
        o = dict(v=mem.out(np.full(n + 1, SENT, np.int32)), m=mem.out(np.full(n + 1, SENT, np.int32)), r=mem.out(np.full(n + 1, SENT, np.int32)),
                 bp=mem.out(np.full(cap + 1, SENT, np.int32)), nb=mem.out(np.full(2, SENT, np.int32)))
        rc = self.L.mcs_covis_cull_keyframes(self.h, n, kid.ctypes.data, None if ne is None else ne.ctypes.data, cap, self.kind, o["v"][0], o["m"][0], o["r"][0],
                                             o["bp"][0], o["nb"][0])
        assert rc == 0, self.L.mcs_last_error()
        r = {k: v[1]() for k, v in o.items()}
        for k in r:
            assert r[k][-1] == SENT, "%s: written past its end" % k
        nb = int(r["nb"][0])
        assert nb >= 0 and (r["bp"][min(nb, cap):cap] == -1).all()                                        # bad_points[n_bad_points .. cap) reads -1
        return dict(verdict=r["v"][:n].tolist(), n_mps=r["m"][:n].tolist(), n_redundant=r["r"][:n].tolist(), bad_points=r["bp"][:min(nb, cap)].tolist(),
                    n_bad_points=nb)

    def observations(self, ids):
        mem = Mem(self.G, self.device)
        ids = np.ascontiguousarray(ids, np.int32)
        o = mem.out(np.full(len(ids) + 1, SENT, np.int32))
        rc = self.L.mcs_covis_observations(self.h, mem.p(ids), len(ids), self.kind, o[0])
        assert rc == 0, self.L.mcs_last_error()
        r = o[1]()
        assert r[-1] == SENT
        return r[:-1].tolist()

    def cull_points(self, cur, ids, found, visible, first, expect=0):
        mem = Mem(self.G, self.device)
        ids = np.ascontiguousarray(ids, np.int32)
        o = mem.out(np.full(len(ids) + 1, SENT, np.int32))
        rc = self.L.mcs_covis_cull_points(self.h, int(cur), len(ids), mem.p(ids), mem.p(np.ascontiguousarray(found, np.int32)),
                                          mem.p(np.ascontiguousarray(visible, np.int32)), mem.p(np.ascontiguousarray(first, np.int64)), self.kind, o[0])
        assert rc == expect, self.L.mcs_last_error()
        r = o[1]()
        assert r[-1] == SENT
        return r[:-1].tolist()


class CullBoth(Both):
    """a model Store with octaves and a device store that receive the same operations"""

    def __init__(self, pkg, G, max_kf, max_feat, max_pts, device):
        self.m, self.d = M.Store(), CullDev(pkg, G, max_kf, max_feat, max_pts, device)
        self.m.octaves = {}

    @classmethod
    def of(cls, pkg, G, store, octaves, device, max_kf=None, max_feat=None, max_pts=None):
        b = super().of(pkg, G, store, device, max_kf, max_feat, max_pts)
        for k in sorted(store.rows):
            if k in (octaves or {}):
                b.set_octaves(k, octaves[k])
        return b

    def set_keyframe(self, kid, points):
        if kid not in self.m.rows or len(self.m.rows[kid]) != len(points):
            self.m.octaves[kid] = [0] * len(points)               # a new row, or one of another length, reads level 0
        super().set_keyframe(kid, points)

    def set_octaves(self, kid, octs):
        self.m.octaves[kid] = [int(o) for o in octs]
        assert self.d.set_octaves(kid, octs) == 0, self.d.L.mcs_last_error()

    def erase(self, kid):
        super().erase(kid)
        self.m.octaves.pop(kid, None)

    def points(self):
        return sorted(set(p for r in self.m.rows.values() for p in r if p >= 0) | self.m.pt_bad)

    def check_observations(self, ids=None, where=""):
        ids = self.points() if ids is None else ids
        if len(ids):
            got, want = self.d.observations(ids), CM.observations(self.m, ids)
            assert got == want, (where, [(p, g, w) for p, g, w in zip(ids, got, want) if g != w][:10])

    def check_cull(self, ids, not_erase=None, cap=None, where="", erase=True):
        """one mcs_covis_cull_keyframes against the model; afterwards the culled keyframes are erased on both sides (the caller's part) and the store's state is
        read back through mcs_covis_observations and a following mcs_covis_update_reference"""
        want = CM.keyframe_culling(self.m, self.m.octaves, ids, not_erase)
        full = len(want["bad_points"])
        cap = full + 3 if cap is None else cap
        got = self.d.cull_keyframes(ids, not_erase, cap)
        for k in ("verdict", "n_mps", "n_redundant"):
            assert got[k] == want[k], (where, k, got[k], want[k])
        assert got["n_bad_points"] == full and got["bad_points"] == want["bad_points"][:cap], (where, got["n_bad_points"], full, got["bad_points"], want["bad_points"])
        holes = self.m.holes
        self.m = want["store"]
        self.m.holes = holes
        pts = self.points()
        self.check_observations(pts, where)                       # culled rows still count for other calls until they are erased
        if erase:
            for k in want["culled"]:
                self.erase(k)
            self.check_observations(pts, where)
        frame = np.array((pts * 3)[:max(8, min(len(pts) * 2, 400))], np.int32)
        self.check_reference(frame, (0.1, 0.2, 0.3), where=where)   # bad points are nulled in the frame, bad keyframes are not local
        return want

    def check_cull_points(self, cur, ids, found, visible, first, where=""):
        want = CM.map_point_culling(self.m, cur, ids, found, visible, first)
        got = self.d.cull_points(cur, ids, found, visible, first)
        assert got == want["verdict"], (where, got, want["verdict"])
        oct_ = self.m.octaves
        holes = self.m.holes
        self.m = want["store"]
        self.m.octaves, self.m.holes = oct_, holes
        self.check_observations(list(ids), where)
        return want
