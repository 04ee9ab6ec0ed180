"""-m gpu: every stage of the covisibility store in rotation on ONE device store (tests/rotation_case.py), host kind and device kind, each call compared with its
model bit for bit:  update_points -> cull_keyframes -> update_connections -> cull_points -> update_points -> observations -> update_reference ->
cull_keyframes -> update_reference.  The stages share the store's per-point scratch (mult, key, the level counters: csrc/mcs_covis.h) and the row walk; a
stage that leaves a mark behind spoils the NEXT stage's result, which no single-stage suite sees.  The last update_reference is also compared with the same call
on a FRESH store loaded with the model's end state: whatever the rotation left in the scratch would show there.

tests/test_covis_rotation_cpu.py runs the same sequence on the models alone and asserts that it is not vacuous."""
import importlib

import numpy as np
import pytest

import mappoint_model as MM
import rotation_case as RC
from cull_pack import CullDev
from newpoints_pack import Mem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import gpu_common as G
    return importlib.import_module("multicol-slam_amd"), G


class RotDev(CullDev):
    """cull_pack.CullDev and the raw C ABI of mcs_covis_set_keyframe_descriptors / mcs_covis_update_points"""

    def set_descriptors(self, kid, desc, mask):
        mem = Mem(self.G, self.device)
        d, m = np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(mask, np.uint8)
        return self.L.mcs_covis_set_keyframe_descriptors(self.h, int(kid), mem.p(d), mem.p(m), d.shape[1], d.shape[1], d.shape[0], self.kind)

    def update_points(self, ids, pos, ref, scales, d0, m0):
        """every output starts from the model's sentinels (desc / mask: from d0 / m0) and is one entry longer than the call may write"""
        mem, n = Mem(self.G, self.device), len(ids)
        S = MM.SENTINEL

        def padded(a):
            a = np.ascontiguousarray(a)
            return np.concatenate([a.reshape(n, -1), np.full((1, a.size // n), 0x3C, a.dtype)]).reshape(-1)

        o = dict(normal=mem.out(padded(np.full((n, 3), S["normal"]))), status=mem.out(padded(np.full(n, S["status"], np.int32))),
                 desc=mem.out(padded(d0)), mask=mem.out(padded(m0)), n_desc=mem.out(padded(np.full(n, S["n_desc"], np.int32))),
                 best_kf=mem.out(padded(np.full(n, S["best_kf"], np.int64))), best_feat=mem.out(padded(np.full(n, S["best_feat"], np.int32))))
        for k in ("min_dist", "max_dist", "min_inv", "max_inv"):
            o[k] = mem.out(padded(np.full(n, S[k])))
        rc = self.L.mcs_covis_update_points(self.h, n, mem.p(np.ascontiguousarray(ids, np.int32)), mem.p(np.ascontiguousarray(pos, np.float64)),
                                            mem.p(np.ascontiguousarray(ref, np.int64)), mem.p(np.ascontiguousarray(scales, np.float64)), len(scales), self.kind,
                                            o["normal"][0], o["min_dist"][0], o["max_dist"][0], o["min_inv"][0], o["max_inv"][0], o["desc"][0], o["mask"][0],
                                            o["n_desc"][0], o["best_kf"][0], o["best_feat"][0], o["status"][0])
        assert rc == 0, self.L.mcs_last_error()
        out = {}
        for k, v in o.items():
            a = v[1]().reshape(n + 1, -1)
            assert (a[n] == 0x3C).all(), "%s: written past its end" % k
            out[k] = a[:n]
        return out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("L", RC.LENGTHS)
def test_every_stage_in_rotation_on_one_store(env, L, device):
    pkg, G = env
    c = RC.make_case(L)
    b = RC.Rotation(RotDev(pkg, G, len(RC.KIDS), L, RC.MAX_PTS, device))
    RC.load(b, c)
    assert b.d.slots() == len(RC.KIDS) and b.d.size() == len(RC.KIDS) - 1
    log = RC.rotate(b, c)
    RC.assert_not_vacuous(c, log)
    # the same call on a store that never ran one, holding the model's end state
    f = RC.fresh_copy(b, RotDev(pkg, G, len(RC.KIDS), L, RC.MAX_PTS, device))
    cap = len(log["final"]["local_points"]) + 3
    assert b.d.update_reference(c.frame, c.frame_t, cap) == f.d.update_reference(c.frame, c.frame_t, cap)
    assert b.d.observations(c.obs_ids) == f.d.observations(c.obs_ids)
