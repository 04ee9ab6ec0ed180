"""The raw C ABI of mcs_frustum / mcs_search_local_points over the scenes of tests/frustum_model.py: host-kind calls on numpy arrays, device-kind calls on
hipMalloc'ed copies (gpu_common.DevBuf).  Results come back in the shape of the model's (frustum_model.search_local_points)."""
import ctypes as C

import numpy as np

from newpoints_pack import Mem


class Call:
    """one prepared call: arrays placed in host or device memory once, run() as often as wanted (the in/out arrays are reset from the scene each time unless
    reset=False), read() -> dict like the model's"""

    def __init__(self, pkg, G, scene, device, search=True, desc_masks=True, th=3.0, nnratio=0.8):
        cap = pkg._capi
        pts, rig, st, desc, mask, F, assigned = scene
        self.pkg, self.G, self.device, self.search, self.th, self.nnratio = pkg, G, device, search, th, nnratio
        self.n, self.nr, self.dim = len(pts["pos"]), len(rig["cams"]), desc.shape[1]
        n, nr = self.n, self.nr
        self.mem = mem = Mem(G, device)
        self.pts = cap.LocalPoints(mem.p(pts["pos"]), mem.p(pts["normal"]), mem.p(pts["min_dist"]), mem.p(pts["max_dist"]), mem.p(pts["flags"]), n)
        ocs = (cap.Ocam * nr)(*[pkg.make_ocam(c) for c in rig["cams"]])
        mp = None
        if rig["masks"] is not None:
            mp = mem.p(np.array([mem.p(m) or 0 for m in rig["masks"]], np.uint64))     # a None entry is a NULL pointer in the array
        self.rig = cap.RigView(mem.p(np.stack(rig["MtMc_inv"]).reshape(-1)), mem.p(np.stack(rig["MtMc"]).reshape(-1)), mem.p(np.frombuffer(ocs, np.uint8).copy()),
                               mp, nr)
        self.init = dict(in_view=st["in_view"].copy(), proj_x=st["proj_x"].copy(), proj_y=st["proj_y"].copy(), level=st["level"].copy(),
                         view_cos=st["view_cos"].copy(), assigned=np.ascontiguousarray(assigned, np.uint8).copy())
        self.io = {k: mem.out(v.copy()) for k, v in self.init.items()}
        self.state = cap.TrackState(*[self.io[k][0] for k in ("in_view", "proj_x", "proj_y", "level", "view_cos")])
        self.scales = mem.p(np.ascontiguousarray(F["scales"], np.float64))
        self.nlevels = len(F["scales"])
        self.out = dict(visible_inc=mem.out(np.full(max(n, 1), -9, np.int32)), n_to_match=mem.out(np.full(1, -9, np.int32)),
                        match=mem.out(np.full(max(n * nr, 1), -9, np.int32)), nmatches=mem.out(np.full(1, -9, np.int32)))
        self.desc, self.mask = mem.p(desc), mem.p(mask) if desc_masks else None
        self.frame = cap.FrameView(mem.p(F["keys"]), mem.p(F["desc"]), mem.p(F["mask"]) if desc_masks else None, mem.p(F["cam"]), self.io["assigned"][0], F["n"],
                                   F["desc"].shape[1], nr, mem.p(F["width"]), mem.p(F["height"]), self.scales, self.nlevels)

    def reset(self):
        for k, v in self.init.items():
            ptr = self.io[k][0]
            if self.device:
                if v.nbytes:
                    assert self.G.hip().hipMemcpy(C.c_void_p(ptr), v.ctypes.data_as(C.c_void_p), v.nbytes, 1) == 0
            else:
                C.memmove(ptr, v.ctypes.data, v.nbytes)

    def run(self, ctx, reset=True):
        L, kind = self.pkg.lib(), 1 if self.device else 0
        if reset:
            self.reset()
        if self.search:
            return L.mcs_search_local_points(ctx.h, C.byref(self.pts), C.byref(self.rig), C.byref(self.state), self.desc, self.mask, self.dim, C.byref(self.frame),
                                             self.th, self.nnratio, self.dim, kind, self.out["match"][0], self.out["nmatches"][0], self.out["n_to_match"][0],
                                             self.out["visible_inc"][0])
        return L.mcs_frustum(ctx.h, C.byref(self.pts), C.byref(self.rig), self.scales, self.nlevels, C.byref(self.state), kind, self.out["visible_inc"][0],
                             self.out["n_to_match"][0])

    def read(self):
        n, nr = self.n, self.nr
        st = {k: self.io[k][1]().reshape(n, nr).copy() for k in ("in_view", "proj_x", "proj_y", "level", "view_cos")}
        r = dict(state=st, visible_inc=self.out["visible_inc"][1]()[:n].copy(), n_to_match=int(self.out["n_to_match"][1]()[0]))
        if self.search:
            r.update(match=self.out["match"][1]()[:n * nr].reshape(n, nr).copy(), nmatches=int(self.out["nmatches"][1]()[0]), assigned=self.io["assigned"][1]().copy())
        return r


def same_doubles(a, b):
    """bit-equal, except that any NaN equals any NaN (0 / 0 is -nan on x86 and +nan on the device: the payload carries nothing)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def compare_fields(got, want, where=""):
    """the issue's rule: in_view, level, view_cos, untouched fields, visible_inc and n_to_match bit-equal; proj_x / proj_y as test_world_to_cam_matches_oracle
    compares uv (atan comes from ocml on the device and from glibc in the model): atol 1e-9 px, more than 95 % bit-equal, identical finiteness"""
    g, w = got["state"], want["state"]
    assert np.array_equal(g["in_view"], w["in_view"]), where
    assert np.array_equal(g["level"], w["level"]), where
    assert same_doubles(g["view_cos"], w["view_cos"]), where
    assert np.array_equal(got["visible_inc"], want["visible_inc"]) and got["n_to_match"] == want["n_to_match"], where
    fresh = want["fresh"].astype(bool)
    for k in ("proj_x", "proj_y"):
        assert same_doubles(g[k][~fresh], w[k][~fresh]), (where, k)   # rejected and skipped slots: untouched
        a, b = g[k][fresh], w[k][fresh]
        fin = np.isfinite(b)
        assert np.array_equal(np.isfinite(a), fin), (where, k)
        if fin.any():
            assert np.allclose(a[fin], b[fin], rtol=0, atol=1e-9), (where, k, float(np.abs(a[fin] - b[fin]).max()))
            assert (a[fin] == b[fin]).mean() > 0.95, (where, k, float((a[fin] == b[fin]).mean()))
