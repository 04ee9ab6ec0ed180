"""The raw C ABI of the grid-window searches over the cases of tests/hostile_windows.py: host-kind calls on numpy arrays, device-kind calls on hipMalloc'ed
copies (gpu_common.DevBuf).  Results come back in the shape of the definition's (hostile_windows.run)."""
import ctypes as C

import numpy as np

import hostile_windows as H
from newpoints_pack import Mem


class Call:
    """one case prepared for one memory kind: enqueue() makes the call (a device-kind call only enqueues), read() -> dict like the definition's"""

    def __init__(self, pkg, G, c, device):
        cap = pkg._capi
        F, P, rule = c["frame"], c["probes"], c["rule"]
        self.pkg, self.c, self.device = pkg, c, device
        self.np, self.nf = len(P["cam"]), len(F["keys"])
        self.mem = mem = Mem(G, device)
        n, nf = self.np, self.nf
        self.asg = mem.out(F["assigned"].copy())
        self.frame = cap.FrameView(mem.p(F["keys"]), mem.p(F["desc"]), mem.p(F["mask"]), mem.p(F["cam"]), self.asg[0], nf, F["desc"].shape[1], len(F["width"]),
                                   mem.p(F["width"]), mem.p(F["height"]), mem.p(F["scales"]), len(F["scales"]))
        self.match, self.nm = mem.out(np.full(max(n, 1), -7, np.int32)), mem.out(np.full(1, -7, np.int32))
        self.acc = self.dist = None
        if rule == 0:
            self.probes = cap.ProjectionSet(mem.p(P["x"]), mem.p(P["y"]), mem.p(P["view_cos"]), mem.p(P["level"]), mem.p(P["cam"]), mem.p(P["desc"]), mem.p(P["mask"]), n,
                                            P["desc"].shape[1])
        else:
            if rule == 3:
                self.acc = mem.out(np.full(max(n, 1), -7, np.int32))
            if rule in ("best", "best_taken"):
                self.dist = mem.out(np.full(max(n, 1), -7, np.int32))
            self.probes = cap.WindowProbes(mem.p(P["x"]), mem.p(P["y"]), mem.p(P["r"]), mem.p(P["lo"]), mem.p(P["hi"]), mem.p(P["cam"]), mem.p(P["desc"]), mem.p(P["mask"]), n,
                                           P["desc"].shape[1], self.acc[0] if self.acc else None)

    def enqueue(self, ctx):
        L, c, kind = self.pkg.lib(), self.c, 1 if self.device else 0
        rule = c["rule"]
        if rule == 0:
            rc = L.mcs_search_by_projection(ctx.h, C.byref(self.probes), C.byref(self.frame), c["th"], c["nnratio"], c["dim"], kind, self.match[0], self.nm[0])
        elif rule in ("best", "best_taken"):
            rc = L.mcs_window_best(ctx.h, C.byref(self.probes), C.byref(self.frame), c["max_dist"], int(rule == "best_taken"), c["dim"], kind, self.match[0], self.dist[0],
                                   self.nm[0])
        else:
            rc = L.mcs_window_match(ctx.h, C.byref(self.probes), C.byref(self.frame), rule, c["nnratio"], c["dim"], kind, self.match[0], self.nm[0])
        self.pkg.check(rc)

    def read(self):
        n = self.np
        r = dict(match=self.match[1]()[:n].copy(), nmatches=int(self.nm[1]()[0]), assigned=self.asg[1]()[:self.nf].copy())
        if self.acc:
            r["accepted"] = self.acc[1]()[:n].copy()
        if self.dist:
            r["dist"] = self.dist[1]()[:n].copy()
        return r


def run(pkg, G, ctx, c, device):
    call = Call(pkg, G, c, device)
    call.enqueue(ctx)
    if device:
        ctx.synchronize()
    return call.read()


def compare(got, want, where):
    """every field the call gives, bit for bit"""
    for k, v in got.items():
        w = want[k]
        assert np.array_equal(np.asarray(v), np.asarray(w)), (where, k, np.flatnonzero(np.asarray(v) != np.asarray(w))[:8].tolist() if np.ndim(v) else (v, w))


def window_search_frames(pkg, G, ctx, c, device):
    """a rule 1 case whose probes are keypoints, through mcs_window_search_frames -> dict(match, nmatches) in the probes' terms"""
    cap = pkg._capi
    F, P = c["frame"], c["probes"]
    n, nf = len(P["cam"]), len(F["keys"])
    mem = Mem(G, device)
    k1 = np.zeros(n, H.KP_DTYPE)
    k1["x"], k1["y"] = P["x"].astype(np.float32), P["y"].astype(np.float32)
    k1["octave"] = np.arange(n) % 8
    tf = cap.TrackedFrame(mem.p(k1), mem.p(P["desc"]), mem.p(P["mask"]), mem.p(P["cam"]), mem.p(np.arange(n, dtype=np.int32)), None, n, P["desc"].shape[1])
    tab = cap.PointTable(mem.p(np.zeros((max(n, 1), 3))), mem.p(np.zeros(max(n, 1), np.uint8)), n)
    fv = cap.FrameView(mem.p(F["keys"]), mem.p(F["desc"]), mem.p(F["mask"]), mem.p(F["cam"]), None, nf, F["desc"].shape[1], len(F["width"]), mem.p(F["width"]),
                       mem.p(F["height"]), mem.p(F["scales"]), len(F["scales"]))
    m21, nm = mem.out(np.full(max(nf, 1), -7, np.int32)), mem.out(np.full(1, -7, np.int32))
    pkg.check(pkg.lib().mcs_window_search_frames(ctx.h, C.byref(tf), C.byref(tab), C.byref(fv), int(P["r"][0]), 0, 2**31 - 1, c["nnratio"], c["dim"], 0, 1 if device else 0,
                                                 m21[0], None, nm[0]))
    if device:
        ctx.synchronize()
    m21v = m21[1]()[:nf]
    match = np.full(n, -1, np.int32)
    match[m21v[m21v >= 0]] = np.flatnonzero(m21v >= 0)
    return dict(match=match, nmatches=int(nm[1]()[0]), assigned=(m21v >= 0).astype(np.uint8))


def keypoint_probes(c):
    """can mcs_window_search_frames express this case?  Centres that are floats, one integer radius, no level check, nothing taken on entry."""
    P = c["probes"]
    if c["rule"] != 1 or len(P["cam"]) == 0 or c["frame"]["assigned"].any() or not (np.all(P["lo"] == -1) and np.all(P["hi"] == -1)):
        return False
    r = P["r"]
    if not (np.all(r == r[0]) and np.isfinite(r[0]) and float(r[0]) == int(r[0]) and abs(r[0]) < 2**31):
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        return np.array_equal(P["x"].astype(np.float32).astype(np.float64), P["x"]) and np.array_equal(P["y"].astype(np.float32).astype(np.float64), P["y"])


# ---------------------------------------------------------------------------------------------- the slot form of rule 0
LP_BAD, LP_SEEN = 1, 2


def slot_scene(c, nr, rig, fresh_pos, rng, next_above=True):
    """A rule 0 case as the scene of mcs_search_local_points (frustum_pack.Call) with nr cameras: one MCS_LP_SEEN point per probe whose slot of the LAST camera
    holds the probe exactly as the caller prescribes it; the point's other slots are idle (not in view, NaN projections, level 1000); bad points whose slots
    claim to be in view with the same garbage lie in between, and one fresh point at the end brings n_to_match above 0 (the search runs only then).
    The frame's features move to the last camera.  -> (scene, slot_of_probe [np])"""
    P, F = c["probes"], c["frame"]
    n_probe, dim = len(P["cam"]), c["dim"]
    kinds = []
    for p in range(n_probe):
        if p % 3 == 1:
            kinds.append(-1 if p % 2 else -2)
        kinds.append(p)
    kinds.append(-3)
    n = len(kinds)
    cam = nr - 1
    st = dict(in_view=np.zeros((n, nr), np.uint8), proj_x=np.full((n, nr), np.nan), proj_y=np.full((n, nr), np.nan), level=np.full((n, nr), 1000, np.int32),
              view_cos=np.full((n, nr), np.nan))
    flags = np.full(n, LP_SEEN, np.uint8)
    desc = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    vcs = [0.5, 0.998, float("nan"), 0.9999 if next_above else 0.5, 0.998, float(np.nextafter(0.998, 1.0)) if next_above else 0.998]
    slot = np.zeros(n_probe, np.int64)
    for i, k in enumerate(kinds):
        if k >= 0:
            st["in_view"][i, cam], st["proj_x"][i, cam], st["proj_y"][i, cam], st["level"][i, cam] = 1, P["x"][k], P["y"][k], P["level"][k]
            st["view_cos"][i, cam] = vcs[k % len(vcs)]
            desc[i] = P["desc"][k, :dim]
            slot[k] = i * nr + cam
        elif k == -3:
            flags[i] = 0
            st["level"][i], st["proj_x"][i], st["proj_y"][i], st["view_cos"][i] = 0, 0.0, 0.0, 0.0
        else:
            flags[i] = LP_BAD if k == -1 else LP_BAD | LP_SEEN
            st["in_view"][i] = 1
    pos = np.zeros((n, 3))
    pos[-1] = fresh_pos
    pts = dict(pos=pos, normal=np.tile([0.0, 0.0, 1.0], (n, 1)), min_dist=np.full(n, 0.01), max_dist=np.full(n, 1000.0), flags=flags)
    F2 = dict(F, cam=np.full(len(F["keys"]), cam, np.int32), width=np.full(nr, int(F["width"][0]), np.int32), height=np.full(nr, int(F["height"][0]), np.int32),
              n=len(F["keys"]))
    return (pts, rig, st, desc, None, F2, F["assigned"].copy()), slot


def compacted(c, scene, state):
    """the probe list SearchByProjection visits on `state` (map point, then camera; bad points skipped; a level outside the pyramid is not searched) as a rule 0
    case over the scene's frame -> (case, slots [n])"""
    pts, rig, st, desc, mask, F2, asg = scene
    n, nr = state["in_view"].shape
    nl = len(F2["scales"])
    sl = [(i, k) for i in range(n) if not (pts["flags"][i] & LP_BAD) for k in range(nr) if state["in_view"][i, k] and 0 <= state["level"][i, k] < nl]
    ii, kk = np.array([s[0] for s in sl], np.int64), np.array([s[1] for s in sl], np.int64)
    Pc = H.probes0(state["proj_x"][ii, kk], state["proj_y"][ii, kk], state["view_cos"][ii, kk], state["level"][ii, kk], desc[ii], cam=kk.astype(np.int32))
    F3 = {k: v for k, v in F2.items() if k != "n"}
    F3["assigned"] = asg.copy()
    return H.case(c["name"] + "/slots", c["group"], 0, F3, Pc, c["nnratio"], c["th"], None, c["dim"]), ii * nr + kk
