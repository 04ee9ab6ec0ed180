"""(MI355X) the frame-to-frame search of cTracking::TrackWithMotionModel, cORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th)
(src/cORBmatcher.cpp:1990-2118), on the synthetic pairs of tests/lastframe_scene.py at 3 x 1000 and 8 x 2000 features per frame:
  (a)  ONE device-kind call, mcs_search_last_frame: frames and point tables resident, the call enqueues;
  (a') the same call in host kind;
  (b)  the composed route in device kind, as a careful caller would write it: positions and cameras of the selected features in ONE upload ->
       mcs_world_to_cam -> projections and flags read back (one synchronisation, two copies) -> host loop that builds the probes -> the probe arrays packed
       into ONE upload -> mcs_window_match (which ends in a synchronisation) -> matches and count read back (two copies), inverted on the host -> one upload ->
       mcs_rotation_consistency -> result read back (one synchronisation, two copies).  Without the filter the route ends after the inversion;
  (c)  the composed route in host kind, as frontend.cORBmatcher.SearchByProjectionLast runs it today (tests/test_gpu_lastframe.py: composed()).
Timing: HIP events on the context's stream around each whole route; the stop event is synchronised, so host work inside a route counts.  Median, minimum
and maximum over --reps repetitions after --warm unmeasured ones; the in/out arrays are reset outside the timed window.
Checks: every route's result is compared with route (c) before it is timed (the same device arithmetic: bit for bit).  equals_oracle says whether that
result is also the CPU oracle's: a last-place atan difference may move a window edge at these sizes.
--kernels: per-kernel event times of (a) (mcs_ctx_enable_timing, a run of its own): track_probes, track_candidates, track_greedy, track_tail.
--window: the same for mcs_window_search_frames, without route (b)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("multicol-slam_amd")
import gpu_common as G            # noqa: E402
import lastframe_scene as LS      # noqa: E402
import test_gpu_lastframe as T    # noqa: E402


class Events:
    def __init__(self, stream):
        self.hip, self.stream = G.hip(), stream
        self.a, self.b = C.c_void_p(), C.c_void_p()
        self.hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.hip.hipEventSynchronize.argtypes = [C.c_void_p]
        self.hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        assert self.hip.hipEventCreate(C.byref(self.a)) == 0 and self.hip.hipEventCreate(C.byref(self.b)) == 0

    def time(self, fn):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0 and self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value


def median_ms(ev, prepare, fn, reps, warm):
    t = []
    for k in range(warm + reps):
        prepare()
        ms = ev.time(fn)
        if k >= warm:
            t.append(ms)
    return round(float(np.median(t)), 4), round(float(np.min(t)), 4), round(float(np.max(t)), 4)


def up(buf, arr):
    arr = np.ascontiguousarray(arr)
    if arr.nbytes:
        assert G.hip().hipMemcpy(buf.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes, 1) == 0


def sync():
    assert G.hip().hipDeviceSynchronize() == 0      # the context's stream does not synchronise with the blocking copy's


def down(buf, arr):
    if arr.nbytes:
        assert G.hip().hipMemcpy(arr.ctypes.data_as(C.c_void_p), buf.ptr, arr.nbytes, 2) == 0


def al(n):
    return (n + 255) // 256 * 256


class ComposedDevice:
    """route (b): the existing entry points in device kind with the host visits between them.  Every device buffer is allocated once; what goes up between
    two calls is packed into one buffer and sent with one copy, what comes down is read behind one synchronisation"""

    def __init__(self, env, S):
        cap = pkg._capi
        self.env, self.S, self.cap = env, S, cap
        La, Cu, rig = S["last"], S["cur"], S["rig"]
        nr, nl, nc, dim = Cu["nr"], La["n"], Cu["n"], S["dim"]
        D = G.DevBuf
        # the two packed uploads: [positions | cameras] and [x | y | radius | min level | max level | camera | descriptors | masks], pieces 256-byte aligned
        self.off1 = dict(pts3=0, pc=al(nl * 24))
        sizes = [("x", 8), ("y", 8), ("r", 8), ("lo", 4), ("hi", 4), ("cam", 4), ("dd", dim), ("mm", dim)]
        self.off2, at = {}, 0
        for k, b in sizes:
            self.off2[k] = at
            at += al(nl * b)
        self.host1, self.host2 = np.zeros(al(nl * 24) + al(nl * 4), np.uint8), np.zeros(at, np.uint8)
        self.d = dict(in1=D(self.host1), in2=D(self.host2), uv=D(np.zeros((nl, 2))), fl=D(np.zeros(nl, np.uint8)), match=D(np.zeros(nl, np.int32)),
                      nm=D(np.zeros(1, np.int32)), mcur=D(np.zeros(nc, np.int32)), rem=D(np.zeros(1, np.int32)), assigned=D(S["assigned"]), keys=D(Cu["keys"]),
                      desc=D(Cu["desc"]), mask=D(Cu["mask"]) if S["masks"] else None, fcam=D(Cu["cam"]), w=D(Cu["width"]), h=D(Cu["height"]),
                      sc=D(np.ascontiguousarray(Cu["scales"], np.float64)), lkeys=D(La["keys"]))
        self.Minv = np.ascontiguousarray(np.stack(rig["MtMc_inv"]).reshape(nr, 16))     # host values for either kind of mcs_world_to_cam, like the calibrations
        self.ocs = (cap.Ocam * nr)(*[cap.make_ocam(c) for c in rig["cams"]])
        self.masks = [D(m) for m in rig["masks"]]
        self.mp = (C.c_void_p * nr)(*[m.ptr.value for m in self.masks])
        self.good = LS.good(S) != 0

    def reset(self):
        up(self.d["assigned"], self.S["assigned"])

    @staticmethod
    def pack(host, off, parts):
        for k, a in parts:
            a = np.ascontiguousarray(a)
            host[off[k]:off[k] + a.nbytes] = a.view(np.uint8).reshape(-1)

    def run(self, ori):
        S, d, cap, L = self.S, self.d, self.cap, pkg.lib()
        ctx = self.env["ctx"]
        La, Cu, Tb = S["last"], S["cur"], S["pts"]
        nr, dim = Cu["nr"], S["dim"]
        at1 = lambda k: C.c_void_p(d["in1"].ptr.value + self.off1[k])      # noqa: E731
        at2 = lambda k: C.c_void_p(d["in2"].ptr.value + self.off2[k])      # noqa: E731
        sel = np.flatnonzero(self.good & (La["outlier"] == 0))                     # the host loop: NULL / bad / outlier
        self.pack(self.host1, self.off1, (("pts3", Tb["pos"][La["points"][sel]]), ("pc", La["cam"][sel].astype(np.int32))))
        up(d["in1"], self.host1)                                                   # upload 1
        pkg.check(L.mcs_world_to_cam(ctx.h, cap.np_ptr(self.Minv), self.ocs, nr, self.mp, at1("pts3"), at1("pc"), len(sel), cap.MEM_DEVICE, d["uv"].ptr, d["fl"].ptr))
        uv, fl = np.zeros((len(sel), 2)), np.zeros(len(sel), np.uint8)
        sync()
        down(d["uv"], uv)
        down(d["fl"], fl)
        ok = (fl & 1) != 0                                                         # ... / outside the mask
        rows = sel[ok]
        octv = La["keys"]["octave"][rows].astype(np.int32)
        n = len(rows)
        self.pack(self.host2, self.off2, (("x", uv[ok, 0]), ("y", uv[ok, 1]), ("r", LS.TH * np.asarray(Cu["scales"], np.float64)[octv]), ("lo", octv - 1),
                                          ("hi", octv + 1), ("cam", La["cam"][rows].astype(np.int32)), ("dd", La["desc"][rows]))
                  + ((("mm", La["mask"][rows]),) if S["masks"] else ()))
        up(d["in2"], self.host2)                                                   # upload 2
        pr = cap.WindowProbes(at2("x"), at2("y"), at2("r"), at2("lo"), at2("hi"), at2("cam"), at2("dd"), at2("mm") if S["masks"] else None, n, dim, None)
        fv = cap.FrameView(d["keys"].ptr, d["desc"].ptr, d["mask"].ptr if S["masks"] else None, d["fcam"].ptr, d["assigned"].ptr, Cu["n"], dim, nr, d["w"].ptr,
                           d["h"].ptr, d["sc"].ptr, len(Cu["scales"]))
        pkg.check(L.mcs_window_match(ctx.h, C.byref(pr), C.byref(fv), cap.WINDOW_BEST, 0.8, dim, cap.MEM_DEVICE, d["match"].ptr, d["nm"].ptr))
        match, nm = np.zeros(n, np.int32), np.zeros(1, np.int32)
        down(d["match"], match)                                                    # (the call has synchronised the stream)
        down(d["nm"], nm)
        mcur = np.full(Cu["n"], -1, np.int32)
        hit = match >= 0
        mcur[match[hit]] = rows[hit]                                               # the host inversion
        nmatches = int(nm[0])
        if ori:
            up(d["mcur"], mcur)                                                    # upload 3
            off, sz = cap.KP_DTYPE.fields["angle"][1], cap.KP_DTYPE.itemsize
            pkg.check(L.mcs_rotation_consistency(ctx.h, 0, C.c_void_p(d["keys"].ptr.value + off), sz, C.c_void_p(d["lkeys"].ptr.value + off), sz, None, d["mcur"].ptr,
                                                 Cu["n"], La["n"], 1, cap.MEM_DEVICE, d["rem"].ptr))
            rem = np.zeros(1, np.int32)
            sync()
            down(d["mcur"], mcur)
            down(d["rem"], rem)
            nmatches -= int(rem[0])
        self.out = (mcur, nmatches)


def run(env, nr_cams, nfeat, reps, warm, kernels, window, ori):
    cap, L, ctx = pkg._capi, pkg.lib(), env["ctx"]
    S = LS.make_pair(seed=100 + nr_cams, nr_cams=nr_cams, nfeat=nfeat, dim=32, masks=True, window=window)
    want = T.composed(env, S, ori)      # the same device arithmetic as the one call: must agree bit for bit
    oracle = T.expected(S, ori)
    res = dict(equals_oracle=bool(oracle["nmatches"] == want["nmatches"] and np.array_equal(oracle["match"], want["match"])),
               call="mcs_window_search_frames" if window else "mcs_search_last_frame", cams=nr_cams, features=S["cur"]["n"], tracked=S["last"]["n"],
               nmatches=want["nmatches"], check_orientation=ori, reps=reps, warm=warm)
    # (a)
    call = T.Call(env, S, True)

    def reset_a():
        up(call.assigned, S["assigned"])
        up(call.cur_points, S["cur_points"])
    pkg.check(call.run(ori))
    T.same(call.read(), want, "one call")
    stream = C.c_void_p()
    pkg.check(L.mcs_ctx_result_stream(ctx.h, C.byref(stream)))
    ev = Events(stream)
    res["one_call_device_ms"] = median_ms(ev, reset_a, lambda: pkg.check(call.run(ori)), reps, warm)
    if kernels:
        pkg.check(L.mcs_ctx_enable_timing(ctx.h, 1))
        reset_a()
        pkg.check(call.run(ori))
        ctx.synchronize()
        for name in ("track_probes", "track_candidates", "track_greedy", "track_tail"):
            ms = C.c_float()
            pkg.check(L.mcs_ctx_kernel_ms(ctx.h, name.encode(), C.byref(ms)))
            res[name + "_ms"] = round(ms.value, 4)
        pkg.check(L.mcs_ctx_enable_timing(ctx.h, 0))
    # (a') the same call in host kind
    hc = T.Call(env, S, False)

    def reset_h():
        hc.assigned[:] = np.resize(S["assigned"], hc.assigned.shape)
        hc.cur_points[:] = np.resize(S["cur_points"], hc.cur_points.shape)
    res["one_call_host_ms"] = median_ms(ev, reset_h, lambda: pkg.check(hc.run(ori)), reps, warm)
    if not window:
        # (b)
        cd = ComposedDevice(env, S)
        cd.reset()
        cd.run(ori)
        assert np.array_equal(cd.out[0], want["match"]) and cd.out[1] == want["nmatches"], "composed route, device kind"
        res["composed_device_ms"] = median_ms(ev, cd.reset, lambda: cd.run(ori), reps, warm)
    # (c)
    T.same(T.composed(env, S, ori), want, "composed route, host kind")
    res["composed_host_ms"] = median_ms(ev, lambda: None, lambda: T.composed(env, S, ori), reps, warm)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="per-kernel event times of the one-call device-kind form (one extra call per shape)")
    ap.add_argument("--window", action="store_true", help="mcs_window_search_frames instead")
    ap.add_argument("--check-orientation", type=int, default=0)
    a = ap.parse_args()
    e = dict(G=G, pkg=pkg, ctx=G.ctx())
    for nr_cams, nfeat in [(3, 1000)] + ([] if a.small_only else [(8, 2000)]):
        print(json.dumps(run(e, nr_cams, nfeat, a.reps, a.warm, a.kernels, a.window, a.check_orientation)), flush=True)
