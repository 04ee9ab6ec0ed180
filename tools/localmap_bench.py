"""(MI355X) the search step of cTracking::TrackLocalMap (SearchReferencePointsInFrustum from src/cTracking.cpp:978 on) as ONE call, mcs_search_local_points:
  (a) device-kind: inputs and outputs resident, the call enqueues and the timing ends in a synchronisation;
  (b) host-kind: everything staged up and down by the call;
  (c) the route through the entry points the library had before: host-kind mcs_world_to_cam for every (point, camera), the frustum arithmetic of
      cMultiFrame::isInFrustum in numpy on the host, the in-view slots compacted, host-kind mcs_search_by_projection.
Shapes: 3 cameras x 1000 features against 2 000 and 8 000 local points, 8 cameras x 2000 features against 20 000.  Medians over warm calls; the in/out arrays
are reset outside the timed window.  Every timed output is checked against tests/frustum_model.py.  Per-kernel times of (a): --kernels (event timing on the
context, a run of its own), or `rocprofv3 --kernel-trace --stats -- python tools/localmap_bench.py`."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("multicol-slam_amd")
import gpu_common as G      # noqa: E402
import frustum_model as M   # noqa: E402
import frustum_pack as P    # noqa: E402


def median_ms(prepare, fn, reps, warm=3):
    t = []
    for k in range(warm + reps):
        prepare()
        t0 = time.perf_counter()
        fn()
        if k >= warm:
            t.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(t))


def numpy_frustum(pts, rig, scales, st, uv, inm):
    """isInFrustum (src/cMultiFrame.cpp:230-267) for all slots at once, the statements in the reference's order -> fields updated in place, fresh [n][nr]"""
    n, nr = inm.shape
    live = (pts["flags"] == 0)[:, None]
    T = np.stack(rig["MtMc"])[:, :3, 3]                                   # [nr][3]
    PO = pts["pos"][:, None, :] - T[None, :, :]                           # [n][nr][3]
    s = np.zeros((n, nr))
    for k in range(3):
        s = s + PO[:, :, k] * PO[:, :, k]
    with np.errstate(all="ignore"):
        dist = np.sqrt(s)
        ok = inm & ~((dist < pts["min_dist"][:, None]) | (dist > pts["max_dist"][:, None])) & live
        d = np.zeros((n, nr))
        for k in range(3):
            d = d + PO[:, :, k] * pts["normal"][:, None, k]
        vcos = d / dist
        ratio = dist / pts["min_dist"][:, None]
    lvl = np.where(np.isnan(ratio), 0, np.minimum(np.searchsorted(scales, np.where(np.isnan(ratio), 0.0, ratio), side="left"), len(scales) - 1)).astype(np.int32)
    st["in_view"][live[:, 0]] = ok[live[:, 0]]
    st["proj_x"][ok], st["proj_y"][ok], st["level"][ok], st["view_cos"][ok] = uv[:, :, 0][ok], uv[:, :, 1][ok], lvl[ok], vcos[ok]
    return ok.astype(np.uint8)


def run(ctx, nr_cams, per_cam, npoints, reps, kernels):
    cap, L = pkg._capi, pkg.lib()
    fr = M.oracle_frames(32, nr_cams, per_cam)
    sc = M.make_scene(1000 + npoints, npoints, 32, nr_cams, per_cam, True, frames=fr)
    pts, rig, st, desc, mask, F, asg = sc
    want = M.search_local_points(pts, rig, st, desc, mask, F, asg)
    n, nr = npoints, nr_cams
    res = dict(cams=nr, features=F["n"], points=n, slots=n * nr, n_to_match=int(want["n_to_match"]), searched=len(M.searched_slots(pts, want["state"])),
               nmatches=int(want["nmatches"]))

    def check(got, where):
        P.compare_fields(got, want, where)
        assert np.array_equal(got["match"], want["match"]) and got["nmatches"] == want["nmatches"] and np.array_equal(got["assigned"], want["assigned"]), where

    # (a), (b)
    for device in (True, False):
        call = P.Call(pkg, G, sc, device)

        def go():
            pkg.check(call.run(ctx, reset=False))
            ctx.synchronize()
        call.reset()
        go()
        check(call.read(), "device" if device else "host")
        res["device_ms" if device else "host_ms"] = round(median_ms(call.reset, go, reps), 3)
        if device and kernels:
            pkg.check(L.mcs_ctx_enable_timing(ctx.h, 1))
            call.reset()
            go()
            for name in ("frustum", "lm_candidates", "lm_greedy"):
                ms = C.c_float()
                pkg.check(L.mcs_ctx_kernel_ms(ctx.h, name.encode(), C.byref(ms)))
                res[name + "_ms"] = round(ms.value, 3)
            pkg.check(L.mcs_ctx_enable_timing(ctx.h, 0))

    # (c) the route of the earlier entry points
    p = cap.np_ptr
    MtMcInv = np.ascontiguousarray(np.stack(rig["MtMc_inv"]).reshape(nr, 16))
    ocs = (cap.Ocam * nr)(*[pkg.make_ocam(c) for c in rig["cams"]])
    mkeep = [np.ascontiguousarray(m, np.uint8) for m in rig["masks"]]
    mp = (C.c_void_p * nr)(*[m.ctypes.data for m in mkeep])
    pos_rep = np.ascontiguousarray(np.repeat(pts["pos"], nr, axis=0))
    pcam = np.ascontiguousarray(np.tile(np.arange(nr, dtype=np.int32), n))
    scales = np.ascontiguousarray(F["scales"], np.float64)
    w, h = np.ascontiguousarray(F["width"], np.int32), np.ascontiguousarray(F["height"], np.int32)
    notbad = ((pts["flags"] & M.LP_BAD) == 0)[:, None]
    box = {}

    def prepare():
        box["st"] = M.copy_state(st)
        box["asg"] = np.ascontiguousarray(asg, np.uint8).copy()

    def route():
        s2, a2 = box["st"], box["asg"]
        uv, fl = np.zeros((n * nr, 2)), np.zeros(n * nr, np.uint8)
        pkg.check(L.mcs_world_to_cam(ctx.h, p(MtMcInv), ocs, nr, mp, p(pos_rep), p(pcam), n * nr, cap.MEM_HOST, p(uv), p(fl)))
        fresh = numpy_frustum(pts, rig, scales, s2, uv.reshape(n, nr, 2), (fl & 1).astype(bool).reshape(n, nr))
        match = np.full((n, nr), -1, np.int32)
        nm = np.zeros(1, np.int32)
        if fresh.sum() > 0:
            ii, cc = np.nonzero((s2["in_view"] != 0) & notbad)
            px, py, vc = (np.ascontiguousarray(s2[k][ii, cc]) for k in ("proj_x", "proj_y", "view_cos"))
            lv, pc = np.ascontiguousarray(s2["level"][ii, cc], np.int32), np.ascontiguousarray(cc, np.int32)
            dd, mm = np.ascontiguousarray(desc[ii]), np.ascontiguousarray(mask[ii])
            ps = cap.ProjectionSet(p(px), p(py), p(vc), p(lv), p(pc), p(dd), p(mm), len(ii), 32)
            fv = cap.FrameView(p(F["keys"]), p(F["desc"]), p(F["mask"]), p(F["cam"]), p(a2), F["n"], 32, nr, p(w), p(h), p(scales), len(scales))
            m = np.full(len(ii), -1, np.int32)
            pkg.check(L.mcs_search_by_projection(ctx.h, C.byref(ps), C.byref(fv), 3.0, 0.8, 32, cap.MEM_HOST, p(m), p(nm)))
            match[ii, cc] = m
        box["out"] = dict(state=s2, visible_inc=fresh.sum(axis=1).astype(np.int32), n_to_match=int(fresh.sum()), match=match, nmatches=int(nm[0]), assigned=a2)

    prepare()
    route()
    check(box["out"], "earlier entry points")
    res["earlier_route_ms"] = round(median_ms(prepare, route, reps), 3)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--kernels", action="store_true", help="per-kernel event times of the device-kind chain (one extra call per shape)")
    a = ap.parse_args()
    ctx = G.ctx()
    shapes = [(3, 1000, 2000), (3, 1000, 8000)] + ([] if a.small_only else [(8, 2000, 20000)])
    for nr_cams, per_cam, npoints in shapes:
        print(json.dumps(run(ctx, nr_cams, per_cam, npoints, a.reps, a.kernels)), flush=True)
