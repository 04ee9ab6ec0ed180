#!/usr/bin/env python3
"""One SHA-256 per entry point and memory kind over every output byte of the calls that go through csrc/mcs_geom.h and csrc/mcs_lm.h, on the small scenes
the tests already have (tests/poseopt_scenes.py, sim3opt_scenes.py, lba_scenes.py, essgraph_scenes.py, the hostile tables for new points, Sim3 and windows,
tests/frustum_pack.py, tests/lastframe_scene.py).  Nothing is asserted:
the lines of two libraries (MCS_HIP_LIB selects one) are compared with diff.  Equal lines from two processes of one library show the outputs do not depend on
the process; equal lines from two libraries show a refactor of the shared arithmetic changed no output bit.  One process, a few seconds on an MI355X."""
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_common as G   # noqa: E402
import essgraph_scenes as ES   # noqa: E402
import frustum_model as FM   # noqa: E402
import frustum_pack   # noqa: E402
import hostile_newpoints as HN   # noqa: E402
import hostile_sim3 as HS   # noqa: E402
import hostile_windows as HW   # noqa: E402
import lastframe_scene as LS   # noqa: E402
import lba_scenes as LBS   # noqa: E402
import newpoints_pack as NP   # noqa: E402
import poseopt_scenes as PS   # noqa: E402
import sim3opt_scenes as SS   # noqa: E402
import window_pack as WP   # noqa: E402
from test_gpu_lastframe import Call as TrackCall   # noqa: E402
from test_gpu_sim3 import Batch   # noqa: E402

pkg = G.mcs
KINDS = ((False, "host"), (True, "device"))


def feed(h, v):
    """every byte of every array, in a fixed order"""
    if isinstance(v, dict):
        for k in sorted(v):
            h.update(str(k).encode())
            feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        for x in v:
            feed(h, x)
    elif v is not None:
        a = np.ascontiguousarray(v)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())


def line(name, kind, outputs):
    h = hashlib.sha256()
    feed(h, outputs)
    print("%-28s %-6s %s" % (name, kind, h.hexdigest()), flush=True)


def world_to_cam(ctx):
    """the Lafida rig with its masks, seeded points and the corners of the branch table: the axis, z = +-0, a NaN"""
    cams = G.cams3()
    rig = FM.make_rig(cams, 0, with_masks=True, synth=G.synth)
    rng = np.random.default_rng(3)
    pts = np.concatenate([rng.normal(0, 3.0, (2000, 3)), [[0.0, 0.0, 2.0], [1.0, 1.0, 0.0], [1.0, 1.0, -0.0], [np.nan, 1.0, 1.0]]])
    n, nr = len(pts), len(cams)
    pc = (np.arange(n) % nr).astype(np.int32)
    M = np.ascontiguousarray(np.stack(rig["MtMc_inv"]).reshape(nr, 16))
    ocs = (pkg._capi.Ocam * nr)(*[pkg.make_ocam(c) for c in cams])
    masks = [np.ascontiguousarray(m) for m in rig["masks"]]
    L = pkg.lib()
    for device, kind in KINDS:
        if device:
            dm = [G.DevBuf(m) for m in masks]
            mp = (C.c_void_p * nr)(*[b.ptr.value for b in dm])
            dpts, dpc, duv, dfl = G.DevBuf(pts), G.DevBuf(pc), G.DevBuf(np.zeros((n, 2))), G.DevBuf(np.zeros(n, np.uint8))
            pkg.check(L.mcs_world_to_cam(ctx.h, M.ctypes.data, ocs, nr, mp, dpts.ptr, dpc.ptr, n, pkg.MEM_DEVICE, duv.ptr, dfl.ptr))
            line("mcs_world_to_cam", kind, [duv.read(), dfl.read()])
        else:
            mp = (C.c_void_p * nr)(*[m.ctypes.data for m in masks])
            uv, fl = np.zeros((n, 2)), np.zeros(n, np.uint8)
            pkg.check(L.mcs_world_to_cam(ctx.h, M.ctypes.data, ocs, nr, mp, pts.ctypes.data, pc.ctypes.data, n, pkg.MEM_HOST, uv.ctypes.data, fl.ctypes.data))
            line("mcs_world_to_cam", kind, [uv, fl])


def local_points(ctx):
    """tests/frustum_pack.py on a frustum scene, and the slot form of the hostile window cases on a three-camera rig"""
    sc = FM.make_scene(**FM.SCENES["2000"])
    rig = FM.make_rig([G.cams3()[k % 3] for k in range(3)], 0, with_masks=False)
    cand = np.random.default_rng(3).normal(0, 2.0, (200, 3))
    fresh = cand[np.flatnonzero(FM.project(rig, cand)[1].any(axis=1))[0]]
    names = ("cluster/identical/40/r0", "chain/r0", "order/zero/r0")
    hostile = [c for c in HW.cases() if c["name"] in names]
    for device, kind in KINDS:
        outs = []
        scenes = [(sc, {})] + [(WP.slot_scene(c, 3, rig, fresh, np.random.default_rng(7), next_above=not c["name"].startswith("chain"))[0],
                                dict(desc_masks=False, th=c["th"], nnratio=c["nnratio"])) for c in hostile]
        for scene, kw in scenes:
            call = frustum_pack.Call(pkg, G, scene, device, **kw)
            pkg.check(call.run(ctx))
            ctx.synchronize()
            outs.append(call.read())
        line("mcs_search_local_points", kind, outs)


def track(ctx):
    env = dict(G=G, pkg=pkg, ctx=ctx)
    for window, name in ((False, "mcs_search_last_frame"), (True, "mcs_window_search_frames")):
        for device, kind in KINDS:
            outs = []
            for scene in sorted(LS.SCENES):
                for ori in (0, 1):
                    c = TrackCall(env, LS.make_pair(window=window, **LS.SCENES[scene]), device)
                    pkg.check(c.run(ori))
                    ctx.synchronize()
                    outs.append(c.read())
            if window:
                outs += [WP.window_search_frames(pkg, G, ctx, c, device) for c in HW.cases()
                         if c["group"] in ("cluster", "chain", "order", "collision") and WP.keypoint_probes(c)]
            line(name, kind, outs)


def new_points(ctx):
    for device, kind in KINDS:
        outs = []
        for name in HN.camera_rigs():
            kf1, nb = HN.camera_scene(name)
            outs.append(NP.chain(pkg, ctx, G, kf1, nb, device=device))
        for name in ("n3", "n257"):
            if name in HN.median_calls():
                kf1, nb, _ = HN.median_calls()[name]
                outs.append(NP.chain(pkg, ctx, G, kf1, nb, device=device))
        kf1, nb = HN.rig_scene(HN.RIG_SIZES[0])
        outs.append(NP.chain(pkg, ctx, G, kf1, nb, device=device))
        line("mcs_create_new_map_points", kind, outs)
        cases = HN.exact_pairs()
        outs = [NP.triangulate(pkg, ctx, G, [(a, b) for _, a, b in cases], [np.array([0], np.int32)] * len(cases), device=device)]
        a, b, m12 = HN.threshold_pair()
        outs.append(NP.triangulate(pkg, ctx, G, [(a, b)], [m12], device=device))
        pairs, matches = HN.aba_pairs()
        outs.append(NP.triangulate(pkg, ctx, G, pairs, matches, device=device))
        line("mcs_triangulate_matches", kind, outs)


def sim3(ctx):
    """create / hypotheses / iterate / best; the entry points take host arrays only"""
    scenes = [HS.exact_scene(), HS.poison_scene(), HS.threshold_scene()] + [HS.projection_scene(n) for n in HS.projection_rigs()]
    hyp, rounds, best = [], [], []
    for sc in scenes:
        b = Batch(pkg, ctx, sc["cams"], sc["M_c"], sc["pairs"], sc["params"], sc["seed"], draws=sc["draws"])
        n, mx, _ = b.info()
        hyp.append([b.hypotheses(s, 0, min(int(mx[s]), 20)) for s in range(len(sc["pairs"])) if mx[s] > 0])
        b = Batch(pkg, ctx, sc["cams"], sc["M_c"], sc["pairs"], sc["params"], sc["seed"], draws=sc["draws"])
        rounds.append([[list(r) for r in b.iterate(k)] for k in (1, 4, 15)])
        ns, pp = len(sc["pairs"]), pkg.np_ptr
        R, t, s, T12 = np.full((ns, 9), -7.0), np.full((ns, 3), -7.0), np.full(ns, -7.0), np.full((ns, 16), -7.0)
        bi, it = np.full(ns, -7, np.int32), np.full(ns, -7, np.int32)
        pkg.check(b.L.mcs_sim3_best(b.h, pp(R), pp(t), pp(s), pp(T12), pp(bi), pp(it)))
        best.append([R, t, s, T12, bi, it])
    line("mcs_sim3_hypotheses", "host", hyp)
    line("mcs_sim3_iterate", "host", rounds)
    line("mcs_sim3_best", "host", best)


def pose_optimization(ctx):
    names = list(PS.SIZES) + list(PS.QUIRKS)
    for device, kind in KINDS:
        got = [PS.run_library(pkg, ctx, [PS.build(n)], device) for n in names]   # a call of its own each: the scenes' rigs differ
        assert all(isinstance(g, list) for g in got), got
        got = [g[0] for g in got]
        line("mcs_pose_optimization", kind, [[g[k] for k in ("pose", "MtMc", "MtMc_inv", "outlier", "diag", "n_inliers", "share")] for g in got])


def sim3_optimize(ctx):
    """the sizes up to the stride of a workgroup and a scene per path, a call of its own each; every output array and the diag record"""
    names = [n for n in SS.SIZES if SS.SIZES[n]["n"] <= SS.T + 1] + list(SS.PATHS)
    for device, kind in KINDS:
        got = [SS.run_library(pkg, ctx, [SS.build(n)], device) for n in names]
        assert all(isinstance(g, list) for g in got), got
        line("mcs_sim3_optimize", kind, [[g[0][k] for k in ("S12", "R12", "keep", "n_inliers", "diag")] for g in got])


def local_bundle_adjustment(ctx):
    names = ("pair", "window", "twice", "split")
    for device, kind in KINDS:
        got = [LBS.run_library(pkg, ctx, LBS.build(n), device) for n in names]
        assert all(isinstance(g, dict) for g in got), got
        line("mcs_local_bundle_adjustment", kind, [[g[k] for k in ("status", "kf_pose", "kf_t", "pos", "edge_state", "pt_state", "diag")] for g in got])


def optimize_essential_graph(ctx):
    names = ("chain6", "dup", "isolated", "fixed_mid")
    for device, kind in KINDS:
        got = [ES.run_library(pkg, ctx, ES.build(n), device) for n in names]
        assert all(isinstance(g, dict) for g in got), got
        line("mcs_optimize_essential_graph", kind, [[g[k] for k in ("status", "Scw_out", "pose", "kf_t", "pos", "diag")] for g in got])


def main():
    print("library: %s" % os.path.basename(os.path.dirname(os.path.abspath(pkg._capi.LIB_PATH))), file=sys.stderr)
    ctx = G.ctx()
    for part in (world_to_cam, local_points, track, new_points, sim3, pose_optimization, sim3_optimize, local_bundle_adjustment, optimize_essential_graph):
        part(ctx)


if __name__ == "__main__":
    main()
