#!/usr/bin/env python3
"""Per-call time of mcs_sim3_optimize on an MI355X (not part of any test; nothing is asserted: there is no earlier implementation to compare with).

Shapes: 1 problem x 100, 1 x 1000 and 16 x 300 correspondences (two edges each), device kind (arrays resident, the call only enqueues) and host kind (through
the staging block), the median of --reps synchronised calls.  Next to each, as the scale, mcs_pose_optimization over the same number of problems with as many
edges (2 per correspondence) in the same kind.  Prints one JSON line per shape.  Scenes: tests/sim3opt_scenes.scene and tests/poseopt_scenes.scene (3 Lafida
cameras, 8 % outliers, the default Huber bounds)."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import poseopt_scenes as PS   # noqa: E402
import sim3opt_scenes as S    # noqa: E402


def timed(ctx, fn, pre, reps):
    pre(); fn(); ctx.synchronize()
    ts = []
    for _ in range(reps):
        pre()
        ctx.synchronize()
        t = time.perf_counter()
        fn()
        ctx.synchronize()
        ts.append(time.perf_counter() - t)
    return round(1e3 * float(np.median(ts)), 4)


def sim3_call(pkg, FE, ctx, prs, device):
    cap, L = pkg._capi, pkg.lib()
    mem = FE._DEVICE if device else FE._HOST
    nb, p0 = len(prs), prs[0]
    nr = len(p0.Mc)
    ocs = np.frombuffer((cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams]), np.uint8).copy()
    g = dict(Mc=p0.Mc.reshape(nr, 16), ocs=ocs, Mt=np.array([p.Mt_inv for p in prs]).reshape(nb, 32), std=np.array([p.std_sim for p in prs]),
             R=np.array([p.R12 for p in prs]).reshape(nb, 9), t=np.array([p.t12 for p in prs]).reshape(nb, 3), s=np.array([p.s12 for p in prs]), S=np.zeros((nb, 8)),
             Ro=np.zeros((nb, 9)), nin=np.zeros(nb, np.int32), diag=np.zeros(nb, cap.SIM3OPT_DIAG_DTYPE))
    g = {k: mem.put(np.ascontiguousarray(v)) for k, v in g.items()}
    per = [dict(Xw=mem.put(p.Xw.reshape(-1)), cam=mem.put(p.cam.astype(np.int32).reshape(-1)), obs=mem.put(p.obs.reshape(-1)), w=mem.put(p.w.reshape(-1)),
                keep=mem.put(np.zeros(p.n, np.uint8))) for p in prs]
    pr = (cap.Sim3OptProblem * nb)(*[cap.Sim3OptProblem(mem.ptr(q["Xw"]), mem.ptr(q["cam"]), mem.ptr(q["obs"]), mem.ptr(q["w"]), p.n) for q, p in zip(per, prs)])
    outs = (C.c_void_p * nb)(*[mem.ptr(q["keep"]) for q in per])

    def call():   # the inputs are not written: every repetition starts from the same estimate
        pkg.check(L.mcs_sim3_optimize(ctx.h, nb, pr, mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["Mt"]), mem.ptr(g["std"]), mem.ptr(g["R"]), mem.ptr(g["t"]),
                                      mem.ptr(g["s"]), mem.kind, mem.ptr(g["S"]), mem.ptr(g["Ro"]), outs, mem.ptr(g["nin"]), mem.ptr(g["diag"])))
    return call, lambda: mem.read(g["diag"]), (g, per, pr, outs)


def pose_call(pkg, FE, ctx, prs, device):
    cap, L = pkg._capi, pkg.lib()
    mem = FE._DEVICE if device else FE._HOST
    nb, p0, nr = len(prs), prs[0], 3
    ocs = np.frombuffer((cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams]), np.uint8).copy()
    base = np.cumsum([0] + [len(p.pos) for p in prs])
    pos = np.concatenate([p.pos for p in prs])
    pose0 = np.array([p.pose0 for p in prs])
    g = {k: mem.put(v) for k, v in dict(pos=pos, Mc=p0.Mc_min, ocs=ocs, sig=p0.inv_sigma2, hub=np.ones(nb), pose=pose0.copy(), MtMc=np.zeros((nb, nr, 16)),
                                        inv=np.zeros((nb, nr, 16)), nin=np.zeros(nb, np.int32), share=np.zeros(nb), diag=np.zeros(nb, cap.POSE_DIAG_DTYPE)).items()}
    per = [dict(keys=mem.put(PS.keys_of(p, cap)), cam=mem.put(p.cam), points=mem.put((p.points + b).astype(np.int32)), out=mem.put(np.zeros(p.n, np.uint8)))
           for p, b in zip(prs, base)]
    fr = (cap.PoseFrame * nb)(*[cap.PoseFrame(mem.ptr(q["keys"]), mem.ptr(q["cam"]), mem.ptr(q["points"]), p.n) for q, p in zip(per, prs)])
    outs = (C.c_void_p * nb)(*[mem.ptr(q["out"]) for q in per])
    tab = cap.PointTable(mem.ptr(g["pos"]), None, len(pos))
    fresh = mem.put(pose0.copy())

    def reset():   # every repetition starts from the same pose: one small copy in front of the call
        if device:
            FE._hip().hipMemcpy(g["pose"].ptr, fresh.ptr, pose0.nbytes, 3)
        else:
            g["pose"][:] = pose0

    def call():
        pkg.check(L.mcs_pose_optimization(ctx.h, nb, fr, C.byref(tab), mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(p0.inv_sigma2),
                                          mem.ptr(g["hub"]), mem.kind, mem.ptr(g["pose"]), mem.ptr(g["MtMc"]), mem.ptr(g["inv"]), outs, mem.ptr(g["nin"]),
                                          mem.ptr(g["share"]), mem.ptr(g["diag"])))
    return call, reset, (g, per, fr, outs, tab, fresh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    pkg = importlib.import_module("multicol-slam_amd")
    FE = importlib.import_module("multicol-slam_amd.frontend")
    ctx = pkg.Context(0)
    for nb, n in ((1, 100), (1, 1000), (16, 300)):
        distinct = [S.scene(s, n, 3, n_outliers=n // 12) for s in range(min(nb, 4))]
        prs = [distinct[i % len(distinct)] for i in range(nb)]
        pdistinct = [PS.scene(s, 2 * n, 3, n_outliers=n // 6) for s in range(min(nb, 4))]
        pprs = [pdistinct[i % len(pdistinct)] for i in range(nb)]
        row = dict(problems=nb, correspondences=n, edges=2 * n)
        for device in (True, False):
            kind = "device" if device else "host"
            call, diag, keep = sim3_call(pkg, FE, ctx, prs, device)
            row["sim3_optimize_%s_ms" % kind] = timed(ctx, call, lambda: None, a.reps)
            if device:
                d = diag()
                row["iters"], row["trials"] = d["iters"].sum(axis=1).tolist()[:4], d["trials"].sum(axis=(1, 2)).tolist()[:4]
            pcall, reset, pkeep = pose_call(pkg, FE, ctx, pprs, device)
            row["pose_optimization_%s_ms" % kind] = timed(ctx, pcall, reset, a.reps)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
