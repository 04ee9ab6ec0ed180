#!/usr/bin/env python3
"""Per-call time of mcs_pose_optimization on an MI355X (not part of any test; nothing is asserted: there is no earlier implementation to compare with).

Shapes: 1 problem x 300 / 3 000 / 16 000 edges and 64 problems x 3 000 edges, device kind (arrays resident, the call only enqueues; time per call of a
back-to-back series, one synchronisation at the end) and host kind (through the staging block, each call waits).  Next to each, mcs_world_to_cam over the same
points in the same kind: one projection per edge, the floor of ONE residual pass (an optimisation makes 2 passes per trial and a Jacobian pass per iteration).
Prints one JSON line per shape.  Scenes: tests/poseopt_model.lafida_like_scene (3 Lafida cameras, 8 % outliers)."""
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
import poseopt_scenes as S   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    pkg = importlib.import_module("multicol-slam_amd")
    FE = importlib.import_module("multicol-slam_amd.frontend")
    cap, L = pkg._capi, pkg.lib()
    ctx = pkg.Context(0)
    for ne, nb in ((300, 1), (3000, 1), (16000, 1), (3000, 64)):
        distinct = [S.scene(s, ne, 3, n_outliers=ne // 12) for s in range(min(nb, 4))]
        prs = [distinct[i % len(distinct)] for i in range(nb)]
        row = dict(edges=ne, problems=nb)
        for device in (True, False):
            mem = FE._DEVICE if device else FE._HOST
            p0, nr = prs[0], 3
            ocs = np.frombuffer((cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams]), np.uint8).copy()
            base = np.cumsum([0] + [len(p.pos) for p in prs])
            pos = np.concatenate([p.pos for p in prs])
            pose0 = np.array([p.pose0 for p in prs])
            g = {k: mem.put(v) for k, v in dict(pos=pos, Mc=p0.Mc_min, ocs=ocs, sig=p0.inv_sigma2, hub=np.ones(nb), pose=pose0.copy(), MtMc=np.zeros((nb, nr, 16)),
                                                inv=np.zeros((nb, nr, 16)), nin=np.zeros(nb, np.int32), share=np.zeros(nb), diag=np.zeros(nb, cap.POSE_DIAG_DTYPE)).items()}
            per = [dict(keys=mem.put(S.keys_of(p, cap)), cam=mem.put(p.cam), points=mem.put((p.points + b).astype(np.int32)), out=mem.put(np.zeros(p.n, np.uint8)))
                   for p, b in zip(prs, base)]
            fr = (cap.PoseFrame * nb)(*[cap.PoseFrame(mem.ptr(q["keys"]), mem.ptr(q["cam"]), mem.ptr(q["points"]), p.n) for q, p in zip(per, prs)])
            outs = (C.c_void_p * nb)(*[mem.ptr(q["out"]) for q in per])
            tab = cap.PointTable(mem.ptr(g["pos"]), None, len(pos))
            fresh = mem.put(pose0.copy())      # every repetition starts from the same pose: one small copy in front of the call
            nbytes = pose0.nbytes

            def reset():
                if device:
                    FE._hip().hipMemcpy(g["pose"].ptr, fresh.ptr, nbytes, 3)
                else:
                    g["pose"][:] = pose0

            def call():
                pkg.check(L.mcs_pose_optimization(ctx.h, nb, fr, C.byref(tab), mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(p0.inv_sigma2),
                                                  mem.ptr(g["hub"]), mem.kind, mem.ptr(g["pose"]), mem.ptr(g["MtMc"]), mem.ptr(g["inv"]), outs, mem.ptr(g["nin"]),
                                                  mem.ptr(g["share"]), mem.ptr(g["diag"])))
            # the floor: one projection per edge of the whole batch
            allp = np.concatenate([p.pos[p.points] for p in prs])
            allc = np.concatenate([p.cam for p in prs]).astype(np.int32)
            w = {k: mem.put(v) for k, v in dict(pts=allp, cam=allc, uv=np.zeros((len(allp), 2)), fl=np.zeros(len(allp), np.uint8)).items()}
            M = np.ascontiguousarray(np.zeros((nr, 16)) + np.eye(4).reshape(16))      # matrices and calibrations are host values of that call for either kind
            host_ocs = (cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams])

            def floor():
                pkg.check(L.mcs_world_to_cam(ctx.h, cap.np_ptr(M), host_ocs, nr, None, mem.ptr(w["pts"]), mem.ptr(w["cam"]), len(allp), mem.kind, mem.ptr(w["uv"]),
                                             mem.ptr(w["fl"])))
            for name, fn, pre in (("pose_optimization", call, reset), ("world_to_cam", floor, lambda: None)):
                pre(); fn(); ctx.synchronize()
                ts = []
                for _ in range(a.reps):
                    pre()
                    ctx.synchronize()
                    t = time.perf_counter()
                    fn()
                    ctx.synchronize()
                    ts.append(time.perf_counter() - t)
                row["%s_%s_ms" % (name, "device" if device else "host")] = round(1e3 * float(np.median(ts)), 4)
            if device:
                d = mem.read(g["diag"])
                row["iters"], row["trials"] = d["iters"].sum(axis=1).tolist()[:4], d["trials"].sum(axis=(1, 2)).tolist()[:4]
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
