"""The scenes of the PoseOptimization tests (tests/test_poseopt_cpu.py, tests/test_gpu_poseopt*.py) and the packing of a poseopt_model.Problem into the
arguments of mcs_pose_optimization.  Every seed below was found by a search over the MODEL (tools/poseopt_seed_search.py prints the table): the scene must show
the property its test is about and keep every decision at least poseopt_model.MARGIN from its edge.  The tests assert both again, on the model."""
import ctypes as C
import importlib

import numpy as np

import poseopt_model as PM

# Cayley parameters and translations of the three Lafida cameras in the rig frame (tests/test_io_formats.py: CAYLEY)
def rig(nr):
    import test_io_formats as T
    synth = importlib.import_module("multicol-slam_amd.synth")
    return synth.lafida_cameras()[:nr], np.array(T.CAYLEY, np.float64)[:nr]


def scene(seed, n_edges, nr=3, **kw):
    cams, Mc = rig(nr)
    return PM.lafida_like_scene(seed, n_edges, cams, Mc, **kw)


def same_point_scene(seed, n_edges, nr=3, spread=3.0):
    """n_edges features of ONE camera that all hold the SAME map point, at different keypoints: a rank-deficient H (rank 2) whose minimum is not a perfect fit,
    and the reference's `if (pMP)` alone (a point held at several features gives several edges)."""
    pr = scene(seed, 1, nr, noise=0.0, start=0.05)
    rng = np.random.default_rng(1000 + seed)
    pr.xy = (np.repeat(pr.xy, n_edges, 0) + rng.normal(0, spread, (n_edges, 2))).astype(np.float32)
    pr.octave = np.repeat(pr.octave, n_edges)
    pr.cam = np.repeat(pr.cam, n_edges)
    pr.points = np.zeros(n_edges, np.int32)
    pr.n = n_edges
    return pr


# name -> (builder, kwargs).  Edge counts: 1-3 rank-deficient, 8 small, 63/64/65 the wave boundary, 1025 more edges than a workgroup has threads, 5000 many
# edges per thread; rigs of 2 and 3 cameras.
SIZES = {
    "e1": (same_point_scene, dict(seed=0, n_edges=1, nr=2)),
    "e2": (same_point_scene, dict(seed=7, n_edges=2, nr=3)),
    "e3": (same_point_scene, dict(seed=0, n_edges=3, nr=2)),
    "e8": (scene, dict(seed=0, n_edges=8, nr=3, n_outliers=1)),
    "e63": (scene, dict(seed=0, n_edges=63, nr=2, n_outliers=5, n_null=9)),
    "e64": (scene, dict(seed=0, n_edges=64, nr=3, n_outliers=5)),
    "e65": (scene, dict(seed=1, n_edges=65, nr=2, n_outliers=5, n_null=30)),
    "e1025": (scene, dict(seed=0, n_edges=1025, nr=3, n_outliers=100, n_null=200)),
    "e5000": (scene, dict(seed=0, n_edges=5000, nr=3, n_outliers=400, n_null=1000)),
}
# the quirk scenes: what each shows is asserted in tests/test_poseopt_cpu.py
QUIRKS = {
    "dead_round_two": (scene, dict(seed=0, n_edges=65, nr=3, n_outliers=5)),                          # round one ends on the gain test
    "round_two_runs": (scene, dict(seed=58, n_edges=65, nr=3, n_outliers=5, start=6.0, noise=0.5)),   # round one uses its 10 iterations
}


def build(name):
    fn, kw = {**SIZES, **QUIRKS}[name]
    return fn(**kw)


_model_cache = {}


def model(name, **kw):
    """the model's result for a named scene, computed once and shared (callers do not modify it)"""
    key = (name, tuple(sorted((k, tuple(v) if isinstance(v, (set, list, tuple)) else v) for k, v in kw.items())))
    if key not in _model_cache:
        _model_cache[key] = PM.optimize(build(name), **kw)
    return _model_cache[key]


def spread(name):
    """largest difference of the final pose between the model's edge sums in index order and in reversed order"""
    return float(np.abs(model(name).pose - model(name, reverse=True).pose).max())


def keys_of(pr, cap):
    k = np.zeros(pr.n, cap.KP_DTYPE)
    k["x"], k["y"], k["octave"] = pr.xy[:, 0], pr.xy[:, 1], pr.octave
    return k


def run_library(pkg, ctx, problems, device, with_rig=True, with_diag=True):
    """mcs_pose_optimization over a list of problems that share rig, point table layout and levels -> list of dicts (pose, MtMc, MtMc_inv, outlier, n_inliers,
    share, diag).  Every problem keeps its own point table: the tables are stacked and the ids shifted."""
    cap = pkg._capi
    fe = importlib.import_module("multicol-slam_amd.frontend")
    mem = fe._DEVICE if device else fe._HOST
    L = pkg.lib()
    npb, p0 = len(problems), problems[0]
    nr = len(p0.Mc_min)
    ocs = (cap.Ocam * nr)(*[cap.make_ocam(c) for c in p0.cams])
    base = np.cumsum([0] + [len(p.pos) for p in problems])
    pos = np.concatenate([p.pos for p in problems]) if npb else np.zeros((0, 3))
    g = dict(pos=pos, Mc=p0.Mc_min, ocs=np.frombuffer(ocs, np.uint8).copy(), sig=p0.inv_sigma2, hub=np.array([p.huber for p in problems], np.float64),
             pose=np.array([p.pose0 for p in problems], np.float64).reshape(npb, 6), MtMc=np.zeros((npb, nr, 16)), inv=np.zeros((npb, nr, 16)),
             nin=np.full(npb, -7, np.int32), share=np.full(npb, -7.0), diag=np.zeros(npb, cap.POSE_DIAG_DTYPE))
    g = {k: mem.put(v) for k, v in g.items()}
    per = []
    for p, b in zip(problems, base):
        pts = np.where((p.points >= 0) & (p.points < len(p.pos)), p.points + b, p.points).astype(np.int32)
        pts = np.where(p.points >= len(p.pos), len(pos) + 5, pts).astype(np.int32)   # a hostile id stays out of every table
        per.append(dict(keys=mem.put(keys_of(p, cap)), cam=mem.put(p.cam.astype(np.int32)), points=mem.put(pts), out=mem.put(np.full(max(p.n, 1), 9, np.uint8))))
    fr = (cap.PoseFrame * max(npb, 1))(*[cap.PoseFrame(mem.ptr(q["keys"]), mem.ptr(q["cam"]), mem.ptr(q["points"]), p.n) for q, p in zip(per, problems)])
    outs = (C.c_void_p * max(npb, 1))(*[mem.ptr(q["out"]) for q in per])
    tab = cap.PointTable(mem.ptr(g["pos"]), None, len(pos))
    rc = L.mcs_pose_optimization(ctx.h, npb, fr, C.byref(tab), mem.ptr(g["Mc"]), mem.ptr(g["ocs"]), nr, mem.ptr(g["sig"]), len(p0.inv_sigma2), mem.ptr(g["hub"]),
                                 mem.kind, mem.ptr(g["pose"]), mem.ptr(g["MtMc"]) if with_rig else None, mem.ptr(g["inv"]) if with_rig else None, outs,
                                 mem.ptr(g["nin"]), mem.ptr(g["share"]), mem.ptr(g["diag"]) if with_diag else None)
    if rc != 0:
        return rc
    r = {k: mem.read(g[k]) for k in ("pose", "MtMc", "inv", "nin", "share", "diag")}
    return [dict(pose=r["pose"][i], MtMc=r["MtMc"][i].reshape(nr, 4, 4), MtMc_inv=r["inv"][i].reshape(nr, 4, 4), outlier=mem.read(per[i]["out"])[:problems[i].n],
                 n_inliers=int(r["nin"][i]), share=float(r["share"][i]), diag=r["diag"][i]) for i in range(npb)]
