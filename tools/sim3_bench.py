"""(MI355X) The device Sim3 RANSAC (mcs_sim3_*): hypothesis x correspondence evaluations per second and per-call latency, solvers in {1, 8, 32} x N in
{50, 500, 3000, 16000}, for the two call patterns of cLoopClosing::ComputeSim3: a full 300-iteration sweep per solver, and the loop closer's
iterate(50) rounds.  Medians over warm calls, each ending in the call's own synchronisation.  Every size is checked against tests/sim3_model.py
(picks, counts, masks of sampled hypotheses) before it is timed.  Kernel times: run under `rocprofv3 --kernel-trace --stats -- python tools/sim3_bench.py`.

The pairs are pure outliers with minInliers = 0.3 N and probability 0.999999, so no call stops early and mRansacMaxIts is 300 at every N (at the loop
closer's (0.98, 15, 300) the iteration count of N >= 12 282 collapses to 1: DESIGN.md section 7)."""
import argparse
import ctypes as C
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
pkg = importlib.import_module("multicol-slam_amd")
synth = importlib.import_module("multicol-slam_amd.synth")
import sim3_model as M   # noqa: E402


class Batch:
    def __init__(self, ctx, cams, M_c, pairs, params, seed):
        L = pkg.lib()
        nr, ns = len(cams), len(pairs)
        self.L, self.ns = L, ns
        Mc = np.ascontiguousarray(np.stack(M_c).reshape(nr, 16))
        ocs = (pkg._capi.Ocam * nr)(*[pkg.make_ocam(c) for c in cams])
        off = np.zeros(ns + 1, np.int32)
        off[1:] = np.cumsum([len(p["index1"]) for p in pairs])
        cat = lambda k, dt: np.ascontiguousarray(np.concatenate([p[k] for p in pairs]), dt)
        self.n1 = np.array([p["mN1"] for p in pairs], np.int32)
        self.p = np.array([q[0] for q in params], np.float64)
        self.mi = np.array([q[1] for q in params], np.int32)
        self.mx = np.array([q[2] for q in params], np.int32)
        a = [Mc, ocs, off, np.ascontiguousarray(np.stack([p["M_t_inv"] for p in pairs])), np.ascontiguousarray(np.stack([p["MtMc_inv"] for p in pairs])),
             cat("Xw", np.float64), cat("cam", np.int32), cat("sigma2", np.float64), cat("index1", np.int32)]
        self.keep = a
        pp = pkg.np_ptr
        self.h = C.c_void_p()
        pkg.check(L.mcs_sim3_create(ctx.h, nr, pp(a[0]), a[1], ns, pp(self.n1), pp(a[2]), pp(a[3]), pp(a[4]), pp(self.p), pp(self.mi), pp(self.mx),
                                    pp(a[5]), pp(a[6]), pp(a[7]), pp(a[8]), C.c_uint64(seed), None, C.byref(self.h)))
        ns = self.ns
        self.succ, self.nm, self.ni, self.T = np.zeros(ns, np.uint8), np.zeros(ns, np.uint8), np.zeros(ns, np.int32), np.zeros((ns, 16))
        self.vb = np.zeros(int(self.n1.sum()), np.uint8)

    def reset(self):
        pkg.check(self.L.mcs_sim3_set_ransac_parameters(self.h, pkg.np_ptr(self.p), pkg.np_ptr(self.mi), pkg.np_ptr(self.mx)))

    def iterate(self, n):
        pp = pkg.np_ptr
        nit = np.full(self.ns, n, np.int32)
        pkg.check(self.L.mcs_sim3_iterate(self.h, pp(nit), pp(self.succ), pp(self.nm), pp(self.ni), pp(self.T), pp(self.vb)))

    def info(self):
        n, mx, it = np.zeros(self.ns, np.int32), np.zeros(self.ns, np.int32), np.zeros(self.ns, np.int32)
        pkg.check(self.L.mcs_sim3_info(self.h, pkg.np_ptr(n), pkg.np_ptr(mx), pkg.np_ptr(it)))
        return n, mx, it

    def hypotheses(self, s, first, count, N):
        pp = pkg.np_ptr
        picks, cnt, hyp, inl = np.zeros((count, 3), np.int32), np.zeros(count, np.int32), np.zeros((count, 45)), np.zeros((count, N), np.uint8)
        pkg.check(self.L.mcs_sim3_hypotheses(self.h, s, first, count, pp(picks), pp(cnt), pp(hyp), pp(inl)))
        return picks, cnt, inl.astype(bool)

    def __del__(self):
        self.L.mcs_sim3_destroy(self.h)


def check_against_model(b, pair, cams, M_c, seed, param):
    m = M.model_of(pair, cams, M_c)
    m.SetRansacParameters(*param)
    N = len(pair["index1"])
    picks, cnt, inl = b.hypotheses(0, 0, 3, N)
    for k in range(3):
        p, h, einl, near = m.evaluate(k, M.generated_draws(seed, 0, N))
        assert list(picks[k]) == p and np.array_equal(inl[k] & ~near, einl & ~near) and (near.any() or cnt[k] == einl.sum()), ("model mismatch", N, k)
    return True


def median_ms(fn, reps, before=None):
    t = []
    for _ in range(reps):
        if before:
            before()
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solvers", default="1,8,32")
    ap.add_argument("--sizes", default="50,500,3000,16000")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    ctx = pkg.Context(0)
    cams3 = synth.lafida_cameras()
    rows = []
    for N in [int(x) for x in a.sizes.split(",")]:
        nr = 8 if N >= 16000 else 3
        cams = [cams3[c % 3] for c in range(nr)]
        M_c = M.rig_poses(nr)
        rng = np.random.default_rng(N)
        base = M.make_pair(rng, M_c, N, inlier_frac=0.0)
        param = (0.999999, int(math.ceil(0.3 * N)), 300)
        for ns in [int(x) for x in a.solvers.split(",")]:
            b = Batch(ctx, cams, M_c, [base] * ns, [param] * ns, seed=11)
            assert b.info()[1].tolist() == [300] * ns
            check_against_model(b, base, cams, M_c, 11, param)
            b.iterate(300)   # warm
            full = median_ms(lambda: b.iterate(300), a.reps, b.reset)
            assert b.info()[2].tolist() == [300] * ns and not b.succ.any()
            b.reset()
            b.iterate(50)
            r50 = median_ms(lambda: b.iterate(50), a.reps, b.reset)
            evals = ns * 300 * N
            row = dict(solvers=ns, N=N, cams=nr, sweep300_ms=round(full, 4), evals_per_s=float("%.4g" % (evals / (full * 1e-3))), round50_ms=round(r50, 4),
                       checked=True)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del b
    return rows


if __name__ == "__main__":
    main()
