#!/usr/bin/env python3
"""Seed search over the PoseOptimization MODEL (tests/poseopt_model.py) for the scenes of tests/poseopt_scenes.py: for every named scene, the first seeds whose
run keeps every decision at least MARGIN from its edge and, for the quirk scenes, shows the property the test is about.  No GPU.  Prints one line per hit:
name, seed, iterations, stop codes, trials, inliers, margin, spread (index order against reversed order).

--hostile: the same over the table of tests/hostile_poseopt.py (the property of each scene is what tests/test_poseopt_hostile_cpu.py asserts; here a hit is a
seed that runs, keeps its status and its margin; an excused scene is printed with its margin whatever it is).
--late: the search behind group F of that table: runs whose first evaluation passes the screen and whose later build or trial pass holds a non-finite sum."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import poseopt_model as PM   # noqa: E402
import poseopt_scenes as S   # noqa: E402

WANT = {
    "dead_round_two": lambda r: r.stop[0] == PM.STOP_GAIN and r.iters[1] == 0,
    "round_two_runs": lambda r: r.iters[0] == 10 and r.stop[0] == PM.STOP_ITERATIONS and r.iters[1] > 0 and r.outlier.any(),
}
# ... and every "repaired" variant of the second round must give another result on that scene
FIXES = {"round_two_runs": ("second_all_levels", "reset_nbad", "second_clears"), "dead_round_two": ("clear_stop",)}


def differs(a, b):
    return not (np.array_equal(a.pose, b.pose) and np.array_equal(a.outlier, b.outlier) and a.n_inliers == b.n_inliers and a.share == b.share)


def line(name, seed, pr, r):
    sp = np.abs(PM.optimize(pr, reverse=True).pose - r.pose).max()
    print(name, seed, "status", r.status, r.iters, r.stop, r.trials[0][:r.iters[0]].tolist(), r.trials[1][:r.iters[1]].tolist(), r.n_inliers,
          "failed solves %d active %s late %s" % (r.failed_solves, r.n_active, r.late_nonfinite), "margin %.2e spread %.2e" % (r.margin, sp))


def hostile(a):
    import hostile_poseopt as H
    for name in a.names or H.SCENES:
        fn, kw = H.SCENES[name]
        want = PM.POSE_NONFINITE if name in H.NONFINITE else PM.POSE_OK
        hits = 0
        for seed in [kw["seed"]] + [s for s in range(a.seeds) if s != kw["seed"]]:      # the table's own seed first
            try:
                pr = fn(**{**kw, "seed": seed})
            except AssertionError:               # the builder could not place its special features at this seed
                continue
            r = PM.optimize(pr)
            if r.status != want or not (r.margin >= PM.MARGIN or name in H.EXCUSED):
                continue
            line(name, seed, pr, r)
            hits += 1
            if hits >= a.hits:
                break
        if not hits:
            print(name, "no seed below", a.seeds)


def late(a):
    """the control at seeds 0 .. 9 and starts 0.02, 3, 10, 30 under huge weights, scales, keys, Cayley starts and points"""
    import hostile_poseopt as H
    n = 0
    for seed in range(10):
        for start in (0.02, 3, 10, 30):
            cands = []
            for w in (1e290, 1e300, 1e303, 1e305, 1e306, 1e307):
                for every in (False, True):
                    pr = H.base(seed, start=start)
                    pr.inv_sigma2 = pr.inv_sigma2 * w if every else np.where(np.arange(len(pr.inv_sigma2)) == 3, w, pr.inv_sigma2)
                    cands.append(("%s weight %g" % ("every" if every else "one", w), pr))
            for f in (1e100, 1e140, 1e150, 1e152, 1e153):
                pr = H.base(seed, start=start)
                pr.pos, pr.Mc_min = pr.pos * f, pr.Mc_min * np.array([1, 1, 1, f, f, f])
                pr.pose0[3:] *= f
                cands.append(("scale %g" % f, pr))
            for k in (1e30, 1e38, 3.4e38):
                pr = H.base(seed, start=start)
                pr.xy[pr.edges()[7]] = (k, -k)
                cands.append(("key %g" % k, pr))
            for c in (1e3, 1e5, 1e8, 1e100, 1e153, 1e154):
                pr = H.base(seed, start=start)
                pr.pose0[:3] = c
                cands.append(("cayley %g" % c, pr))
            for X in ((1e154, 1e154, 0), (1e200, 0, 0), (1e300, 1e300, 1e300), (1e305, 0, 0), (1e307, 1e307, 1e307)):
                pr = H.base(seed, start=start)
                pr.pos[pr.points[pr.edges()[11]]] = X
                cands.append(("point %s" % (X,), pr))
            for tag, pr in cands:
                r = PM.optimize(pr)
                n += 1
                if r.status == PM.POSE_OK and any(r.late_nonfinite):
                    line("%s start %g" % (tag, start), seed, pr, r)
    print("searched", n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--hits", type=int, default=3)
    ap.add_argument("--hostile", action="store_true")
    ap.add_argument("--late", action="store_true")
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    if a.hostile or a.late:
        return hostile(a) if a.hostile else late(a)
    table = {**S.SIZES, **S.QUIRKS}
    for name in a.names or table:
        fn, kw = table[name]
        hits = 0
        for seed in range(a.seeds):
            pr = fn(**{**kw, "seed": seed})
            r = PM.optimize(pr)
            if not r.margin >= PM.MARGIN or not WANT.get(name, lambda r: True)(r):
                continue
            if not all(differs(r, PM.optimize(pr, fix={f})) for f in FIXES.get(name, ())):
                continue
            sp = np.abs(PM.optimize(pr, reverse=True).pose - r.pose).max()
            print(name, seed, r.iters, r.stop, r.trials[0][:r.iters[0]].tolist(), r.trials[1][:r.iters[1]].tolist(), r.n_inliers, "margin %.2e spread %.2e" % (r.margin, sp))
            hits += 1
            if hits >= a.hits:
                break
        if not hits:
            print(name, "no seed below", a.seeds)


if __name__ == "__main__":
    main()
