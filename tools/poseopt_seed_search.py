#!/usr/bin/env python3
"""Seed search over the PoseOptimization MODEL (tests/poseopt_model.py) for the scenes of tests/poseopt_scenes.py: for every named scene, the first seeds whose
run keeps every decision at least MARGIN from its edge and, for the quirk scenes, shows the property the test is about.  No GPU.  Prints one line per hit:
name, seed, iterations, stop codes, trials, inliers, margin, spread (index order against reversed order)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--hits", type=int, default=3)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
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
