#!/usr/bin/env python3
"""Find the seeds of tests/sim3opt_scenes.py (CPU only, the model alone; not part of any test).  For every scene of the table, scan seeds until the model's run
shows the property the scene stands for, keeps every decision at least --margin from its edge, and takes the same decisions under reversed edge sums and
under the eight perturbation seeds.  Prints one line per scene: the seed to put into the table, or what the first seeds lacked.

    python tools/sim3opt_seed_search.py [--margin 1e-6] [--seeds 200] [name ...]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sim3opt_model as M   # noqa: E402
import sim3opt_scenes as S  # noqa: E402

# what a scene must show (m: the model's plain run)
WANT = {
    "nbad0": lambda m, pr: m.n_bad1 == 0 and m.iters[1] >= 1,
    "nbad": lambda m, pr: m.n_bad1 > 0 and m.iters[1] > 5 and M.rel_spread(m.S12, M.optimize(pr, fix=("always_5",)).S12) > 1e-4,   # the second round needs more than 5 of its 10 iterations, visibly
    "return0": lambda m, pr: 0 < m.n_corr - m.n_bad1 < 3,
    "dead_round_two": lambda m, pr: m.stop == [M.STOP_GAIN, M.STOP_NOT_RUN] and m.n_bad1 > 0,
    "far_start": lambda m, pr: m.trials[0, :3].max() > 1 and m.iters[1] >= 1,       # rejected on the way, not at the noise floor of the last iteration
    "tiny_step": lambda m, pr: m.branches[0] == 0,
    "negative_trace": lambda m, pr: pr.R12[0, 0] + pr.R12[1, 1] + pr.R12[2, 2] < 0 and m.n_bad1 > 0,
    "n3": lambda m, pr: m.n_inliers == 3,
}


def ok(kw, want, margin):
    pr = S.scene(**kw)
    m = M.optimize(pr)
    if not want(m, pr):
        return "property"
    if not m.margin >= margin:
        return "margin %.1e" % m.margin
    for o in [M.optimize(pr, reverse=True)] + [M.optimize(pr, lm=M.Libm(s)) for s in S.SEEDS]:
        if not (o.iters == m.iters and o.stop == m.stop and (o.trials == m.trials).all() and (o.keep == m.keep).all()):
            return "unstable"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--margin", type=float, default=1e-6)
    ap.add_argument("--seeds", type=int, default=200)
    ap.add_argument("names", nargs="*")
    a = ap.parse_args()
    for name in a.names or list(S.ALL):
        want = WANT.get(name, lambda m, pr: m.n_corr < 3 or m.iters[1] >= 1)   # a size scene: both rounds run
        why = {}
        for seed in range(a.seeds):
            r = ok({**S.ALL[name], "seed": seed}, want, a.margin)
            if r is None:
                print("%-16s seed=%d" % (name, seed), flush=True)
                break
            why[r.split()[0]] = why.get(r.split()[0], 0) + 1
        else:
            print("%-16s none in %d seeds: %s" % (name, a.seeds, why), flush=True)


if __name__ == "__main__":
    main()
