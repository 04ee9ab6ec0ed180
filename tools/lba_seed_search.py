#!/usr/bin/env python3
"""Finds the seeds of tests/lba_scenes.py: for every named scene the first seed whose MODEL run (tests/lba_model.py, no GPU) keeps every decision at least
lba_model.MARGIN from its edge, in index order and in reversed order, and shows the path the scene is there for.  Prints one line per scene; paste the seeds
into lba_scenes.SCENES.

    python tools/lba_seed_search.py [scene ...] [--tries N]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import lba_model as LM  # noqa: E402
import lba_scenes as S  # noqa: E402

# what the scene must show, on the model's result with a NULL flag (m) and, where asked, with the caller's flag (mf)
PATHS = {
    "pair": lambda m, mf: m.status == 0 and m.iters[0] >= 2,
    "window": lambda m, mf: m.status == 0 and m.n_erased[0] >= 6 and m.stop[0] == LM.STOP_ITERATIONS and m.iters[1] >= 2,
    "slow": lambda m, mf: m.status == 0 and m.stop[0] == LM.STOP_ITERATIONS and m.iters[0] == 10 and m.iters[1] >= 2,
    "twice": lambda m, mf: m.status == 0 and m.pt_state[2] == LM.PT_KEPT and m.pt_state[3] == LM.PT_WRITTEN,
    "split": lambda m, mf: m.status == 0 and m.stop[0] == LM.STOP_GAIN and mf.status == LM.LBA_STOPPED and mf.flag_out,
    "hub": lambda m, mf: m.status == 0,
    "long_row": lambda m, mf: m.status == 0 and m.n_erased[0] >= 10,
    "cap": lambda m, mf: m.status == 0 and m.n_free == 64,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=list(S.SCENES))
    ap.add_argument("--tries", type=int, default=200)
    a = ap.parse_args()
    for name in a.scenes:
        fn, kw = S.SCENES[name]
        for seed in range(a.tries):
            S.SCENES[name] = (fn, dict(kw, seed=seed))
            S._model_cache.clear()
            m, r = S.model(name), S.model(name, reverse=True)
            mf = S.model(name, flag=False)
            same = m.iters == r.iters and m.stop == r.stop and (m.trials == r.trials).all() and (m.edge_state == r.edge_state).all()
            if min(m.margin, r.margin, mf.margin) >= LM.MARGIN and same and m.failed_solves == 0 and PATHS[name](m, mf):
                print("%-9s seed %3d  margin %.2e  iters %s  stop %s  erased %s  spread %.2e" % (name, seed, min(m.margin, r.margin), m.iters, m.stop, m.n_erased,
                                                                                                S.spread(name)), flush=True)
                break
        else:
            print("%-9s no seed in %d tries" % (name, a.tries), flush=True)
        S.SCENES[name] = (fn, kw)


if __name__ == "__main__":
    main()
