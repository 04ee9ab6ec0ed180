#!/usr/bin/env python3
"""The search behind the seeds of tests/essgraph_scenes.py (no GPU): for each scene, the first seed whose model run (tests/essgraph_model.py)

  * ends with status OK and takes the same decisions (iterations, trials, stop reason) in every run of the spread — sums in edge order and reversed, and
    eight seeds that move every acos / sin / cos / exp / log result by the OpenCL full-profile ulp bounds;
  * keeps every decision (the sign of rho, the gain against 1e-6, every branch of exp and log, every quaternion-conversion case, every LU pivot choice) at
    least its essgraph_scenes.MARGIN from its edge in all of those runs;
  * moves no output, lambda or chi2 by more than essgraph_scenes.MAX_SPREAD relative between those runs (the device may differ by twice the spread, and
    never by more than 1e-4).

    python tools/essgraph_seed_search.py [scene ...] [--first K] [--seeds N]
prints one line per scene and seed tried; paste the seeds into essgraph_scenes.SCENES.  `identity` is not searched: its decisions are taken on exact zeros."""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import essgraph_model as M   # noqa: E402
import essgraph_scenes as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scenes", nargs="*", default=[n for n in S.SCENES if n != "identity"])
    ap.add_argument("--seeds", type=int, default=40)
    ap.add_argument("--first", type=int, default=0)
    a = ap.parse_args()
    for name in a.scenes:
        for seed in range(a.first, a.first + a.seeds):
            pr = S.build(name, seed)
            runs = []
            for r in S.RUNS:
                runs.append(M.optimize(pr, lm=M.Libm(r["seed"]), reverse=r["reverse"]))
                if runs[-1].status != M.EG_OK or S.margin_ratio(runs[-1]) < 1.0:
                    break
            spread, margin, same = S.measure(runs) if len(runs) == len(S.RUNS) else (float("inf"), S.margin_ratio(runs[-1]), False)
            good = same and margin >= 1.0 and spread <= S.MAX_SPREAD
            m = runs[0]
            print("%-10s seed %3d  iters %2d stop %d trials %s  spread %.3g margin/MARGIN %.3g %s  %s" % (name, seed, m.iters, m.stop, m.trials[:m.iters], spread, margin,
                                                                                                 {k: "%.2g" % v for k, v in runs[-1].margins.m.items()},
                                                                                                 "<-- take" if good else ""), flush=True)
            if good:
                break


if __name__ == "__main__":
    main()
