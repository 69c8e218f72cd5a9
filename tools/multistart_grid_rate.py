"""Wall time of parafac2_aoadmm_grid: G grid points x 4 starts as ONE fused launch (mcl_multistart_run_grid) against the same G
points as G calls of parafac2_aoadmm_multistart(method="fused") with 4 starts each - the way without the grid.  NN PARAFAC2 (the
examples' model), 200 outer iterations with tol=None; the points differ in l2_penalty and feasibility_penalty_scale.

    python tools/multistart_grid_rate.py [--out profiles/multistart_grid_rate.txt] [--reps 7]

Both ways are warmed up, then timed alternately `--reps` times each (host clock around a device synchronise); the table gives
the medians and, for the ratio's spread, the extremes."""
import argparse
import itertools
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import decomposition as dec  # noqa: E402

SHAPES = [("examples: simulated non-negative", 10, 15, 20, 3), ("examples: examining components", 5, 10, 15, 4),
          ("2^16 elements", 16, 64, 64, 3)]
POINTS = [1, 4, 16, 64]
STARTS = 4


def problem(I, J, K, rank, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.uniform(size=(I, rank)) + 0.1
    Bb = np.maximum(rng.standard_normal(size=(J, rank)), 0)
    C = np.maximum(rng.standard_normal(size=(K, rank)), 0)
    mats = [(np.roll(Bb, i, axis=0) * A[i]) @ C.T for i in range(I)]
    return [M + 0.2 * rng.uniform(size=M.shape) * np.linalg.norm(M) / np.sqrt(M.size) for M in mats]


def grid_of(n):
    l2 = [0.0, 0.01, 0.1, 1.0, 0.003, 0.03, 0.3, 3.0]
    scale = [0.5, 1, 2, 4, 0.25, 0.75, 1.5, 3]
    return [dict(l2_penalty=a, feasibility_penalty_scale=b) for a, b in itertools.islice(itertools.product(l2, scale), n)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    kw = dict(non_negative=True, n_iter_max=args.iters, tol=None)
    lines = [f"parafac2_aoadmm_grid wall time, NN PARAFAC2, {args.iters} outer iterations, tol=None, {STARTS} starts per grid point, "
             f"fp32 X from NumPy, median of {args.reps} alternating repetitions ({torch.cuda.get_device_name(0)})",
             "shape                              elements points  jobs  grid_ms [min, max]         calls_ms [min, max]       "
             "grid/calls  grid_per_job_ms"]
    for name, I, J, K, r in SHAPES:
        mats = problem(I, J, K, r)
        for n in POINTS:
            grid = grid_of(n)
            one = lambda: dec.parafac2_aoadmm_grid(mats, r, grid, range(STARTS), method="fused", **kw)
            many = lambda: [dec.parafac2_aoadmm_multistart(mats, r, range(STARTS), method="fused", **kw, **p) for p in grid]
            one(), many()  # warm-up
            tg, tc = [], []
            for _ in range(args.reps):
                tg.append(timed(one))
                tc.append(timed(many))
            mg, mc = statistics.median(tg), statistics.median(tc)
            lines.append(f"{name:34s} {I * J * K:8d} {n:6d} {n * STARTS:5d} {1e3 * mg:8.1f} [{1e3 * min(tg):7.1f}, {1e3 * max(tg):7.1f}] "
                         f"{1e3 * mc:9.1f} [{1e3 * min(tc):7.1f}, {1e3 * max(tc):7.1f}] {mg / mc:10.4f} {1e3 * mg / (n * STARTS):12.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
