"""Wall time of parafac2_aoadmm_missing at the examples' size (10 matrices of 15 x 20, rank 3, NonNegativity on every mode and
PARAFAC2, 200 iterations, tol=None, 30 % of the entries missing at random, column-mean fill): 64 and 1024 jobs in one launch of
k_multistart_missing against parafac2_aoadmm_multistart(method="fused") on the complete data with the same number of starts, in
the same process, and of both the time inside the library's entry point (the copy into the fp64 slices and the fit kernel;
synchronised before and after).

    python tools/missing_rate.py [--out profiles/missing_rate.txt]

Every figure is the median of --reps alternating repetitions after a warm-up of each method."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import _engine, missing  # noqa: E402
from matcouply_amd import decomposition as dec  # noqa: E402
from tests.test_gpu_multistart import _example_problem  # noqa: E402

ENTRY = {}


def _stamped(name):
    inner = getattr(_engine, name)

    def run(*args, **kwargs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(*args, **kwargs)
        torch.cuda.synchronize()
        ENTRY[name] = time.perf_counter() - t0
        return out

    setattr(_engine, name, run)


def timed(fn, entry):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, ENTRY[entry]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--jobs", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    mats = _example_problem(10, 15, 20, 3, 0.2, False)
    rng = np.random.RandomState(0)
    holed = [np.where(rng.uniform(size=m.shape) >= 0.3, m, np.nan) for m in mats]
    kw = dict(non_negative=True, n_iter_max=args.iters, tol=None)
    _stamped("multistart_run_missing")
    _stamped("multistart_run")
    lines = [
        f"parafac2_aoadmm_missing wall time, the examples' size ({len(mats)} matrices, {sum(m.size for m in mats)} elements, rank 3), "
        f"non_negative=True, {args.iters} iterations, tol=None, {100 * float(np.mean(np.isnan(np.concatenate(holed)))):.1f} % of the "
        f"entries missing, fill=\"column_mean\", fp32 X from NumPy, median of {args.reps} alternating repetitions "
        f"({torch.cuda.get_device_name(0)})"]
    for n in args.jobs:
        runs = {
            "missing": (lambda: missing.parafac2_aoadmm_missing(holed, 3, None, range(n), **kw), "multistart_run_missing"),
            "complete": (lambda: dec.parafac2_aoadmm_multistart(mats, 3, range(n), method="fused", **kw), "multistart_run"),
        }
        for fn, _ in runs.values():  # warm-up
            fn()
        times = {name: [] for name in runs}
        for _ in range(args.reps):  # alternating
            for name, (fn, entry) in runs.items():
                times[name].append(timed(fn, entry))
        wall = {name: float(np.median([t[0] for t in ts])) for name, ts in times.items()}
        entry = {name: float(np.median([t[1] for t in ts])) for name, ts in times.items()}
        lines += [
            f"{n:5d} jobs, parafac2_aoadmm_missing                              {wall['missing'] * 1e3:10.2f} ms   in the entry point {entry['missing'] * 1e3:10.2f} ms",
            f"{n:5d} starts, parafac2_aoadmm_multistart fused, complete data    {wall['complete'] * 1e3:10.2f} ms   in the entry point {entry['complete'] * 1e3:10.2f} ms",
            f"{n:5d} missing / complete                                         {wall['missing'] / wall['complete']:10.4f}      in the entry point {entry['missing'] / entry['complete']:10.4f}",
            f"{n:5d} all repetitions, wall ms: " + "; ".join(f"{name} " + " ".join(f"{1e3 * t[0]:.1f}" for t in ts) for name, ts in times.items()),
        ]
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
