"""Wall time of parafac2_aoadmm_resample at the examples' size (10 matrices of 15 x 20, rank 3, NonNegativity on every mode and
PARAFAC2, 200 iterations, tol=None): 64 bootstrap jobs in one launch of the fused kernel (k_multistart_weighted) against the
sequential method (4 jobs timed, scaled to 64), and the weighted launch against cmf_aoadmm_multistart on the same 64 starts.

    python tools/cmf_resample_rate.py [--out profiles/cmf_resample_rate.txt]

Every figure is the median of --reps alternating repetitions after a warm-up of each method.  The fused kernel skips the passes
over X, the systems and the prox steps of a job's zero-weight matrices (about 35 % of the matrices of a bootstrap job); "all
weights 1" runs the same kernel on 64 jobs that have none, which is the time without the skip."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import decomposition as dec  # noqa: E402
from matcouply_amd import resampling as rs  # noqa: E402
from tests.test_gpu_multistart import _example_problem  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--seq-jobs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    mats = _example_problem(10, 15, 20, 3, 0.2, False)
    n, I = args.jobs, len(mats)
    weights = rs.resampling_weights(I, "bootstrap", n=n, random_state=0)
    kw = dict(non_negative=True, n_iter_max=args.iters, tol=None)
    runs = {
        "fused": lambda: rs.parafac2_aoadmm_resample(mats, 3, weights, range(n), method="fused", **kw),
        "sequential": lambda: rs.parafac2_aoadmm_resample(mats, 3, weights[: args.seq_jobs], range(args.seq_jobs), method="sequential", **kw),
        "ones": lambda: rs.parafac2_aoadmm_resample(mats, 3, np.ones((n, I)), range(n), method="fused", **kw),
        "multistart": lambda: dec.parafac2_aoadmm_multistart(mats, 3, range(n), method="fused", **kw),
    }
    for fn in runs.values():  # warm-up
        fn()
    times = {name: [] for name in runs}
    for _ in range(args.reps):  # alternating
        for name, fn in runs.items():
            times[name].append(timed(fn))
    med = {name: float(np.median(t)) for name, t in times.items()}
    seq = med["sequential"] * n / args.seq_jobs
    lines = [
        f"parafac2_aoadmm_resample wall time, the examples' size ({I} matrices, {sum(m.size for m in mats)} elements, rank 3), "
        f"non_negative=True, {args.iters} iterations, tol=None, fp32 X from NumPy, median of {args.reps} alternating repetitions "
        f"({torch.cuda.get_device_name(0)})",
        f"zero-weight matrices per bootstrap job: {100 * float(np.mean(weights == 0)):.1f} %",
        f"{n} bootstrap jobs, fused (one launch)                      {med['fused'] * 1e3:10.2f} ms   {med['fused'] * 1e3 / n:8.3f} ms per job",
        f"{n} bootstrap jobs, sequential ({args.seq_jobs} timed: {med['sequential'] * 1e3:.1f} ms, scaled)  {seq * 1e3:10.2f} ms   {seq * 1e3 / n:8.3f} ms per job",
        f"fused / sequential                                          {med['fused'] / seq:10.4f}",
        f"{n} jobs with all weights 1, fused (no matrix skipped)       {med['ones'] * 1e3:10.2f} ms",
        f"cmf_aoadmm_multistart, the same {n} starts, fused            {med['multistart'] * 1e3:10.2f} ms",
        f"weighted (all weights 1) / cmf_aoadmm_multistart            {med['ones'] / med['multistart']:10.4f}",
        f"bootstrap weights / all weights 1 (the skip)                {med['fused'] / med['ones']:10.4f}",
        "all repetitions, ms: " + "; ".join(f"{name} " + " ".join(f"{1e3 * t:.1f}" for t in ts) for name, ts in times.items()),
    ]
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
