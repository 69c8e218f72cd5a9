"""Wall time of cmf_aoadmm_multistart: the fused kernel (one launch, one workgroup per start) against the sequential loop of
cmf_aoadmm calls, 200 outer iterations with tol=None, NN PARAFAC2 (the examples' model) at four shapes.

    python tools/multistart_rate.py [--out profiles/multistart_rate.txt] [--seq-max 16]

Sequential calls are timed for N <= --seq-max starts; beyond that the per-start time of the largest measured N is scaled
(marked "~"): the calls are independent, one after the other."""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import decomposition as dec  # noqa: E402

SHAPES = [("examples: simulated non-negative", 10, 15, 20, 3), ("examples: examining components", 5, 10, 15, 4),
          ("2^16 elements", 16, 64, 64, 3), ("2^18 elements", 64, 64, 64, 3)]
STARTS = [1, 16, 64, 256, 1024]


def problem(I, J, K, rank, seed=0):
    rng = np.random.default_rng(seed)
    A = rng.uniform(size=(I, rank)) + 0.1
    Bb = np.maximum(rng.standard_normal(size=(J, rank)), 0)
    C = np.maximum(rng.standard_normal(size=(K, rank)), 0)
    mats = [(np.roll(Bb, i, axis=0) * A[i]) @ C.T for i in range(I)]
    return [M + 0.2 * rng.uniform(size=M.shape) * np.linalg.norm(M) / np.sqrt(M.size) for M in mats]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--seq-max", type=int, default=16)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    kw = dict(non_negative=True, n_iter_max=args.iters, tol=None)
    lines = [f"cmf_aoadmm_multistart wall time, NN PARAFAC2, {args.iters} outer iterations, tol=None, fp32 X from NumPy "
             f"({torch.cuda.get_device_name(0)})",
             "shape                              elements  N     fused_s   seq_s      fused/seq  fused_per_start_ms"]
    for name, I, J, K, r in SHAPES:
        mats = problem(I, J, K, r)
        dec.parafac2_aoadmm_multistart(mats, r, range(2), method="fused", **kw)  # warm-up
        dec.parafac2_aoadmm_multistart(mats, r, range(1), method="sequential", **kw)
        per_start_seq = None
        for n in STARTS:
            tf = timed(lambda: dec.parafac2_aoadmm_multistart(mats, r, range(n), method="fused", **kw))
            if n <= args.seq_max:
                ts = timed(lambda: dec.parafac2_aoadmm_multistart(mats, r, range(n), method="sequential", **kw))
                per_start_seq, mark = ts / n, " "
            else:
                ts, mark = per_start_seq * n, "~"
            lines.append(f"{name:34s} {I * J * K:9d} {n:5d} {tf:9.4f} {mark}{ts:9.3f} {tf / ts:10.4f} {1e3 * tf / n:12.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
