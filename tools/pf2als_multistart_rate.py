"""Wall time of parafac2_als_multistart: the fused kernel (one launch, one workgroup per start) against the sequential loop of
parafac2_als calls, 200 iterations with tol=0 (every iteration runs) at four shapes.

    python tools/pf2als_multistart_rate.py [--out profiles/pf2als_multistart_rate.txt] [--seq-max 16]

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
from tests import parafac2_als_restatement as R  # noqa: E402

# (name, I, J_range, K, rank, nn_modes, seed); the semiconductor seed keeps X under the fused bound of 2^18 elements
SHAPES = [("semiconductor 108 x 100-120 x 21", 108, (100, 120), 21, 2, [0], 3), ("10 x 15 x 20", 10, (15, 15), 20, 3, None, 0),
          ("16 x 64 x 64", 16, (64, 64), 64, 4, None, 0), ("64 x 64 x 64", 64, (64, 64), 64, 8, None, 0)]
STARTS = [1, 16, 64, 256, 1024]


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
    lines = [f"parafac2_als_multistart wall time, {args.iters} iterations, tol=0, n_iter_parafac=5, fp32 X from NumPy "
             f"({torch.cuda.get_device_name(0)})",
             "shape                              rank elements  N     fused_s   seq_s      fused/seq  fused_per_start_ms"]
    for name, I, J_range, K, r, nn_modes, seed in SHAPES:
        mats = R.parafac2_problem(I, J_range, K, r, seed=seed, noise=0.2)[0]
        n_el = sum(m.size for m in mats)
        kw = dict(n_iter_max=args.iters, tol=0, nn_modes=nn_modes)
        dec.parafac2_als_multistart(mats, r, range(2), method="fused", **kw)  # warm-up
        dec.parafac2_als_multistart(mats, r, range(1), method="sequential", **kw)
        per_start_seq = None
        for n in STARTS:
            tf = timed(lambda: dec.parafac2_als_multistart(mats, r, range(n), method="fused", **kw))
            if n <= args.seq_max:
                ts = timed(lambda: dec.parafac2_als_multistart(mats, r, range(n), method="sequential", **kw))
                per_start_seq, mark = ts / n, " "
            else:
                ts, mark = per_start_seq * n, "~"
            lines.append(f"{name:34s} {r:4d} {n_el:8d} {n:5d} {tf:9.4f} {mark}{ts:9.3f} {tf / ts:10.4f} {1e3 * tf / n:12.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
