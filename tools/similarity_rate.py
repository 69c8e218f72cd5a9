"""Wall time of multistart_similarity at 1024 models of the examples' size (I 10, J 15, K 20): one-vs-all and all-pairs on the
device (csrc/similarity.hip) and on the host (NumPy + one scipy linear_sum_assignment per pair), rank 3 and rank 16.

    python tools/similarity_rate.py [--out profiles/similarity_rate.txt] [--host-all-pairs-models 128]

"call" is the whole multistart_similarity call from NumPy models (packing, upload, launch, download); "launch" is
_engine.fms_scores alone on models already packed on the device (upload of the pairs, two kernels, one synchronise).  Each is
the median of --repeats calls after a warm-up.  The host all-pairs time is measured at --host-all-pairs-models models and scaled
by the number of pairs (marked "~"): the pairs are independent, one after the other."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import _engine, similarity as sim  # noqa: E402

I, J, K, N_MODELS = 10, 15, 20, 1024


def models_of(rank, n, seed=0):
    rng = np.random.RandomState(seed)
    return [(rng.uniform(0.5, 2.0, rank), (rng.standard_normal((I, rank)), [rng.standard_normal((J, rank)) for _ in range(I)],
                                           rng.standard_normal((K, rank)))) for _ in range(n)]


def timed(fn, repeats):
    fn()  # warm-up: library load, code objects, allocator
    times = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-all-pairs-models", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similarity_rate.py measures on an MI355X: no device is visible")
    n, m = N_MODELS, args.host_all_pairs_models
    lines = [f"multistart_similarity wall time, {n} models of I {I}, J {J} (N {I * J}), K {K}, weights given, permutations returned, "
             f"median of {args.repeats} ({torch.cuda.get_device_name(0)})",
             "rank  what         pairs    device_call_s  device_launch_s  host_s      host/device_call  device_us_per_pair"]
    for rank in (3, 16):
        models = models_of(rank, n)
        sim_models = [sim._Model(c) for c in models]
        packed, weights = sim._pack(sim_models, torch.device("cuda"))
        s, t = np.triu_indices(n)
        cases = [("one-vs-all", np.stack([np.zeros(n, dtype=np.int64), np.arange(n)], 1), dict(reference=0)),
                 ("all-pairs", np.stack([s, t], 1), dict(all_pairs=True))]
        for what, pairs, how in cases:
            call = timed(lambda: sim.multistart_similarity(models, return_permutations=True, method="device", **how), args.repeats)
            pairs32 = pairs.astype(np.int32)
            launch = timed(lambda: _engine.fms_scores(packed, I, I * J, K, rank, weights, pairs32, 3, -1, True), args.repeats)
            if what == "one-vs-all":
                host, mark = timed(lambda: sim.multistart_similarity(models, return_permutations=True, method="host", **how), 1), " "
            else:
                host = timed(lambda: sim.multistart_similarity(models[:m], return_permutations=True, method="host", **how), 1)
                host, mark = host * len(pairs) / (m * (m + 1) // 2), "~"
            # the two methods on the same pairs, before the times are believed
            dev = sim.multistart_similarity(models[:m], return_permutations=True, method="device", **how)
            ref = sim.multistart_similarity(models[:m], return_permutations=True, method="host", **how)
            assert np.abs(dev[0] - ref[0]).max() <= 1e-12, np.abs(dev[0] - ref[0]).max()
            lines.append(f"{rank:4d}  {what:11s} {len(pairs):7d} {call:14.5f} {launch:16.5f} {mark}{host:10.4f} {host / call:17.1f} "
                         f"{1e6 * launch / len(pairs):19.3f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
