"""Wall time of multistart_evaluation at 1024 models: rank 3 at the examples' size (I 10, J 15, K 20) and rank 16 at I 20, J 40,
K 24 (the core needs I, J_i and K of at least the rank).  The device form (csrc/evaluate.hip: one read of X per model, the r x r
and r x r x r algebra in a second kernel) against the dense route a user has without it: cmf_to_matrices of every model, the data
on the host, and the algebra in NumPy (pinv of A, B_i and C).

    python tools/evaluation_rate.py [--out profiles/evaluation_rate.txt] [--dense-models 64]

"call" is the whole multistart_evaluation(method="device") call from NumPy models and NumPy data (packing, upload, two entries,
download); "launch" is _engine.eval_tables + _engine.eval_core alone on models and data already on the device, synchronised.
Each is the median of --repeats calls after a warm-up.  The dense route is measured at --dense-models models and scaled by the
number of models (marked "~"): the models are independent, one after the other."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import _engine, evaluation as ev, similarity as sim  # noqa: E402
from matcouply_amd.coupled_matrices import cmf_to_matrices  # noqa: E402
from matcouply_amd.decomposition import _pack as pack_data  # noqa: E402

N_MODELS = 1024
SIZES = {3: (10, 15, 20), 16: (20, 40, 24)}  # rank -> (I, J, K)


def problem(rank, n, seed=0):
    """data from one model plus noise, and n models around it (every factor perturbed by 10 %)"""
    I, J, K = SIZES[rank]
    rng = np.random.RandomState(seed)
    A, B_is, C = rng.uniform(0.1, 1.1, (I, rank)), [rng.standard_normal((J, rank)) for _ in range(I)], rng.standard_normal((K, rank))
    Xs = [(B_i * A[i]) @ C.T for i, B_i in enumerate(B_is)]
    Xs = [(X + 0.2 * np.linalg.norm(X) / np.sqrt(X.size) * rng.standard_normal(X.shape)).astype(np.float32) for X in Xs]
    near = lambda F: F + 0.1 * np.abs(F).mean() * rng.standard_normal(F.shape)
    return Xs, [(None, (near(A), [near(B_i) for B_i in B_is], near(C))) for _ in range(n)]


def dense_route(Xs, models):
    """what a user writes today: one dense reconstruction per model, then NumPy"""
    out = []
    X64 = [X.astype(np.float64) for X in Xs]
    norm = sum(np.sum(X ** 2) for X in X64)
    for cmf in models:
        _, (A, B_is, C) = cmf
        sse = np.array([np.sum((X - M) ** 2) for X, M in zip(X64, cmf_to_matrices(cmf))])
        Cp = np.linalg.pinv(C)
        W = np.stack([np.linalg.pinv(B_i) @ X @ Cp.T for B_i, X in zip(B_is, X64)])
        G = np.einsum("pi,iqs->pqs", np.linalg.pinv(A), W)
        r = len(G)
        T = np.zeros_like(G)
        T[np.arange(r), np.arange(r), np.arange(r)] = 1.0
        out.append((1.0 - sse.sum() / norm, sse, 100.0 * (1.0 - np.sum((G - T) ** 2) / r)))
    return out


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
    ap.add_argument("--dense-models", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("evaluation_rate.py measures on an MI355X: no device is visible")
    n, m = N_MODELS, args.dense_models
    lines = [f"multistart_evaluation wall time, {n} models, float32 data, median of {args.repeats} ({torch.cuda.get_device_name(0)})",
             "rank   I   J   K  device_call_s  device_launch_s  dense_numpy_s  dense/device_call  device_us_per_model"]
    for rank, (I, J, K) in SIZES.items():
        Xs, models = problem(rank, n)
        device = torch.device("cuda")
        packed, _ = sim._pack([sim._Model(c) for c in models], device)
        X, row_ptr = pack_data(Xs, device)

        def launch():
            S, BtB, sse, norm = _engine.eval_tables(X, row_ptr, rank, packed)
            return _engine.eval_core(packed, I, I * J, K, rank, S, BtB)

        call_s = timed(lambda: ev.multistart_evaluation(Xs, models, method="device"), args.repeats)
        launch_s = timed(launch, args.repeats)
        dense_s = timed(lambda: dense_route(Xs, models[:m]), 1) * n / m
        # the two routes on the same models, before the times are believed
        got, want = ev.multistart_evaluation(Xs, models[:m], method="device"), dense_route(Xs, models[:m])
        assert np.abs(got.fit - [w[0] for w in want]).max() <= 1e-5, np.abs(got.fit - [w[0] for w in want]).max()
        assert (np.abs(got.slab_sse - [w[1] for w in want]) / [w[1] for w in want]).max() <= 1e-3
        lines.append(f"{rank:4d} {I:3d} {J:3d} {K:3d} {call_s:14.5f} {launch_s:16.5f}  ~{dense_s:12.4f} {dense_s / call_s:18.1f} {1e6 * launch_s / n:20.3f}")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
