"""Wall time of parafac2_project: new matrices fitted to a fixed PARAFAC2 model, at the semiconductor example's shape (J 110,
K 21, rank 2) and at 64 x 64, rank 16, for 16, 1024 and 16384 new matrices.

    python tools/projection_rate.py [--out profiles/projection_rate.txt] [--repeats 7] [--host-matrices 256]

"numpy" is the whole parafac2_project(method="device") call from a list of NumPy matrices (packing, upload, the entry, download,
splitting), "packed" the same call on a PackedMatrices resident on the device, "entry" _engine.pf2_project alone on device
inputs, synchronised, and "host" parafac2_project(method="host") on the same NumPy matrices.  Each is the median of --repeats
repetitions after a warm-up, the four taken in turn within a repetition.  The host loop is measured on at most --host-matrices
matrices and scaled by the number of matrices (marked "~"): the matrices are independent, one after the other.  The two methods
are checked against each other before a time is reported."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from matcouply_amd import _engine, projection as pj  # noqa: E402
from matcouply_amd.decomposition import PackedMatrices  # noqa: E402

SHAPES = [(110, 21, 2), (64, 64, 16)]  # (J, K, rank)
SIZES = [16, 1024, 16384]


def problem(J, K, rank, n, seed=0):
    """a model with factors of condition number 2 and n matrices that follow it, plus noise of relative norm 0.3"""
    rng = np.random.RandomState(seed)

    def factor(rows):
        U, V = np.linalg.qr(rng.standard_normal((rows, rank)))[0], np.linalg.qr(rng.standard_normal((rank, rank)))[0]
        return ((U * np.linspace(1.0, 2.0, rank)) @ V.T).astype(np.float32)

    Delta, C = factor(rank), factor(K)
    Xs = []
    for _ in range(n):
        P = np.linalg.qr(rng.standard_normal((J, rank)))[0]
        X = (P @ Delta * rng.uniform(0.5, 1.5, rank)) @ C.T
        E = rng.standard_normal(X.shape)
        Xs.append((X + 0.3 * np.linalg.norm(X) / np.linalg.norm(E) * E).astype(np.float32))
    return Delta, C, Xs


def medians(fns, repeats):
    for fn in fns:  # warm-up: library load, code objects, allocator
        fn()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    return [statistics.median(t) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "projection_rate.txt"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-matrices", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("projection_rate.py measures on an MI355X: no device is visible")
    lines = [f"parafac2_project wall time, float32 data, default tolerances, median of {args.repeats} ({torch.cuda.get_device_name(0)})",
             "   J   K rank matrices  numpy_call_s  packed_call_s      entry_s       host_s  host/numpy_call  entry_us_per_matrix  mean_n_iter"]
    device = torch.device("cuda")
    for J, K, rank in SHAPES:
        Delta, C, all_Xs = problem(J, K, rank, max(SIZES))
        model = (Delta, C)
        up = lambda M: torch.from_numpy(np.ascontiguousarray(M, dtype=np.float64)).to(device)
        for n in SIZES:
            Xs = all_Xs[:n]
            m = min(n, args.host_matrices)
            row_ptr = np.arange(n + 1, dtype=np.int64) * J
            packed = PackedMatrices(torch.from_numpy(np.concatenate(Xs, 0)).to(device), row_ptr)
            dev_in = (up(Delta), up(C), up(np.ones((n, rank))))
            # the two methods on the same matrices, before the times are believed
            got, want = pj.parafac2_project(Xs[:m], model, method="device"), pj.parafac2_project(Xs[:m], model, method="host")
            worst = np.abs(got.cmf[1][0] - want.cmf[1][0]).max() / np.abs(want.cmf[1][0]).max()
            assert worst <= 1e-4, worst
            numpy_s, packed_s, entry_s, host_s = medians([
                lambda: pj.parafac2_project(Xs, model, method="device"),
                lambda: pj.parafac2_project(packed, model, method="device"),
                lambda: _engine.pf2_project(packed.X, row_ptr, rank, *dev_in, 100, 1e-8, 1e-13, False),
                lambda: pj.parafac2_project(Xs[:m], model, method="host")], args.repeats)
            host_s *= n / m
            mark = "~" if m < n else " "
            lines.append(f"{J:4d} {K:3d} {rank:4d} {n:8d} {numpy_s:13.5f} {packed_s:14.5f} {entry_s:12.5f} {mark}{host_s:11.4f} "
                         f"{host_s / numpy_s:16.1f} {1e6 * entry_s / n:20.3f} {got.n_iter.mean():12.1f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
