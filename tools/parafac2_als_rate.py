"""Rate of parafac2_als on one MI355X -> profiles/parafac2_als_rate.txt.

    python tools/parafac2_als_rate.py [--out profiles/parafac2_als_rate.txt]

Per-iteration time (difference of the median wall times of runs with 22 and 2 iterations at tol = 0, svd start) at the config-3
shape (I=1024, J=512, K=256, rank 16) and the config-4 shape (ragged J_i in [128, 1024]), n_iter_parafac 1 and 5, priced against
the streaming-read rate of X; and the wall time of the example-sized call (nn_modes=[0], tol=1e-9, n_iter_max=10_000)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matcouply_amd import _engine  # noqa: E402
from matcouply_amd.decomposition import PackedMatrices, parafac2_als  # noqa: E402


def packed(I, J, K, r, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    J = np.asarray(J)
    row_ptr = np.concatenate([[0], np.cumsum(J)]).astype(np.int64)
    C = torch.rand((K, r), device="cuda", generator=g)
    X = torch.empty((int(row_ptr[-1]), K), device="cuda")
    for i in range(I):
        Bi = torch.rand((int(J[i]), r), device="cuda", generator=g) * torch.rand(r, device="cuda", generator=g)
        X[row_ptr[i]: row_ptr[i + 1]] = Bi @ C.T
    X += 0.01 * X.std() * torch.randn(X.shape, device="cuda", generator=g)
    return PackedMatrices(X.contiguous(), row_ptr)


def per_iteration(p, r, n_iter_parafac, iterations=20, reps=3):
    def med(n):
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parafac2_als(p, r, n_iter_max=n, tol=0, init="svd", n_iter_parafac=n_iter_parafac)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts))

    med(2)
    return (med(2 + iterations) - med(2)) / iterations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "parafac2_als_rate.txt"))
    args = ap.parse_args()
    out = [f"# parafac2_als rate on {torch.cuda.get_device_name()} (tools/parafac2_als_rate.py)"]
    rng = np.random.RandomState(0)
    shapes = {"config-3 (I=1024, J=512, K=256, r=16)": (1024, [512] * 1024, 256, 16),
              "config-4 shape (I=1024, J_i in [128, 1024], K=256, r=16)": (1024, list(rng.randint(128, 1025, size=1024)), 256, 16)}
    for name, (I, J, K, r) in shapes.items():
        p = packed(I, J, K, r)
        read_s = p.X.numel() * 4 / (_engine.read_bandwidth(p.X) * 1e9)
        out.append(f"{name}: one read of X {read_s * 1e6:.1f} us")
        for nip in (1, 5):
            t = per_iteration(p, r, nip)
            out.append(f"  n_iter_parafac={nip}: {t * 1e6:.1f} us per iteration = 2 reads + {(t - 2 * read_s) * 1e6:.1f} us")
        del p
        torch.cuda.empty_cache()
    # the example-sized call: the reference's semiconductor-etch example fits parafac2(X, 2, n_iter_max=10_000, nn_modes=[0],
    # tol=1e-9); stand-in data of that order of size (I=108 wafers, J_i in [100, 120] time points, K=21 channels)
    J = rng.randint(100, 121, size=108)
    mats = [rng.uniform(size=(int(j), 21)).astype(np.float32) for j in J]
    mats = [torch.from_numpy(m).cuda() for m in mats]
    parafac2_als(mats, 2, n_iter_max=10, nn_modes=[0], random_state=0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, errs = parafac2_als(mats, 2, n_iter_max=10_000, tol=1e-9, nn_modes=[0], random_state=0, return_errors=True)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out.append(f"example-sized call (I=108, J_i in [100, 120], K=21, rank 2, nn_modes=[0], tol=1e-9): {len(errs)} iterations, "
               f"{wall:.2f} s wall ({wall / len(errs) * 1e6:.0f} us per iteration), final error {errs[-1]:.6f}")
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
