"""fp32 X against 16-bit X of the same data, alternating in one process: per-site kernel time from the engine's own launch-site
timers (PROF_SWEEP / PROF_XC / PROF_XT) and the step rate.  The fp32 twin runs on X16.float() (the exact upcast), so both
runs compute the same numbers and only the bytes of X differ.

    python tools/x16_rate.py --configs c3,c4 [--dtype bfloat16] [--reps 5] [--steps 100] [--out profiles/x16_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402
from matcouply_amd import _engine  # noqa: E402

SITES = [("sweep", _engine.PROF_SWEEP), ("X C", _engine.PROF_XC), ("X^T", _engine.PROF_XT)]


def measure(eng, steps):
    """(us per step, {site: us per launch}) of `steps` outer iterations"""
    eng.profile_enable(steps * 4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.iterate(steps)
    torch.cuda.synchronize()
    step_us = 1e6 * (time.perf_counter() - t0) / steps
    sites = {}
    for name, s in SITES:
        ms, n = eng.profile_read(s)
        if n > 0:
            sites[name] = 1e3 * ms / n
    return step_us, sites


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="c3,c4")
    ap.add_argument("--dtype", default="bfloat16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = [f"tools/x16_rate.py --configs {a.configs} --dtype {a.dtype} --reps {a.reps} --steps {a.steps}",
             f"device: {torch.cuda.get_device_name(dev)}; fastest of {a.reps} alternating repetitions, same process", ""]
    for name in a.configs.split(","):
        cfg = dict(bench.CONFIGS[name])
        X, row_ptr, I_loc = bench.make_shard(cfg, 0, 1, dev)
        X16 = X.to(getattr(torch, a.dtype))
        del X
        X32 = X16.float()
        engs = {"fp32": bench.make_engine(cfg, X32, row_ptr, I_loc, 0, dev), a.dtype: bench.make_engine(cfg, X16, row_ptr, I_loc, 0, dev)}
        for e in engs.values():
            e.iterate(10)
        best = {k: (float("inf"), {}) for k in engs}
        for _ in range(a.reps):
            for k, e in engs.items():  # alternating: a neighbour's load hits both forms alike
                step, sites = measure(e, a.steps)
                b_step, b_sites = best[k]
                best[k] = (min(step, b_step), {s: min(v, b_sites.get(s, float("inf"))) for s, v in sites.items()})
        lines.append(f"{cfg['desc']}  (X: {X32.numel() * 4 / 1e6:.0f} MB fp32, {X16.numel() * 2 / 1e6:.0f} MB {a.dtype})")
        for k, e in engs.items():
            step, sites = best[k]
            variants = "; ".join(f"{s}: {e.kernel_variant(p)}" for s, p in SITES if e.kernel_variant(p))
            lines.append(f"  {k:9s} step {step:8.1f} us ({1e6 / step:7.0f} it/s)  " +
                         "  ".join(f"{s} {v:8.1f} us" for s, v in sites.items()) + f"   [{variants}]")
        (s32, t32), (s16, t16) = best["fp32"], best[a.dtype]
        lines.append(f"  ratio 16-bit / fp32: step {s16 / s32:.3f}  " +
                     "  ".join(f"{s} {t16[s] / t32[s]:.3f}" for s in t32 if s in t16))
        lines.append("")
        for e in engs.values():
            e.close()
        del engs, X16, X32
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
