"""Sliding-window attention microbenchmark: attn_fwd / attn_bwd with a kv_lo
window bound against the plain causal call (the unchanged LO = false path).

    python tools/attn_window_bench.py [--shape B H T D] [--windows 1024 4096]

The arms (plain, one per window) alternate in one process: 10 windows of 5
calls each ending in a synchronise, median and min..max reported, forward
and backward apart.  Beside each measured ratio window / plain stands the
ratio of visited key tiles, about 2W/T - (W/T)^2.  Prints one JSON line at
the end.
"""

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from timeit import default_timer as timer

import torch

from saturn_amd.ops import require_ext
from saturn_amd.ops.flash import window_lo

ROUNDS = 10
CALLS = 5


def timed(fn):
    torch.cuda.synchronize()
    t0 = timer()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (timer() - t0) / CALLS


def tile_ratio(T, W):
    """Visited (row, key) area of a window over the causal triangle's."""
    if W >= T:
        return 1.0
    return (W * (W + 1) / 2 + (T - W) * W) / (T * (T + 1) / 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=4, default=[4, 32, 8192, 128],
                    metavar=("B", "H", "T", "D"))
    ap.add_argument("--windows", type=int, nargs="+", default=[1024, 4096])
    args = ap.parse_args()
    B, H, T, D = args.shape
    ext = require_ext()
    torch.manual_seed(0)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k, v, do = torch.randn_like(q), torch.randn_like(q), torch.randn_like(q)

    arms = {"plain": None}
    for W in args.windows:
        arms[f"W{W}"] = window_lo(T, W, q.device)
    fwd, bwd = {}, {}
    for name, lo in arms.items():
        fwd[name] = (lambda lo=lo: ext.attn_fwd(q, k, v, True, T, kv_lo=lo))
        o, lse = fwd[name]()
        bwd[name] = (lambda lo=lo, o=o, lse=lse:
                     ext.attn_bwd(do, q, k, v, o, lse, True, T, kv_lo=lo))
    # ramp the clocks on the work to be measured
    for _ in range(3):
        for name in arms:
            timed(fwd[name])
            timed(bwd[name])

    times = {(p, n): [] for p in ("fwd", "bwd") for n in arms}
    for _ in range(ROUNDS):
        for name in arms:
            times["fwd", name].append(timed(fwd[name]))
            times["bwd", name].append(timed(bwd[name]))

    res = {"shape": [B, H, T, D], "rounds": ROUNDS, "calls": CALLS,
           "paths": {"plain": ext.attn_dispatch(T, D),
                     "window": ext.attn_dispatch(T, D, has_lo=True)},
           "arms": {}}
    print(f"B{B} H{H} T{T} D{D} bf16, {ROUNDS} windows x {CALLS} calls, "
          "median [min..max] us")
    for name in arms:
        row = {}
        for p in ("fwd", "bwd"):
            ts = [t * 1e6 for t in times[p, name]]
            base = statistics.median(times[p, "plain"]) * 1e6
            row[p] = {"median_us": round(statistics.median(ts), 1),
                      "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                      "ratio": round(statistics.median(ts) / base, 3)}
        W = int(name[1:]) if name != "plain" else T
        row["tile_ratio"] = round(tile_ratio(T, W), 3)
        res["arms"][name] = row
        print(f"  {name:>6}: " + " | ".join(
            f"{p} {row[p]['median_us']:9.1f} [{row[p]['min_us']:.1f}.."
            f"{row[p]['max_us']:.1f}] x{row[p]['ratio']:.3f}"
            for p in ("fwd", "bwd")) + f" | tiles x{row['tile_ratio']:.3f}",
            flush=True)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
