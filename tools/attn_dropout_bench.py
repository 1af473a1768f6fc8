"""Attention-dropout microbenchmark: attn_fwd / attn_bwd with dropout_p = 0.1
(the DROP instantiations) against the plain call (the unchanged DROP = false
path) on the same inputs.

    python tools/attn_dropout_bench.py [--shapes B,H,T,D ...] [--p 0.1]

The two arms alternate in one process: 10 windows of 5 calls each ending in a
synchronise, median and min..max reported, forward and backward (delta + dQ +
dK/dV) apart.  Beside each ratio dropout / plain stand the 64-bit hashes the
kernels compute per score: v1 forward 1, v2 forward 1/4, dQ 1/4, dK/dV 1/4.
Prints one JSON line per shape.
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

ROUNDS = 10
CALLS = 5
SEED = 20261021


def timed(fn):
    torch.cuda.synchronize()
    t0 = timer()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (timer() - t0) / CALLS


def hashes_per_score(path):
    """64-bit hashes per attention score in (forward, backward kernels)."""
    fwd = 0.25 if path.startswith("attn_fwd_v2_kernel") else 1.0
    return {"fwd": fwd, "bwd": 0.25 + 0.25}


def run(ext, B, H, T, D, p, causal=True):
    torch.manual_seed(0)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k, v, do = torch.randn_like(q), torch.randn_like(q), torch.randn_like(q)
    arms = {"plain": 0.0, f"p{p}": p}
    fwd, bwd = {}, {}
    for name, pp in arms.items():
        fwd[name] = (lambda pp=pp: ext.attn_fwd(q, k, v, causal, T,
                                                dropout_p=pp, seed=SEED))
        o, lse = fwd[name]()
        bwd[name] = (lambda pp=pp, o=o, lse=lse:
                     ext.attn_bwd(do, q, k, v, o, lse, causal, T,
                                  dropout_p=pp, seed=SEED))
    # ramp the clocks on the work to be measured
    for _ in range(3):
        for name in arms:
            timed(fwd[name])
            timed(bwd[name])

    times = {(ph, n): [] for ph in ("fwd", "bwd") for n in arms}
    for _ in range(ROUNDS):
        for name in arms:
            times["fwd", name].append(timed(fwd[name]))
            times["bwd", name].append(timed(bwd[name]))

    paths = {"plain": ext.attn_dispatch(T, D),
             "dropout": ext.attn_dispatch(T, D, has_drop=True)}
    res = {"shape": [B, H, T, D], "causal": causal, "p": p, "rounds": ROUNDS,
           "calls": CALLS, "paths": paths,
           "hashes_per_score": hashes_per_score(paths["dropout"]), "arms": {}}
    print(f"B{B} H{H} T{T} D{D} bf16 causal={causal}, {ROUNDS} windows x "
          f"{CALLS} calls, median [min..max] us")
    for name in arms:
        row = {}
        for ph in ("fwd", "bwd"):
            ts = [t * 1e6 for t in times[ph, name]]
            base = statistics.median(times[ph, "plain"]) * 1e6
            row[ph] = {"median_us": round(statistics.median(ts), 1),
                       "min_us": round(min(ts), 1), "max_us": round(max(ts), 1),
                       "ratio": round(statistics.median(ts) / base, 3)}
        res["arms"][name] = row
        print(f"  {name:>6}: " + " | ".join(
            f"{ph} {row[ph]['median_us']:9.1f} [{row[ph]['min_us']:.1f}.."
            f"{row[ph]['max_us']:.1f}] x{row[ph]['ratio']:.3f}"
            for ph in ("fwd", "bwd")), flush=True)
    print("  fwd:", paths["dropout"].split()[0], "hashes/score",
          res["hashes_per_score"]["fwd"], "| bwd hashes/score",
          res["hashes_per_score"]["bwd"], flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4,32,2048,128",
                                                    "16,16,512,256"],
                    help="B,H,T,D per shape")
    ap.add_argument("--p", type=float, default=0.1)
    args = ap.parse_args()
    ext = require_ext()
    for s in args.shapes:
        B, H, T, D = (int(x) for x in s.split(","))
        run(ext, B, H, T, D, args.p)


if __name__ == "__main__":
    main()
