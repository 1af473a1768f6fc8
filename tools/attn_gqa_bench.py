"""GQA attention backward microbenchmark: the two dK/dV routes of attn_bwd,
dkv_route=0 (one block per q head, fp32 atomics, fill and cast) against
dkv_route=1 (attn_bwd_kernel<..., GROUP>: one block per 64 keys of a KV head).

    python tools/attn_gqa_bench.py [--cases B,H,Hkv,T,D[,window] ...]

The two routes alternate in one process: 10 windows of 5 backward calls
(delta + dQ + dK/dV, with the atomic route's fills and casts) each ending in a
synchronise, median and min..max reported.  `blocks` is the group route's grid,
B * Hkv * T/64, the quantity the auto rule of attn_bwd bounds.  Prints one JSON
line per case.
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
CASES = ["4,32,8,2048,128", "1,32,8,2048,128", "4,32,8,512,128",
         "4,32,8,2048,128,1024"]
ROUTES = {"atomic": 0, "group": 1}


def timed(fn):
    torch.cuda.synchronize()
    t0 = timer()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (timer() - t0) / CALLS


def run(ext, B, H, Hkv, T, D, window=None):
    torch.manual_seed(0)
    q = torch.randn(B, H, T, D, device="cuda", dtype=torch.bfloat16)
    k = torch.randn(B, Hkv, T, D, device="cuda", dtype=torch.bfloat16)
    v, do = torch.randn_like(k), torch.randn_like(q)
    lo = None if window is None else window_lo(T, window, q.device)
    o, lse = ext.attn_fwd(q, k, v, True, T, kv_lo=lo)
    bwd = {name: (lambda r=r: ext.attn_bwd(do, q, k, v, o, lse, True, T,
                                           kv_lo=lo, dkv_route=r))
           for name, r in ROUTES.items()}
    # the two routes must tell the same story before their times are compared
    ga, gg = bwd["atomic"](), bwd["group"]()
    diff = [float((a.float() - g.float()).abs().max()) for a, g in zip(ga, gg)]
    # ramp the clocks on the work to be measured
    for _ in range(3):
        for name in bwd:
            timed(bwd[name])
    times = {name: [] for name in bwd}
    for _ in range(ROUNDS):
        for name in bwd:
            times[name].append(timed(bwd[name]) * 1e6)

    res = {"shape": [B, H, Hkv, T, D], "window": window, "causal": True,
           "rounds": ROUNDS, "calls": CALLS, "blocks": B * Hkv * (T // 64),
           "path": ext.attn_dispatch(T, D, has_lo=lo is not None, gqa=True),
           "max_abs_diff_dq_dk_dv": diff, "arms": {}}
    for name, ts in times.items():
        res["arms"][name] = {"median_us": round(statistics.median(ts), 1),
                             "min_us": round(min(ts), 1),
                             "max_us": round(max(ts), 1)}
    a, g = res["arms"]["atomic"], res["arms"]["group"]
    res["ratio"] = round(g["median_us"] / a["median_us"], 3)
    # the rule of attn_bwd's auto mode: no worse than the atomic route's
    # median plus this run's own spread
    res["group_no_worse"] = g["median_us"] <= a["median_us"] + (
        a["max_us"] - a["min_us"])
    w = "" if window is None else f" window={window}"
    print(f"B{B} H{H} Hkv{Hkv} T{T} D{D}{w} bf16 causal, blocks "
          f"{res['blocks']}, {ROUNDS} windows x {CALLS} calls, bwd median "
          f"[min..max] us")
    for name, row in res["arms"].items():
        print(f"  {name:>6}: {row['median_us']:9.1f} [{row['min_us']:.1f}.."
              f"{row['max_us']:.1f}]")
    print(f"  group / atomic x{res['ratio']:.3f}  no worse: "
          f"{res['group_no_worse']}", flush=True)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=CASES,
                    help="B,H,Hkv,T,D[,window] per case")
    args = ap.parse_args()
    ext = require_ext()
    for c in args.cases:
        run(ext, *(int(x) for x in c.split(",")))


if __name__ == "__main__":
    main()
