"""One MoEMLP layer, forward + backward, at the 8x7b-proxy shape (hidden
2048, ffn 4096, 8 experts, top-2, N = 8192 tokens, bf16): the per-expert
loop dispatch against the fused kernels (moe.hip, K13) in one process,
alternating, so both see the same machine state.

Every number is a host clock around a window of `--repeats` calls that ends
in a device synchronise; the table gives median and spread (min..max) over
`--windows` windows per path after warm-up.  Besides the whole layer it
times the forward of the routing stage alone (torch chain vs `moe_route`,
both from the router's logits) and of the dispatch stages alone (permute +
combine around identity experts) on both paths.

    python tools/moe_bench.py [--tokens 8192] [--windows 10] [--repeats 5]

Needs a GPU: without one it fails instead of falling back.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from saturn_amd.models.mixtral import (
    PRESETS,
    MoEMLP,
    moe_experts_forward,
    route,
)
from saturn_amd.ops import moe_route, require_ext


def torch_route(logits, top_k, out_dtype):
    """The 5-kernel torch chain route() ran before moe_route."""
    logits = logits.float()
    probs = torch.softmax(logits, dim=-1)
    topv, topi = probs.topk(top_k, dim=-1)
    topv = topv / topv.sum(dim=-1, keepdim=True)
    return topv.to(out_dtype), topi


def windows(fns, n_windows, repeats, warmup):
    """Time the callables in `fns` alternately; returns ms per call for each
    window, {name: [ms, ...]}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(n_windows):
        for name, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(repeats):
                fn()
            torch.cuda.synchronize()
            out[name].append((time.perf_counter() - t0) / repeats * 1e3)
    return out


def row(label, ms):
    med = statistics.median(ms)
    return (f"{label:<34} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} "
            f"{max(ms) - min(ms):9.3f}"), med, max(ms) - min(ms)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tokens", type=int, default=8192)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.repeats < 5:
        ap.error("--repeats must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("moe_bench: no GPU visible; nothing is measured "
                         "on the CPU")
    require_ext()

    cfg = PRESETS["8x7b-proxy"]
    torch.manual_seed(0)
    dev, dt = "cuda", torch.bfloat16
    layer = MoEMLP(cfg).to(device=dev, dtype=dt)
    for m in layer.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.normal_(m.weight, std=0.02)
    N, H = args.tokens, cfg.n_embd
    x = torch.randn(1, N, H, device=dev, dtype=dt)
    gout = torch.randn(1, N, H, device=dev, dtype=dt)
    xf = x.view(N, H)

    def layer_step(dispatch):
        def fn():
            layer.dispatch = dispatch
            for p in layer.parameters():
                p.grad = None
            xi = x.detach().requires_grad_(True)
            layer(xi).backward(gout)
        return fn

    ident = [torch.nn.Identity() for _ in range(cfg.n_expert)]
    with torch.no_grad():
        weights, ids = route(layer.router, xf, cfg.top_k)
        logits = layer.router(xf)
        counts = torch.bincount(ids.reshape(-1).long(),
                                minlength=cfg.n_expert).tolist()

    def no_grad(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    print(f"MoEMLP layer, 8x7b-proxy: hidden {H}, ffn {cfg.ffn_dim}, "
          f"{cfg.n_expert} experts, top-{cfg.top_k}, N = {N} tokens, bf16")
    print(f"device: {torch.cuda.get_device_name(0)}; tokens per expert: "
          f"{counts}")
    print(f"{args.windows} windows per path, alternating; each window is "
          f"{args.repeats} calls then a synchronise; ms per call")
    print(f"{'':<34} {'median':>9} {'min':>9} {'max':>9} {'spread':>9}")

    res = windows({"loop": layer_step("loop"), "fused": layer_step("fused")},
                  args.windows, args.repeats, args.warmup)
    line, med_loop, sp_loop = row("layer fwd+bwd, dispatch=loop", res["loop"])
    print(line)
    line, med_fused, sp_fused = row("layer fwd+bwd, dispatch=fused",
                                    res["fused"])
    print(line)

    res = windows(
        {"torch": no_grad(lambda: torch_route(logits, cfg.top_k, dt)),
         "kernel": no_grad(lambda: moe_route(logits, cfg.top_k, dt))},
        args.windows, args.repeats * 4, args.warmup)
    print(row("routing fwd, torch chain", res["torch"])[0])
    print(row("routing fwd, moe_route", res["kernel"])[0])

    res = windows(
        {d: no_grad(lambda d=d: moe_experts_forward(xf, weights, ids, ident,
                                                    d))
         for d in ("loop", "fused")},
        args.windows, args.repeats * 4, args.warmup)
    print(row("dispatch fwd (identity), loop", res["loop"])[0])
    print(row("dispatch fwd (identity), fused", res["fused"])[0])

    spread = max(sp_loop, sp_fused)
    gain = med_loop - med_fused
    verdict = "fused is faster" if gain > spread else "no gain beyond spread"
    print(f"layer fwd+bwd: loop - fused = {gain:.3f} ms "
          f"({gain / med_loop * 100:.1f} % of loop), run-to-run spread "
          f"{spread:.3f} ms -> {verdict}")


if __name__ == "__main__":
    main()
