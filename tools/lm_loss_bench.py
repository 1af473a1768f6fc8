"""lm_head + cross-entropy, forward + backward, at the two bench shapes
(GPT-J-6B: B16 T512 K4096 V50400 with bias; Llama-3-8B: B4 T2048 K4096
V128256): the fused path (lm_loss.hip, K18: no logits, one vocabulary chunk
of dlogits) against the materialised one (F.linear + fused_cross_entropy) in
one process, alternating, so both see the same machine state.  The fused
path runs at its default chunk width and at `--chunks` other widths.

Every time is a host clock around a window of `--repeats` calls that ends in
a device synchronise; the table gives the median and [min..max] over
`--windows` windows per arm after warm-up, and TF/s = GEMM operations of the
arm (2 N K V each: 3 materialised, 4 fused) over the median.  Peak memory is
`max_memory_allocated` of one call above what was allocated before it
(inputs and parameters resident, gradients freed).

    python tools/lm_loss_bench.py [--windows 10] [--repeats 5] [--chunks 1024,16384]

Needs a GPU: without one it fails instead of falling back.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from saturn_amd.ops import fused_linear_cross_entropy, require_ext
from saturn_amd.ops.functional import fused_cross_entropy

SHAPES = {
    "gptj-6b": dict(B=16, T=512, K=4096, V=50400, bias=True),
    "llama-3-8b": dict(B=4, T=2048, K=4096, V=128256, bias=False),
}


def make_arms(s, chunks):
    g = torch.Generator().manual_seed(0)
    h = torch.randn(s["B"], s["T"], s["K"], generator=g).bfloat16().cuda()
    w = (torch.randn(s["V"], s["K"], generator=g) * 0.02).bfloat16().cuda()
    b = torch.zeros(s["V"]).bfloat16().cuda() if s["bias"] else None
    x = torch.randint(0, s["V"], (s["B"], s["T"]), generator=g).cuda()
    leaves = [t.requires_grad_(True) for t in (h, w, b) if t is not None]

    def call(loss_fn):
        def fn():
            loss_fn().backward()
            for t in leaves:
                t.grad = None
        return fn

    arms = {"materialised": (3, call(
        lambda: fused_cross_entropy(F.linear(h, w, b), x)))}
    for c in [None] + chunks:
        name = "fused, chunk " + ("default" if c is None else str(c))
        arms[name] = (4, call(
            lambda c=c: fused_linear_cross_entropy(h, w, b, x, chunk=c)))
    return arms


def peak_above_baseline(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunks", default="1024,16384",
                    help="further chunk widths of the fused arm (multiples "
                         "of 128), comma-separated; '' for none")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lm_loss_bench needs a GPU")
    require_ext()
    chunks = [int(c) for c in args.chunks.split(",") if c]

    print(f"device: {torch.cuda.get_device_name(0)}; {args.windows} windows "
          f"per arm, alternating; each window is {args.repeats} calls then a "
          "synchronise; ms per call, forward + backward")
    for name in args.shapes.split(","):
        s = SHAPES[name]
        N = s["B"] * s["T"]
        arms = make_arms(s, chunks)
        for _ in range(args.warmup):
            for _, fn in arms.values():
                fn()
        peaks = {a: peak_above_baseline(fn) for a, (_, fn) in arms.items()}
        ms = {a: [] for a in arms}
        for _ in range(args.windows):
            for a, (_, fn) in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.repeats):
                    fn()
                torch.cuda.synchronize()
                ms[a].append((time.perf_counter() - t0) / args.repeats * 1e3)
        print(f"\n{name}: N = {N} rows, K = {s['K']}, V = {s['V']}, "
              f"bias = {s['bias']}; one [N, V] bf16 tensor = "
              f"{N * s['V'] * 2 / 1e9:.2f} GB")
        print(f"{'arm':<24} {'median':>9}  [{'min':>8} .. {'max':>8}]  "
              f"{'TF/s':>7}  {'peak above baseline':>20}")
        med0 = statistics.median(ms["materialised"])
        for a, (gemms, _) in arms.items():
            med = statistics.median(ms[a])
            tf = gemms * 2.0 * N * s["K"] * s["V"] / (med * 1e-3) / 1e12
            print(f"{a:<24} {med:9.3f}  [{min(ms[a]):8.3f} .. "
                  f"{max(ms[a]):8.3f}]  {tf:7.1f}  "
                  f"{peaks[a] / 1e9:17.3f} GB")
        for a in arms:
            if a != "materialised":
                med = statistics.median(ms[a])
                print(f"{a}: {med / med0:.2f} x the materialised time, "
                      f"{peaks[a] / peaks['materialised']:.2f} x its peak")
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
