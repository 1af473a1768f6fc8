"""Cost of global gradient-norm clipping on GPT-J-6B-shaped bf16 gradients
(the bench model's parameter shapes: 28 layers, hidden 4096), in one
process, three arms alternating so all see the same machine state:

  off    FusedSGD.step() without max_grad_norm
  fused  FusedSGD.step() with max_grad_norm: grad_sqsum + clip_coef, then the
         SGD kernels scale g as they load it
  torch  torch.nn.utils.clip_grad_norm_ followed by the unclipped step

plus `grad_sqsum` alone and its achieved GB/s (bytes = 2 per gradient
element, read once), next to the GB/s of the read-write SGD sweep of the
`off` arm (6 bytes per element: p and g read, p written).

Every number is a host clock around a window of `--repeats` calls that ends
in a device synchronise; the table gives median and spread (min..max) over
`--windows` windows per arm after warm-up.

    python tools/clip_bench.py [--layers 28] [--windows 10] [--repeats 5]

Needs a GPU: without one it fails instead of falling back.
"""

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from saturn_amd.models.gptj import GPTJConfig, GPTJForCausalLM
from saturn_amd.ops import require_ext
from saturn_amd.ops.optim import FusedSGD


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
    print(f"{label:<40} {med:9.3f} {min(ms):9.3f} {max(ms):9.3f} "
          f"{max(ms) - min(ms):9.3f}")
    return med


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench: no GPU visible; nothing is measured "
                         "on the CPU")
    ext = require_ext()

    # the parameter shapes of the bench model, without building it
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in
                  GPTJForCausalLM(GPTJConfig(n_layer=args.layers)).parameters()]
    dev, dt = "cuda", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)

    def make_params():
        ps = []
        for s in shapes:
            p = torch.nn.Parameter(
                torch.randn(s, device=dev, generator=g).mul_(0.02).to(dt))
            p.grad = torch.randn(s, device=dev, generator=g).mul_(1e-3).to(dt)
            ps.append(p)
        return ps

    # lr = 0: the kernels do all their reads and writes, and the parameters
    # stay where they are over hundreds of timed steps
    params = make_params()
    grads = [p.grad for p in params]
    n_elem = sum(p.numel() for p in params)
    opt_off = FusedSGD(params, lr=0.0)
    opt_fused = FusedSGD(params, lr=0.0, max_grad_norm=1.0)
    partials = torch.empty(ext.grad_sqsum_slots(len(grads)),
                           dtype=torch.float32, device=dev)

    def torch_arm():
        # clip_grad_norm_ multiplies every gradient by the clamped
        # coefficient whatever its value (it never reads the norm on the
        # host), so the second pass is paid on every call
        torch.nn.utils.clip_grad_norm_(params, 1.0, foreach=True)
        opt_off.step()

    # one clipped step before anything rescales the gradients: its norm
    opt_fused.step()
    norm = float(opt_fused.last_grad_norm)

    print(f"GPT-J shapes, {args.layers} layers: {len(params)} tensors, "
          f"{n_elem / 1e9:.3f} G elements, bf16 "
          f"({2 * n_elem / 1e9:.2f} GB of gradients)")
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{args.windows} windows per arm, alternating; each window is "
          f"{args.repeats} calls then a synchronise; ms per call")
    print(f"{'':<40} {'median':>9} {'min':>9} {'max':>9} {'spread':>9}")

    # the torch arm leaves gradients of norm 1 behind; what the kernels of
    # the other arms cost does not depend on the values they read
    res = windows({"off": opt_off.step, "fused": opt_fused.step,
                   "torch": torch_arm},
                  args.windows, args.repeats, args.warmup)
    med_off = row("FusedSGD.step(), clipping off", res["off"])
    med_fused = row("FusedSGD.step(), max_grad_norm", res["fused"])
    med_torch = row("clip_grad_norm_ + FusedSGD.step()", res["torch"])
    spread = max(max(v) - min(v) for v in res.values())

    res = windows({"sqsum": lambda: ext.grad_sqsum(grads, partials)},
                  args.windows, args.repeats * 4, args.warmup)
    med_sq = row("grad_sqsum alone", res["sqsum"])

    gbs_sq = 2 * n_elem / (med_sq * 1e-3) / 1e9
    gbs_sgd = 6 * n_elem / (med_off * 1e-3) / 1e9
    print(f"grad_sqsum: {gbs_sq:.0f} GB/s read-only (2 B/element); SGD sweep "
          f"of the off arm: {gbs_sgd:.0f} GB/s (6 B/element: p, g read, "
          f"p written)")
    print(f"gradient norm before the first step {norm:.4g}, max_grad_norm "
          f"1.0 -> coefficient {min(1.0, 1.0 / (norm + 1e-6)):.4g}")
    print(f"fused clipping costs {med_fused - med_off:.3f} ms per step over "
          f"off; the torch route costs {med_torch - med_off:.3f} ms; "
          f"largest run-to-run spread of an arm {spread:.3f} ms")


if __name__ == "__main__":
    main()
