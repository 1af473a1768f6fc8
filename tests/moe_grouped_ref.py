"""Reference for the grouped expert GEMMs (K17), computed once per problem:
`ref` is the bf16-rounded inputs multiplied in fp64, `base` the same product
as an fp32 matmul rounded once to bf16 (the kernel's roundings by design)."""

import functools

import torch

# segments off every tile boundary, straddling tiles, two empty experts, a
# single row and an exact multiple of 64; P = 644
COUNTS = (1, 0, 129, 63, 257, 0, 64, 130)


@functools.lru_cache(maxsize=None)
def problem(counts, K, Nout):
    """(xs, ws, dy, ref, base): ref/base are lists [y, dx, dw_0, ...]."""
    g = torch.Generator().manual_seed(17)
    P = sum(counts)
    xs = torch.randn(P, K, generator=g).bfloat16()
    ws = [torch.randn(Nout, K, generator=g).bfloat16() for _ in counts]
    dy = torch.randn(P, Nout, generator=g).bfloat16()

    def products(dt):
        rnd = (lambda t: t) if dt == torch.float64 else torch.Tensor.bfloat16
        xe, de = xs.to(dt).split(counts), dy.to(dt).split(counts)
        y = torch.cat([rnd(x @ w.to(dt).t()) for x, w in zip(xe, ws)])
        dx = torch.cat([rnd(d @ w.to(dt)) for d, w in zip(de, ws)])
        return [y, dx] + [rnd(d.t() @ x) for d, x in zip(de, xe)]

    return xs, ws, dy, products(torch.float64), products(torch.float32)


def run(xs, counts, ws, dy, device):
    """moe_grouped_linear forward + backward on fresh leaves of `device`:
    [y, dx, dw_0, ...]."""
    from saturn_amd.ops import moe_grouped_linear

    xs = xs.to(device).detach().requires_grad_(True)
    ws = [w.to(device).detach().requires_grad_(True) for w in ws]
    cnt = torch.tensor(counts, dtype=torch.int32, device=device)
    y = moe_grouped_linear(xs, cnt, ws)
    y.backward(dy.to(device))
    return [y.detach(), xs.grad] + [w.grad for w in ws]
