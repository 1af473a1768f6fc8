"""Reference and error floor for the fused lm_head + cross-entropy (K18),
computed once per problem and shared (read-only).

`ref`   the bf16-rounded inputs in fp64: F.linear + cross_entropy(sum)/valid,
        gradients by autograd.
`base`  the same in fp32 torch ops with the kernels' roundings by design: fp32
        logits up to the exp, dl rounded once to bf16, dh / dW / dbias one
        rounding of an fp32 sum each.
`plain` loss and lse of a plain fp32 torch composition, for the LSE rule:
        8 x its error against fp64 + 1e-6.
Inputs h ~ randn, W ~ 2 randn / sqrt(K) (logits with spread, no negligible
probability); every 7th target is ignore_index."""

import functools
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

IGNORE = -100


def shifted(targets, shift):
    """The per-position targets the loss scores, flat."""
    if not shift:
        return targets.reshape(-1)
    tg = torch.full_like(targets, IGNORE)
    tg[:, :-1] = targets[:, 1:]
    return tg.reshape(-1)


def _grads(h, w, b, tg, dt):
    """[loss, lse, dh, dW, dbias?] in dtype dt; dt = fp32 makes the floor."""
    exact = dt == torch.float64
    rnd = (lambda t: t) if exact else (lambda t: t.bfloat16().float())
    h2, w2 = h.reshape(-1, h.shape[-1]).to(dt), w.to(dt)
    b2 = None if b is None else b.to(dt)
    leaves = [t.requires_grad_(exact) for t in (h2, w2, b2) if t is not None]
    logits = F.linear(h2, w2, b2)
    lse = torch.logsumexp(logits, dim=-1)
    live = tg != IGNORE
    valid = max(int(live.sum()), 1)
    loss = F.cross_entropy(logits, tg, ignore_index=IGNORE,
                           reduction="sum") / valid
    if exact:
        grads = torch.autograd.grad(loss, leaves)
        return [loss.detach(), lse.detach(), *grads]
    onehot = F.one_hot(tg.clamp(min=0), logits.shape[1]).to(dt)
    dl = rnd((torch.exp(logits - lse[:, None]) - onehot)
             * (live.to(dt) / valid)[:, None])
    out = [loss, lse, rnd(dl @ w2), rnd(dl.t() @ h2)]
    return out + ([] if b is None else [rnd(dl.sum(0))])


@functools.lru_cache(maxsize=None)
def problem(B, T, K, V, bias, shift):
    g = torch.Generator().manual_seed(18)
    h = torch.randn(B, T, K, generator=g).bfloat16()
    w = (2.0 * torch.randn(V, K, generator=g) / math.sqrt(K)).bfloat16()
    b = torch.randn(V, generator=g).bfloat16() if bias else None
    targets = torch.randint(0, V, (B, T), generator=g)
    targets.view(-1)[::7] = IGNORE
    tg = shifted(targets, shift)
    ref = _grads(h, w, b, tg, torch.float64)
    h32 = h.float().reshape(-1, K)
    lg = F.linear(h32, w.float(), None if b is None else b.float())
    plain = [F.cross_entropy(lg, tg, ignore_index=IGNORE),
             torch.logsumexp(lg, dim=-1)]
    tol = [8.0 * (p.double() - r).abs().max().item() + 1e-6
           for p, r in zip(plain, ref)]
    return SimpleNamespace(h=h, w=w, b=b, targets=targets, tg=tg, shift=shift,
                           ref=ref, base=_grads(h, w, b, tg, torch.float32),
                           loss_tol=tol[0], lse_tol=tol[1])


def run(p, chunk, device="cuda"):
    """fused_linear_cross_entropy forward + backward on fresh leaves:
    [loss, dh, dW, dbias?]."""
    from saturn_amd.ops import fused_linear_cross_entropy

    leaves = [t.to(device).requires_grad_(True)
              for t in (p.h, p.w, p.b) if t is not None]
    loss = fused_linear_cross_entropy(
        leaves[0], leaves[1], leaves[2] if p.b is not None else None,
        p.targets.to(device), shift=p.shift, ignore_index=IGNORE, chunk=chunk)
    loss.backward()
    return [loss.detach()] + [t.grad for t in leaves]
