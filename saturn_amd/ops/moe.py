"""MoE routing and token dispatch ops (K13) with pure-torch fallbacks.

Four ops cover everything around the expert GEMMs of the Mixtral path:

``moe_route``    softmax over all experts in fp32, top-k, renormalise
``moe_sort``     stable counting sort of the (token, slot) pairs by expert
``moe_permute``  gather token rows into expert order
``moe_combine``  weighted sum of each token's k expert rows

GPU tensors inside the kernels' envelope (``n_expert <= 64``,
``top_k <= min(8, n_expert)``, ``hidden % 8 == 0``, rows in bf16/fp16/fp32,
``N * top_k < 2**31``) go to ``saturn_amd._C`` and raise loudly when the
extension is missing.  Everything else (CPU, or outside the envelope) uses a
torch fallback with the same contract:

* ids are ordered by descending probability and **ties go to the lower
  expert index** (stable descending sort of the fp32 logits);
* ``order == argsort(ids.flatten(), stable=True)``, ``pos`` is its inverse,
  ``counts == bincount(ids.flatten(), minlength=n_expert)``; all int32;
* reductions over a token's k rows run in fp32, slot-ascending, and round
  once, so results are bitwise reproducible (no float atomics anywhere).
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from saturn_amd.ops import require_ext

MAX_EXPERTS = 64
MAX_TOP_K = 8
_ROW_DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _topk_ok(n: int, n_expert: int, top_k: int) -> bool:
    return (
        n > 0
        and 1 <= n_expert <= MAX_EXPERTS
        and 1 <= top_k <= min(MAX_TOP_K, n_expert)
        and n * top_k < 2**31
    )


def _rows_ok(rows: torch.Tensor, n: int, top_k: int) -> bool:
    return (
        rows.is_cuda
        and rows.dim() == 2
        and rows.dtype in _ROW_DTYPES
        and rows.shape[1] % 8 == 0
        and n > 0
        and 1 <= top_k <= MAX_TOP_K
        and n * top_k < 2**31
    )


# ---------------------------------------------------------------------------
# routing
# ---------------------------------------------------------------------------
class _RouteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, top_k, out_dtype):
        ext = require_ext()
        logits = logits.contiguous()
        weights, ids = ext.moe_route_fwd(logits, top_k, out_dtype)
        ctx.save_for_backward(logits, ids)
        ctx.mark_non_differentiable(ids)
        return weights, ids

    @staticmethod
    def backward(ctx, dweights, _dids):
        ext = require_ext()
        logits, ids = ctx.saved_tensors
        dlogits = ext.moe_route_bwd(logits, ids, dweights.float().contiguous())
        return dlogits, None, None


def _route_torch(logits, top_k, out_dtype):
    lf = logits.float()
    probs = torch.softmax(lf, dim=-1)
    # stable descending sort: equal values keep ascending index order
    ids = torch.sort(lf, dim=-1, descending=True, stable=True)[1][:, :top_k]
    topv = probs.gather(-1, ids)
    topv = topv / topv.sum(dim=-1, keepdim=True)
    return topv.to(out_dtype), ids.to(torch.int32)


def moe_route(
    logits: torch.Tensor, top_k: int, out_dtype: Optional[torch.dtype] = None
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k routing of ``logits`` [N, E]: returns (weights [N, k] in
    ``out_dtype`` (default: the logits' dtype), expert ids [N, k] int32).

    Softmax in fp32 over all E experts, then renormalised over the chosen k
    (Mixtral semantics).  ids are ordered by descending probability; ties go
    to the lower expert index.  Differentiable in ``logits``.
    """
    out_dtype = out_dtype or logits.dtype
    n, n_expert = logits.shape
    if (
        logits.is_cuda
        and logits.dtype in _ROW_DTYPES
        and out_dtype in _ROW_DTYPES
        and _topk_ok(n, n_expert, top_k)
    ):
        return _RouteFn.apply(logits, top_k, out_dtype)
    return _route_torch(logits, top_k, out_dtype)


# ---------------------------------------------------------------------------
# sort
# ---------------------------------------------------------------------------
def moe_sort(
    ids: torch.Tensor, n_expert: int
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Stable counting sort of the pairs ``p = token * k + slot`` by expert.

    Returns int32 ``(order [N*k], pos [N, k], counts [n_expert])``:
    ``order`` lists the pairs grouped by ascending expert and, within an
    expert, by ascending ``p``; ``pos`` is the inverse of ``order``
    (``order[pos[t, j]] == t * k + j``); ``counts`` is the histogram.  ids
    must lie in ``[0, n_expert)``.
    """
    n, top_k = ids.shape
    if ids.is_cuda and _topk_ok(n, n_expert, top_k):
        ext = require_ext()
        order, pos, counts = ext.moe_sort(
            ids.to(torch.int32).contiguous(), n_expert
        )
        return order, pos, counts
    flat = ids.reshape(-1).long()
    order = torch.argsort(flat, stable=True)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel(), device=ids.device)
    counts = torch.bincount(flat, minlength=n_expert)
    return (
        order.to(torch.int32),
        pos.view(n, top_k).to(torch.int32),
        counts.to(torch.int32),
    )


# ---------------------------------------------------------------------------
# permute / combine
# ---------------------------------------------------------------------------
class _PermuteFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, order, pos):
        ext = require_ext()
        ctx.save_for_backward(pos)
        return ext.moe_permute_fwd(x.contiguous(), order, pos.shape[1])

    @staticmethod
    def backward(ctx, dxs):
        ext = require_ext()
        (pos,) = ctx.saved_tensors
        return ext.moe_permute_bwd(dxs.contiguous(), pos), None, None


def moe_permute(
    x: torch.Tensor, order: torch.Tensor, pos: torch.Tensor
) -> torch.Tensor:
    """``xs[i] = x[order[i] // k]`` with ``(order, pos)`` from
    :func:`moe_sort` (``k = pos.shape[1]``): token rows in expert order.
    The backward sums each token's k rows through ``pos`` in fp32."""
    n, top_k = pos.shape
    if _rows_ok(x, n, top_k) and order.dtype == pos.dtype == torch.int32:
        return _PermuteFn.apply(x, order.contiguous(), pos.contiguous())
    return x.index_select(0, order.long() // top_k)


class _CombineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, weights, pos):
        ext = require_ext()
        y = y.contiguous()
        weights = weights.contiguous()
        ctx.save_for_backward(y, weights, pos)
        return ext.moe_combine_fwd(y, weights, pos)

    @staticmethod
    def backward(ctx, dout):
        ext = require_ext()
        y, weights, pos = ctx.saved_tensors
        dy, dweights = ext.moe_combine_bwd(dout.contiguous(), y, weights, pos)
        return dy, dweights.to(weights.dtype), None


def moe_combine(
    y: torch.Tensor, weights: torch.Tensor, pos: torch.Tensor
) -> torch.Tensor:
    """``out[t] = sum_j weights[t, j] * y[pos[t, j]]``, slot-ascending,
    accumulated in fp32 and rounded once.  Differentiable in ``y`` and
    ``weights``."""
    n, top_k = pos.shape
    if (
        _rows_ok(y, n, top_k)
        and weights.dtype == y.dtype
        and pos.dtype == torch.int32
    ):
        return _CombineFn.apply(y, weights, pos.contiguous())
    rows = y.index_select(0, pos.reshape(-1).long()).view(n, top_k, -1)
    out = (rows.float() * weights.float().unsqueeze(-1)).sum(dim=1)
    return out.to(y.dtype)
