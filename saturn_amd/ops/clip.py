"""Global gradient-norm clipping.

One coefficient for the whole model, ``min(1, max_norm / (norm + 1e-6))``
(the formula of ``torch.nn.utils.clip_grad_norm_``), computed without a
host read so the step stays capturable as a hipGraph:

1. ``grad_sqsum`` (``csrc/grad_norm.hip``) reduces every gradient of a
   (device, dtype) group to one fp32 squared sum — read-only, no atomics,
   bitwise reproducible;
2. the sums are added on one device and, under a sharding technique, pass
   through ``norm_reduce`` (an all-reduce of one element) — gradients named
   ``replicated`` are identical on every rank and are added once, after it;
3. ``clip_coef`` leaves ``{norm, coef, skipped_total}`` in a persistent
   device tensor.  A non-finite squared sum gives a non-finite ``norm`` —
   that is the skip flag — and ``coef = 0``.

``FusedSGD`` / ``FusedAdam`` hand that tensor to their kernels, which scale
``g`` as they load it (no second pass over the gradients) and return at once
when the flag is set.  ``clip_grads_`` is the route for optimizers that are
not ours: same coefficient, applied with ``torch._foreach_mul_``.

On CPU the same contract runs on torch ops with fp32 accumulation.
"""

from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import torch

from saturn_amd.ops import require_ext

NormReduce = Callable[[torch.Tensor], torch.Tensor]


def check_max_grad_norm(max_grad_norm: Optional[float]) -> Optional[float]:
    """``None`` or a finite positive float; anything else raises."""
    if max_grad_norm is None:
        return None
    v = float(max_grad_norm)
    if not math.isfinite(v) or v <= 0.0:
        raise ValueError(
            f"max_grad_norm must be a finite positive number, got {max_grad_norm!r}"
        )
    return v


class GradClipper:
    """Persistent state of one model's clipping: the ``grad_sqsum`` partials
    per (device, dtype), the ``{norm, coef, skipped_total}`` tensor on the
    home device and its copies on the other devices of a pipeline.  Nothing
    here is reallocated from step to step unless the gradient list grows."""

    def __init__(
        self,
        max_norm: float,
        norm_reduce: Optional[NormReduce] = None,
        replicated: Iterable[torch.Tensor] = (),
    ) -> None:
        self.max_norm = check_max_grad_norm(max_norm)
        if self.max_norm is None:
            raise ValueError("GradClipper needs a max_norm")
        self.norm_reduce = norm_reduce
        self._replicated = {id(p) for p in replicated}
        self._partials: Dict[Tuple[torch.device, torch.dtype], torch.Tensor] = {}
        self._out: Optional[torch.Tensor] = None
        self._copies: Dict[torch.device, torch.Tensor] = {}

    def set_replicated(self, params: Iterable[torch.Tensor]) -> None:
        self._replicated = {id(p) for p in params}

    # -- squared sums -----------------------------------------------------
    def _sqsum(self, grads: Sequence[torch.Tensor],
               home: torch.device) -> torch.Tensor:
        """fp32[1] on ``home``: squared sum of ``grads``, one reduction per
        (device, dtype) group, added on ``home`` in list order."""
        groups: Dict[Tuple[torch.device, torch.dtype], List[torch.Tensor]] = {}
        for g in grads:
            groups.setdefault((g.device, g.dtype), []).append(g)
        total = None
        for (device, dtype), gs in groups.items():
            if device.type == "cuda":
                ext = require_ext()
                # one buffer per group: calls on a stream run in order
                key = (device, dtype)
                need = ext.grad_sqsum_slots(len(gs))
                buf = self._partials.get(key)
                if buf is None or buf.numel() < need:
                    buf = torch.empty(need, dtype=torch.float32, device=device)
                    self._partials[key] = buf
                with torch.cuda.device(device):
                    sq = ext.grad_sqsum(list(gs), buf)
            else:
                sq = torch.stack(
                    [g.detach().float().pow(2).sum() for g in gs]
                ).sum().reshape(1)
            if sq.device != home:
                # stream-ordered device-to-device copy, no host read
                sq = sq.to(home, non_blocking=True)
            total = sq if total is None else total + sq
        if total is None:
            total = torch.zeros(1, dtype=torch.float32, device=home)
        return total

    # -- coefficient ------------------------------------------------------
    @torch.no_grad()
    def compute(self, params: Sequence[torch.Tensor]) -> torch.Tensor:
        """Reduce the gradients of ``params`` and refresh
        ``{norm, coef, skipped_total}``; returns that tensor (home device).
        This is the one place the coefficient is computed, for the fused
        optimizers and for ``clip_grads_`` alike."""
        with_grad = [p for p in params if p.grad is not None]
        if self._out is not None:
            home = self._out.device
        elif with_grad:
            home = with_grad[-1].grad.device  # a pipeline's last stage
        else:
            home = torch.device("cpu")
        if self._out is None:
            self._out = torch.zeros(3, dtype=torch.float32, device=home)
        if self.norm_reduce is None:
            sq = self._sqsum([p.grad for p in with_grad], home)
        else:
            shards = [p.grad for p in with_grad if id(p) not in self._replicated]
            repl = [p.grad for p in with_grad if id(p) in self._replicated]
            sq = self.norm_reduce(self._sqsum(shards, home))
            if repl:
                sq = sq + self._sqsum(repl, home)
        out = self._out
        if home.type == "cuda":
            with torch.cuda.device(home):
                require_ext().clip_coef(sq.reshape(1), self.max_norm, out)
        else:
            sq = sq.reshape(1).float()
            finite = torch.isfinite(sq)
            norm = sq.sqrt()
            coef = torch.where(
                finite,
                (self.max_norm / (norm + 1e-6)).clamp(max=1.0),
                torch.zeros_like(norm),
            )
            out[0:1] = norm
            out[1:2] = coef
            out[2:3] += (~finite).float()
        return out

    def out_on(self, device: torch.device) -> torch.Tensor:
        """``{norm, coef, skipped_total}`` on ``device`` (a stream-ordered
        copy when that is not the home device)."""
        out = self._out
        if out.device == device:
            return out
        c = self._copies.get(device)
        if c is None:
            c = torch.empty_like(out, device=device)
            self._copies[device] = c
        c.copy_(out, non_blocking=True)
        return c

    # -- results, never synchronising --------------------------------------
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        return None if self._out is None else self._out[0]

    @property
    def skipped_steps(self) -> Optional[torch.Tensor]:
        return None if self._out is None else self._out[2]

    # -- torch route --------------------------------------------------------
    @torch.no_grad()
    def clip_(self, params: Sequence[torch.Tensor]) -> torch.Tensor:
        """Scale the gradients of ``params`` in place by the coefficient;
        zero them when the norm is not finite.  Returns the norm."""
        params = list(params)
        out = self.compute(params)
        by_dev: Dict[torch.device, List[torch.Tensor]] = {}
        for p in params:
            if p.grad is not None:
                by_dev.setdefault(p.grad.device, []).append(p.grad)
        for device, gs in by_dev.items():
            o = self.out_on(device)
            bad = ~torch.isfinite(o[0])
            for g in gs:
                # inf * 0 would leave NaN behind: zero the bad step's grads
                g.masked_fill_(bad, 0)
            torch._foreach_mul_(gs, o[1])
        return out[0]


@torch.no_grad()
def clip_grads_(
    params: Iterable[torch.Tensor],
    max_norm: float,
    norm_reduce: Optional[NormReduce] = None,
    replicated: Iterable[torch.Tensor] = (),
) -> torch.Tensor:
    """Clip the gradients of ``params`` to a global norm of ``max_norm``, in
    place, for an optimizer that is not ``FusedSGD`` / ``FusedAdam``.

    ``norm_reduce`` and ``replicated`` are as in ``FusedSGD``.  A non-finite
    norm zeroes every gradient.  Returns the norm as a 0-d tensor on the
    gradients' device; nothing is read on the host."""
    return GradClipper(max_norm, norm_reduce, replicated).clip_(list(params))
