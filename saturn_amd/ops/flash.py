"""Flash attention dispatch (K2).

``saturn_amd._C.attn_fwd/attn_bwd`` are the hand-written CDNA4 MFMA kernels
(attention.hip); they take bf16 with a head size of 64, 128 or 256.  Any
other (dtype, head size) goes to the explicit-GEMM math composition (rocBLAS
GEMMs + softmax — no Triton, no aotriton) and WARNS once with the reason:
measurements taken on that path are not this framework's attention numbers.

Causal attention takes an optional per-row lower key bound ``kv_lo``: row
``t`` of batch ``b`` attends key ``j`` iff ``kv_lo[b, t] <= j <= t``.  A
sliding window (``window_lo``) and packed documents (``document_lo``) are
both such bounds; the kernels skip the key tiles no row of a block sees.

Attention dropout (``dropout_p``, the models' ``attn_pdrop``) is fused into
the kernels: whether probability (b, h, i, j) is kept is a pure function of
(seed, b*H + h, i, j) — ``dropout_keep`` below is the torch twin of
csrc/attn_rng.h — so forward, backward, the CPU path and the tests'
reference regenerate one mask from the seed and no [B,H,T,T] tensor exists on
the fused path.
"""

from __future__ import annotations

import logging
import math
import struct

import torch

from saturn_amd.ops import require_ext

log = logging.getLogger(__name__)
_warned = False


_window_lo_cache: dict = {}


def window_lo(T: int, window: int, device) -> torch.Tensor:
    """int32 [T]: ``max(0, t - window + 1)`` — row t sees ``window`` keys
    including itself (the Hugging Face Mistral convention).  Cached per
    (T, window, device); treat the result as read-only."""
    if window < 1:
        raise ValueError(f"window must be >= 1, got {window}")
    key = (int(T), int(window), torch.device(device))
    lo = _window_lo_cache.get(key)
    if lo is None:
        t = torch.arange(T, dtype=torch.int32, device=device)
        lo = (t - (int(window) - 1)).clamp_(min=0)
        _window_lo_cache[key] = lo
    return lo


def document_lo(input_ids: torch.Tensor, sep_id: int) -> torch.Tensor:
    """int32 [B, T]: the first position of the document each token belongs
    to, for rows that pack several documents.  A document starts at position
    0 and after every ``sep_id`` token; the separator belongs to the document
    it ends.  Built on ``input_ids``' device from a cummax with no host
    read, so a training step still captures into a hipGraph."""
    if input_ids.dim() != 2:
        raise ValueError("document_lo: input_ids must be [B, T]")
    B, T = input_ids.shape
    pos = torch.arange(T, device=input_ids.device).expand(B, T)
    starts = torch.zeros_like(pos)
    starts[:, 1:] = torch.where(input_ids[:, :-1] == sep_id, pos[:, 1:], 0)
    return starts.cummax(dim=-1).values.to(torch.int32)


def resolve_lo(T: int, device, causal: bool, window=None, kv_lo=None):
    """The bound a (window, kv_lo) pair asks for at length T, or None when
    it is the plain causal triangle.  An explicit ``kv_lo`` is brought into
    the kernels' contract (0 <= lo[t] <= t, non-decreasing) on the device."""
    if window is None and kv_lo is None:
        return None
    if not causal:
        raise ValueError("window / kv_lo need causal=True")
    if window is not None:
        if int(window) != window or window < 1:
            raise ValueError(f"window must be an int >= 1, got {window!r}")
        window = None if window >= T else int(window)
    if kv_lo is None:
        return None if window is None else window_lo(T, window, device)
    if kv_lo.dtype != torch.int32:
        raise ValueError(f"kv_lo must be int32, got {kv_lo.dtype}")
    if kv_lo.dim() not in (1, 2) or kv_lo.shape[-1] != T:
        raise ValueError(
            f"kv_lo must be [T] or [B, T] with T={T}, got {tuple(kv_lo.shape)}")
    if kv_lo.device != torch.device(device):
        raise ValueError(f"kv_lo is on {kv_lo.device}, q on {device}")
    t = torch.arange(T, dtype=torch.int32, device=device)
    lo = torch.minimum(kv_lo.clamp(min=0), t).cummax(dim=-1).values
    if window is not None:
        lo = torch.maximum(lo, window_lo(T, window, device))
    return lo.to(torch.int32).contiguous()


def lo_mask(kv_lo: torch.Tensor) -> torch.Tensor:
    """bool [T, T] or [B, 1, T, T]: may row t see key j (lo[t] <= j <= t)?"""
    T = kv_lo.shape[-1]
    j = torch.arange(T, device=kv_lo.device)
    ok = (j >= kv_lo.long().unsqueeze(-1)) & (j <= j[:, None])
    return ok.unsqueeze(1) if ok.dim() == 3 else ok


# ---------------------------------------------------------------------------
# attention dropout: the keep function (twin of csrc/attn_rng.h)
# ---------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def _i64(x: int) -> int:
    """The int64 with the bit pattern of x mod 2^64."""
    x &= _M64
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(z: torch.Tensor, n: int) -> torch.Tensor:
    """Logical right shift of int64 (>> is arithmetic: mask the sign bits)."""
    return (z >> n) & ((1 << (64 - n)) - 1)


def _mix64(z: torch.Tensor) -> torch.Tensor:
    """splitmix64 finalizer on int64 tensors; + and * wrap mod 2^64 as the
    kernel's unsigned arithmetic does."""
    z = z + _i64(0x9E3779B97F4A7C15)
    z = (z ^ _lsr(z, 30)) * _i64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _i64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def dropout_threshold(p: float):
    """(thr, r): the 16-bit keep threshold floor(p * 65536 + 0.5) (capped at
    65535) and the factor 1 / (1 - thr / 65536), rounded to fp32 as the
    kernels receive it.  The effective rate is thr / 65536; thr == 0 is no
    dropout."""
    if not 0.0 <= p < 1.0:          # also refuses NaN
        raise ValueError(f"dropout_p must be in [0, 1), got {p!r}")
    thr = min(65535, int(math.floor(p * 65536.0 + 0.5)))
    r = 65536.0 / (65536.0 - thr)
    return thr, struct.unpack("f", struct.pack("f", r))[0]


def dropout_keep(seed: int, B: int, H: int, T: int, p: float,
                 device="cpu") -> torch.Tensor:
    """bool [B, H, T, T]: is probability (b, h, i, j) kept?  H is the number
    of q heads.  One 64-bit draw per (row, aligned group of four keys), one
    16-bit field per key; T does not enter the counter, so a ragged T's mask
    is the top-left corner of its padded form's."""
    thr, _ = dropout_threshold(p)
    if T > (1 << 20) or B * H >= (1 << 24):
        raise ValueError("attention dropout needs T <= 2^20 and B*H < 2^24")
    if thr == 0:
        return torch.ones(B, H, T, T, dtype=torch.bool, device=device)
    bh = torch.arange(B * H, dtype=torch.int64, device=device).view(B, H, 1, 1)
    i = torch.arange(T, dtype=torch.int64, device=device).view(1, 1, T, 1)
    j4 = torch.arange((T + 3) // 4, dtype=torch.int64,
                      device=device).view(1, 1, 1, -1)
    r64 = _mix64(_i64(int(seed)) ^ ((bh << 40) | (i << 20) | j4))
    shifts = 16 * torch.arange(4, dtype=torch.int64, device=device)
    # >> is arithmetic, but bits [16f, 16f + 16) are below the sign extension
    keep = ((r64.unsqueeze(-1) >> shifts) & 0xFFFF) >= thr
    return keep.reshape(B, H, T, -1)[..., :T]


def draw_seed() -> int:
    """A 62-bit seed drawn on the host as fused_dropout draws its own (CPU
    randint: follows torch.manual_seed, no device sync).  Under
    torch.distributed the rank enters bits 48.., so tensor- and
    sequence-parallel ranks that hold different heads do not share masks."""
    seed = int(torch.randint(0, 2**62, (1,)).item())
    dist = torch.distributed
    if dist.is_available() and dist.is_initialized():
        seed ^= dist.get_rank() << 48
    return seed


def _pad_t64(t: torch.Tensor) -> torch.Tensor:
    """Zero-pad the T dim (dim -2) up to a multiple of 64."""
    pad = (-t.shape[-2]) % 64
    if pad == 0:
        return t
    return torch.nn.functional.pad(t, (0, 0, 0, pad))


class _FlashFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, kv_lo=None, dropout_p=0.0, seed=0):
        ext = require_ext()
        T = q.shape[-2]
        if T % 64 and kv_lo is not None:
            # padded rows get the last real key as their bound: still
            # non-decreasing and <= t, and no padded row is empty (an empty
            # row would put NaN into LSE and, through exp(s - lse) * 0,
            # into dK/dV)
            kv_lo = torch.nn.functional.pad(kv_lo, (0, (-T) % 64), value=T - 1)
        if T % 64:
            # ragged T (ViT's 197, BERT's raw lengths): zero-pad to the
            # kernels' 64-row tiles; padded KEYS are masked in-kernel via
            # kv_len and padded q rows are sliced off below (their zero
            # dO rows contribute exactly 0 to dK/dV in backward)
            q, k, v = _pad_t64(q), _pad_t64(k), _pad_t64(v)
        if dropout_p > 0.0:
            o, lse = ext.attn_fwd(q, k, v, causal, T, dropout_p=dropout_p,
                                  seed=seed)
        else:
            o, lse = ext.attn_fwd(q, k, v, causal, T, kv_lo=kv_lo)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.drop = (dropout_p, seed)  # the backward regenerates the mask
        ctx.kv_lo = kv_lo  # int32, no gradient
        ctx.causal = causal
        ctx.t_real = T
        return o[:, :, :T] if T % 64 else o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        ext = require_ext()
        T = ctx.t_real
        do = _pad_t64(_dense_rows(do)) if T % 64 else _dense_rows(do)
        p, seed = ctx.drop
        if p > 0.0:
            dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, ctx.causal, T,
                                      dropout_p=p, seed=seed)
        else:
            dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, ctx.causal, T,
                                      kv_lo=ctx.kv_lo)
        if T % 64:
            dq, dk, dv = dq[:, :, :T], dk[:, :, :T], dv[:, :, :T]
        return dq, dk, dv, None, None, None, None


def _kernel_supported(q) -> bool:
    # ragged T is padded to 64 rows by the wrapper; D stays restricted to
    # the MFMA tile shapes
    return q.dtype == torch.bfloat16 and q.shape[-1] in (64, 128, 256)


def _dense_rows(t):
    """The kernels address arbitrary (B, H, T) strides but need a dense,
    16-B-aligned innermost dim — transposed views of the model's [B,T,H,D]
    projections qualify, so no copies in the common path.  Every row must
    start on a 16-B boundary: a view that starts off one (a column slice at
    an offset that is no multiple of 8 elements), or whose batch or head
    stride is no multiple of 8, is copied too.  The copy is a clone into
    fresh (aligned) storage: .contiguous() would hand back an already
    contiguous tensor that merely starts at a misaligned offset."""
    if (t.stride(-1) == 1 and t.storage_offset() % 8 == 0
            and all(s % 8 == 0 for s in t.stride()[:-1])):
        return t
    return t.clone(memory_format=torch.contiguous_format)


def check_dropout(dropout_p, window=None, kv_lo=None) -> float:
    """dropout_p as a float in [0, 1); refuses it together with a window or
    a kv_lo bound (not built: it would double the kv_lo instantiations)."""
    p = float(dropout_p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"dropout_p must be in [0, 1), got {dropout_p!r}")
    if p > 0.0 and (window is not None or kv_lo is not None):
        raise ValueError("dropout_p > 0 is not supported together with "
                         "window / kv_lo")
    return p


def flash_attention(q, k, v, causal: bool = True, window=None,
                    kv_lo=None, dropout_p: float = 0.0,
                    seed=None) -> torch.Tensor:
    """q,k,v: [B, H, T, D] bf16/fp16 contiguous (GQA: H_kv may divide H).

    ``window`` (int >= 1): row t sees keys max(0, t-window+1) .. t.
    ``kv_lo`` (int32 [T] or [B, T] on q's device): row t sees keys
    kv_lo[b,t] .. t; shared by all heads.  Given both, the bound is the
    elementwise maximum.  Both need ``causal=True`` (ValueError otherwise);
    ``window >= T`` without ``kv_lo`` is the plain causal path.

    ``dropout_p`` in [0, 1): attention dropout on the softmax output, kept
    entries scaled by 1/(1-p) (p is quantised to a multiple of 2^-16).  The
    mask is ``dropout_keep(seed, ...)``; ``seed=None`` draws one on the host
    (``draw_seed``).  Not supported together with ``window`` / ``kv_lo``
    (ValueError).  With ``dropout_p == 0`` the seed is ignored and the call
    is the plain one, bit for bit."""
    p = check_dropout(dropout_p, window, kv_lo)
    lo = resolve_lo(q.shape[-2], q.device, causal, window, kv_lo)
    require_ext()
    if p > 0.0 and seed is None:
        seed = draw_seed()
    if _kernel_supported(q) and p > 0.0:
        return _FlashFn.apply(
            _dense_rows(q), _dense_rows(k), _dense_rows(v), causal, None,
            p, _i64(int(seed))
        )
    if _kernel_supported(q):
        # GQA is native in the kernels: kv may keep fewer heads
        if lo is None:
            return _FlashFn.apply(
                _dense_rows(q), _dense_rows(k), _dense_rows(v), causal
            )
        return _FlashFn.apply(
            _dense_rows(q), _dense_rows(k), _dense_rows(v), causal, lo
        )
    global _warned
    if not _warned:
        log.warning(
            "attention kernels take bf16 with head size 64, 128 or 256; got "
            "%s with head size %d — using explicit-GEMM math attention "
            "(slower)", q.dtype, q.shape[-1]
        )
        _warned = True
    from saturn_amd.ops.functional import attention_math

    if k.shape[1] != q.shape[1]:
        rep = q.shape[1] // k.shape[1]
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    return attention_math(q, k, v, causal=causal, kv_lo=lo, dropout_p=p,
                          seed=seed)
