"""Reference, error floor and acceptance criterion for the attention kernels
(attention.hip) in every mask mode: plain causal / full attention, a per-row
lower key bound (``lo``: sliding windows and packed documents) and attention
dropout (``keep``, ``r``).  Shared by the six test_attention_* files and by
tests/attn_run.py, which holds everything that touches the device.

* ``allowed``   bool mask "may row i see key j" from (T, causal, kv_len, lo).
* ``ref64``     the truth: bf16 inputs upcast to fp64, explicit masked softmax;
                with dropout out = (r Z o P) V, LSE that of the undropped
                scores.
* ``base_bf16`` the same operation with exactly the roundings the kernels make
                by design (fp32 S and softmax, bf16 P before PV, bf16 O; FA2
                backward with P recomputed from LSE, delta from the rounded O,
                bf16 P and dS before their GEMMs, bf16 results; with dropout
                the softmax statistics come from the undropped scores, Z is
                applied to the bf16-rounded P and r sits in the epilogues).
                Its error against ``ref64`` is the floor of a correct bf16
                kernel.  ``mut`` plants one bug for the mutation checks.
* ``close``     max|x - ref| <= 2 max|base - ref| + ulp_bf16(max|ref|).
                The kernel's error is a second draw from the distribution of
                the floor's (same roundings; fast exp/log and fp32 summation
                order are ~1e-6 relative, nothing next to 2^-9), 2x covers the
                spread of a maximum and the ulp a final rounding that tips the
                other way.  The tolerance never looks at the kernel's output.

``lo=None``, ``keep=None`` skip the operations they would add; the neutral
values (a zero bound, an all-true mask with r = 1) run them and give the
same bits (test_attention_window_cpu.py, test_attention_dropout_cpu.py).

This is a plain module: no tests, no fixtures, nothing of the GPU.
"""

from __future__ import annotations

import functools
import math
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from saturn_amd.ops.flash import dropout_keep, dropout_threshold  # noqa: E402

NAMES = ("out", "lse", "dq", "dk", "dv")
# the whole-tensor bounds of tests/test_ops_gpu.py, kept beside `close`
NORM_TOL_FWD = 4e-2
NORM_TOL_BWD = 5e-2
FACTOR = 2.0

DS = (64, 128, 256)
KINDS = ("randn", "peaky")
# plain attention, (B, H, Hkv, T, D): shapes of groups A, B and C of
# test_attention_gpu.py
SHAPES = [
    (1, 3, 3, 192, 64),
    (3, 5, 5, 320, 128),
    (1, 3, 3, 512, 256),
    (1, 3, 3, 130, 64),
    (1, 3, 3, 257, 128),
    (1, 6, 2, 197, 128),
    (1, 4, 1, 192, 64),
]
# kv_lo: (B, H) of the matrix; every GPU shape has B*H <= 16 and T <= 384
BH_WINDOW = (2, 3)
# name -> (T, ("window", W) | ("docs", per-batch document lengths))
BOUNDS = {
    "W17_T192": (192, ("window", 17)),
    "W65_T256": (256, ("window", 65)),
    "W100_T320": (320, ("window", 100)),
    "W200_T384": (384, ("window", 200)),
    "docs_T256": (256, ("docs", ([70, 1, 129, 56], [256]))),
    "docs_T192": (192, ("docs", ([33, 95, 64], [1, 190, 1]))),
}
MATRIX_WINDOW = [(D, bn, kind) for D in DS for bn in BOUNDS for kind in KINDS]
# dropout: (B, H) of the numerics matrix, the mask seed, the inputs' seed
BH_DROP = (1, 2)
SEED = 0x5EED_0D20_0F_A77
DROP_INPUT_SEED = 11
# D x T x causal x kind x p.  T=192 reaches the v1 forward, T=256 the v2
# forward at D <= 128; both are several kv tiles and q blocks.
MATRIX_DROP = [(D, T, causal, kind, p)
               for D in DS for T in (192, 256) for causal in (True, False)
               for kind in KINDS for p in (0.1, 0.5)]
MUTANTS = {
    # dropout mutant: tensors `close` must reject it on
    "transpose": ("out", "dq", "dk", "dv"),
    "head": ("out", "dq", "dk", "dv"),
    "shift": ("out", "dq", "dk", "dv"),
    "bwd_seed": ("dq", "dk", "dv"),
    "no_r_dp": ("dq", "dk"),
    "no_r_fwd": ("out",),
}


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def make_inputs(kind, B, H, Hkv, T, D, device="cpu", seed=0):
    """q [B,H,T,D], k/v [B,Hkv,T,D], do [B,H,T,D] in bf16.  Drawn on the CPU
    so that the CPU and GPU tests see the same numbers.

    randn  unit normal.
    peaky  q x 4 and key norms growing 0.25 -> 0.75 with position (score
           spread 1 -> 3): the row maximum keeps moving to later keys, so
           the online-softmax rescale does real work at every kv tile, while
           LSE stays small enough for one zero-score key to be visible in it.
    qzero  q = 0: uniform attention, analytic LSE and running-mean output.
    """
    g = torch.Generator().manual_seed(1_000_003 * seed + 4099 * T + 17 * D + H)
    q = torch.randn(B, H, T, D, generator=g)
    k = torch.randn(B, Hkv, T, D, generator=g)
    v = torch.randn(B, Hkv, T, D, generator=g)
    do = torch.randn(B, H, T, D, generator=g)
    if kind == "peaky":
        q = q * 4.0
        k = k * (0.25 + 0.5 * torch.arange(T, dtype=torch.float32) / T)[:, None]
    elif kind == "qzero":
        q = torch.zeros_like(q)
    elif kind != "randn":
        raise ValueError(kind)
    return tuple(t.bfloat16().to(device) for t in (q, k, v, do))


# ---------------------------------------------------------------------------
# bounds, by plain Python loops (the library's helpers are tested against
# these)
# ---------------------------------------------------------------------------
def window_bound(T, W):
    return torch.tensor([max(0, t - W + 1) for t in range(T)],
                        dtype=torch.int32)


def docs_bound(lengths, T):
    """[B, T] from per-batch lists of document lengths (each sums to T)."""
    rows = []
    for lens in lengths:
        assert sum(lens) == T, (lens, T)
        row, start = [], 0
        for n in lens:
            row += [start] * n
            start += n
        rows.append(row)
    return torch.tensor(rows, dtype=torch.int32)


def make_bound(name):
    T, (what, arg) = BOUNDS[name]
    return window_bound(T, arg) if what == "window" else docs_bound(arg, T)


def keep_r(seed, B, H, T, p, device="cpu"):
    """(Z bool [B,H,T,T], r): the twin mask and the kernels' fp32 factor."""
    return dropout_keep(seed, B, H, T, p, device), dropout_threshold(p)[1]


# ---------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------
def allowed(T, causal, kv_len=None, lo=None, device="cpu"):
    """bool [T, T], or [B, 1, T, T] for a [B, T] bound: may q row i see key
    j?  j < kv_len; under a causal mask j <= i, and with a bound (lo [T] or
    [B, T], causal only) lo[b, i] <= j."""
    j = torch.arange(T, device=device)
    ok = (j < (T if kv_len is None else kv_len))[None, :].expand(T, T)
    if causal:
        ok = ok & (j[None, :] <= j[:, None])
    if lo is None:
        return ok
    if not causal:
        raise ValueError("a lower key bound needs causal=True")
    band = j >= lo.to(device).long().unsqueeze(-1)
    if band.dim() == 3:
        band = band.unsqueeze(1)
    return ok & band


def ref64(q, k, v, causal, do=None, *, lo=None, keep=None, r=1.0):
    """fp64 attention of the bf16-rounded inputs.  GQA by repeat_interleave;
    dk/dv come back summed to the Hkv heads (autograd does the sum).  With a
    dropout mask `keep` (bool [B,H,T,T]) the probabilities are multiplied by
    keep * r; LSE is always that of the undropped masked scores."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    need = do is not None
    q64 = q.double().requires_grad_(need)
    k64 = k.double().requires_grad_(need)
    v64 = v.double().requires_grad_(need)
    kr = k64.repeat_interleave(rep, dim=1)
    vr = v64.repeat_interleave(rep, dim=1)
    s = torch.matmul(q64, kr.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~allowed(T, causal, lo=lo, device=q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    if keep is not None:
        p = p * keep.double() * float(r)
    out = torch.matmul(p, vr)
    if not need:
        return out.detach(), lse.detach()
    dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), do.double())
    return out.detach(), lse.detach(), dq, dk, dv


# ---------------------------------------------------------------------------
# the error floor (and, with `mut`, deliberately broken variants of it)
# ---------------------------------------------------------------------------
def _r16(t):
    return t.bfloat16().float()


def fwd_block_rows(T, D):
    """q rows per forward block under the default dispatch."""
    return 128 if (T % 128 == 0 and D <= 128) else 64


def _early_stop_seen(lo, T, dev):
    """[B|1, 1, T, T]: the (row, key) pairs the dK/dV kernel still visits
    when the q loop of each 64-key block stops one 32-row tile early."""
    lo2 = (lo if lo.dim() == 2 else lo.unsqueeze(0)).long()      # [B|1, T]
    tiles = torch.arange(0, T, 32, device=dev)                   # q tile rows
    kv0 = torch.arange(0, T, 64, device=dev)                     # key blocks
    # stop[b, kb]: first q tile >= kv0 whose first row starts past the
    # block's last key, T if none does
    past = (lo2[:, tiles][:, None, :] > (kv0 + 63)[None, :, None]) & (
        tiles[None, None, :] >= kv0[None, :, None])
    stop = torch.where(past, tiles[None, None, :], T).min(dim=-1).values
    stop = stop - 32                                             # the bug
    q_tile = (torch.arange(T, device=dev) // 32) * 32
    key_blk = torch.arange(T, device=dev) // 64
    seen = q_tile[None, :, None] < stop[:, key_blk][:, None, :]
    return seen.unsqueeze(1)


def base_bf16(q, k, v, causal, do=None, *, kv_len=None, lo=None, keep=None,
              r=1.0, mut=None):
    """Attention with the kernels' roundings, composed from fp32 torch ops.

    kv_len < T masks the trailing keys (the kernels' ragged-T contract).
    mut plants one bug for the mutation checks:
      ("causal_row", i)     row i masks key >= i instead of key > i
      ("kv_len", d)         keys are masked from kv_len + d
      ("gqa_mod",)          q head h reads kv head h % Hkv instead of h // rep
      ("dk_zero", b, h, t0) dk[b, h, t0:t0+16] = 0
      ("o_swap", c0)        O columns [c0, c0+16) and [c0+16, c0+32) swapped
    with a bound:
      ("lo_plus",)     lo + 1 on every row, clamped to t
      ("lo_minus",)    lo - 1 on every row, clamped to 0
      ("round_up",)    the forward's first key tile rounded UP from the bound
                       of each block's first row: the keys between are lost
                       to every row of the block (out, lse)
      ("early_stop",)  the dK/dV q loop of each 64-key block stops one
                       32-row tile early (dk, dv)
    with dropout:
      ("transpose",)      the mask is read as Z[j, i]
      ("head",)           head h reads head h+1's mask
      ("shift",)          the mask is shifted by one key
      ("bwd_seed", Z2)    the backward uses another seed's mask Z2
      ("no_r_dp",)        r missing from dP in dS
      ("no_r_fwd",)       r missing from the forward epilogue
    """
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    kind = mut[0] if mut else None
    dev = q.device
    kv_len = T if kv_len is None else kv_len
    if kind == "kv_len":
        kv_len = kv_len + mut[1]
    if kind == "gqa_mod":
        hmap = torch.arange(H, device=dev) % Hkv
    else:
        hmap = torch.arange(H, device=dev) // rep
    if lo is not None:
        lo = lo.to(dev)
        t_idx = torch.arange(T, device=dev, dtype=lo.dtype)
        if kind == "lo_plus":
            lo = torch.minimum(lo + 1, t_idx)
        elif kind == "lo_minus":
            lo = (lo - 1).clamp(min=0)
    zf = zb = None                       # the forward's and the backward's Z
    r = float(r)
    if keep is not None:
        z = keep
        if kind == "transpose":
            z = z.transpose(-1, -2)
        elif kind == "head":
            z = z.roll(-1, dims=1)
        elif kind == "shift":
            z = z.roll(1, dims=-1)
        zf = z.float()
        zb = mut[1].float() if kind == "bwd_seed" else zf
    scale = 1.0 / math.sqrt(D)
    qf, kf, vf = q.float(), k.float()[:, hmap], v.float()[:, hmap]
    # ok: the mask of the backward; ok_fwd: the forward's (round_up only)
    ok = allowed(T, causal, kv_len, lo, dev)
    ok_fwd = ok
    if kind == "causal_row":
        ok = ok_fwd = ok.clone()
        ok[mut[1], mut[1]:] = False
    elif kind == "round_up":
        rows = fwd_block_rows(T, D)
        first = (t_idx.long() // rows) * rows                 # block's row 0
        begin = (lo.long()[..., first] + 31) // 32 * 32       # [T] or [B,T]
        late = torch.arange(T, device=dev) >= begin.unsqueeze(-1)
        ok_fwd = ok & (late.unsqueeze(1) if late.dim() == 3 else late)
    s_raw = torch.matmul(qf, kf.transpose(-1, -2)) * scale      # fp32 S
    s = s_raw.masked_fill(~ok_fwd, float("-inf"))
    s_b = s if ok_fwd is ok else s_raw.masked_fill(~ok, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)                                         # fp32 softmax
    l = p.sum(dim=-1, keepdim=True)                              # undropped
    if zf is None:
        o = (torch.matmul(_r16(p), vf) / l).bfloat16()           # bf16 P, O
    else:
        r_fwd = 1.0 if kind == "no_r_fwd" else r
        o = (torch.matmul(_r16(p) * zf, vf) * r_fwd / l).bfloat16()  # P o Z
    lse = (m + torch.log(l)).squeeze(-1)
    if kind == "o_swap":
        c0 = mut[1]
        o = o.clone()
        o[..., c0:c0 + 32] = torch.cat(
            (o[..., c0 + 16:c0 + 32], o[..., c0:c0 + 16]), dim=-1)
    if do is None:
        return o, lse
    dof = do.float()
    p2 = torch.exp(s_b - lse.unsqueeze(-1))                      # P from LSE
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)          # rounded O
    if zb is not None:
        dp = (1.0 if kind == "no_r_dp" else r) * zb * dp
    ds = _r16(p2 * (dp - delta) * scale)                         # bf16 dS
    p2 = _r16(p2)                                                # bf16 P
    if zb is not None:
        p2 = p2 * zb                                             # P o Z
    dq = torch.matmul(ds, kf)
    ds_k, p2_k = ds, p2
    if kind == "early_stop":
        seen = _early_stop_seen(lo, T, dev)
        ds_k, p2_k = ds * seen, p2 * seen
    dk_h = torch.matmul(ds_k.transpose(-1, -2), qf)
    dv_h = torch.matmul(p2_k.transpose(-1, -2), dof)
    if zb is not None:
        dv_h = dv_h * r
    dk = torch.zeros(B, Hkv, T, D, device=dev).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, device=dev).index_add_(1, hmap, dv_h)
    if kind == "dk_zero":
        dk[mut[1], mut[2], mut[3]:mut[3] + 16] = 0.0
    return o, lse, dq.bfloat16(), dk.bfloat16(), dv.bfloat16()


# ---------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------
def ulp_bf16(m):
    """Spacing of bf16 (8 significant bits) at magnitude m."""
    if not m > 0.0:
        return 0.0
    return 2.0 ** (math.floor(math.log2(m)) - 7)


def max_err(x, ref):
    return (x.double() - ref.double()).abs().max().item()


def close_info(x, ref, base):
    err = max_err(x, ref)
    floor = max_err(base, ref)
    tol = FACTOR * floor + ulp_bf16(ref.double().abs().max().item())
    # the ratio of the docs table: kernel error over the floor's
    ratio = err / floor if floor > 0.0 else (0.0 if err == 0.0 else math.inf)
    return {"err": err, "floor": floor, "tol": tol, "ratio": ratio,
            "ok": bool(err <= tol)}


def close(x, ref, base):
    """max|x - ref| <= 2 max|base - ref| + ulp_bf16(max|ref|)."""
    return close_info(x, ref, base)["ok"]


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp(min=1e-300)).item()


def lse_tolerance(q, k, mask, lse_ref):
    """8 x the error of a plain fp32 torch logsumexp of the fp32 scores under
    `mask` (an `allowed` result) against fp64 at the same inputs, + 1e-6."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, dim=1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~mask, float("-inf"))
    e = (torch.logsumexp(s, dim=-1).double() - lse_ref).abs().max().item()
    return 8.0 * e + 1e-6


def lse_edge_shift(q, k, lse_ref, every_head=True):
    """What one mask error does to LSE at the longest row (the last one, in
    both mask modes), where a single key weighs least: wrongly masking the
    edge key (the diagonal under a causal mask, key kv_len-1 under a length
    mask) shifts it by -log(1 - p_edge); wrongly admitting one zero padding
    key (score 0) by log(1 + exp(-lse)).  The smaller of the two is
    returned, taken over (b, h) as the MINIMUM (every_head: the fault is
    visible on whichever single head it touches) or as the maximum (visible
    only as a fault that hits every head, since the comparison fails as
    soon as one of them moves; for inputs whose edge key can weigh ~1e-6 on
    some head)."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    kr = k.double().repeat_interleave(rep, dim=1)
    s_edge = (q.double()[:, :, -1] * kr[:, :, -1]).sum(-1) / math.sqrt(D)
    lse_last = lse_ref[:, :, -1]
    p_edge = torch.exp(s_edge - lse_last).clamp(max=1.0)
    masked = -torch.log1p(-p_edge)
    admitted = torch.log1p(torch.exp(-lse_last))
    if every_head:
        return min(masked.min().item(), admitted.min().item())
    return min(masked.max().item(), admitted.max().item())


def check_case(got, ref, base, lse_tol, lse_shift=None):
    """Compare a result (out, lse, dq, dk, dv) at the unpadded length with
    `ref` under `close` (floor: `base`), the LSE tolerance and the norm-wise
    bounds, on the CPU.  got[i] may be None (the public route has no LSE).
    With lse_shift (`lse_edge_shift`) the LSE tolerance must lie below it,
    or the LSE check is vacuous.  Returns (report, failures); never raises.
    Each failure starts with "<tensor>: <check>" where <check> is one of
    shape, non-finite, dtype, max err (`close`, or the LSE tolerance),
    tolerance (vacuous LSE check), norm-wise."""
    rep, bad = {}, []
    for i, name in enumerate(NAMES):
        x, r = got[i], ref[i].cpu()
        if x is None:
            continue
        if tuple(x.shape) != tuple(r.shape):
            bad.append(f"{name}: shape {tuple(x.shape)} != {tuple(r.shape)}")
            continue
        x = x.cpu()
        if not torch.isfinite(x.float()).all():
            bad.append(f"{name}: non-finite values")
            continue
        if name == "lse":
            err = max_err(x, r)
            rep[name] = {"err": err, "tol": lse_tol}
            if x.dtype != torch.float32:
                bad.append(f"lse: dtype {x.dtype}")
            if lse_shift is not None:
                rep[name]["shift"] = lse_shift
                if not lse_tol < lse_shift:
                    bad.append(f"lse: tolerance {lse_tol:.3e} not below the "
                               f"one-key shift {lse_shift:.3e} (vacuous check)")
            if not err <= lse_tol:
                bad.append(f"lse: max err {err:.3e} > {lse_tol:.3e}")
            continue
        info = close_info(x, r, base[i].cpu())
        info["rel"] = rel_err(x, r)
        rep[name] = info
        if x.dtype != torch.bfloat16:
            bad.append(f"{name}: dtype {x.dtype}")
        if not info["ok"]:
            bad.append(f"{name}: max err {info['err']:.4e} > tol "
                       f"{info['tol']:.4e} (floor {info['floor']:.4e}, "
                       f"ratio {info['ratio']:.2f})")
        ntol = NORM_TOL_FWD if name == "out" else NORM_TOL_BWD
        if not info["rel"] < ntol:
            bad.append(f"{name}: norm-wise {info['rel']:.3e} >= {ntol}")
    return rep, bad


def check_plain(got, q, k, v, causal, do, ref=None, every_head=True):
    """`check_case` for plain attention from the inputs alone: truth, floor
    and LSE tolerance computed here (on the inputs' device), and the LSE
    tolerance held below the one-key shift (`lse_edge_shift`)."""
    ref = ref64(q, k, v, causal, do) if ref is None else ref
    mask = allowed(q.shape[2], causal, device=q.device)
    return check_case(got, ref, base_bf16(q, k, v, causal, do),
                      lse_tolerance(q, k, mask, ref[1]),
                      lse_edge_shift(q, k, ref[1], every_head))


def ratios(rep):
    return {n: round(rep[n]["ratio"], 3) for n in rep if n != "lse"}


def rejected(bad):
    """The tensors a failure list names."""
    return {b.split(":", 1)[0] for b in bad}


def padded_t(T):
    return T + (-T) % 64


# ---------------------------------------------------------------------------
# cases: inputs, masks, truth and floor computed once per process and shared
# (treat as read-only)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, B, H, Hkv, T, D, causal=True, bound=None, p=0.0, seed=0,
         drop_seed=SEED):
    """One case on the CPU.  bound: None, a BOUNDS name, ("window", W) or
    ("docs", per-batch tuples of lengths); p > 0: dropout with the mask of
    drop_seed.  `seed` draws the inputs; the dict's "seed" is the mask's, the
    kernels' keyword."""
    q, k, v, do = make_inputs(kind, B, H, Hkv, T, D, "cpu", seed)
    lo = keep = None
    r = 1.0
    if isinstance(bound, str):
        assert BOUNDS[bound][0] == T
        lo = make_bound(bound)
    elif bound is not None:
        lo = (window_bound(T, bound[1]) if bound[0] == "window"
              else docs_bound(bound[1], T))
    if p > 0.0:
        keep, r = keep_r(drop_seed, B, H, T, p)
    ref = ref64(q, k, v, causal, do, lo=lo, keep=keep, r=r)
    base = base_bf16(q, k, v, causal, do, lo=lo, keep=keep, r=r)
    return {"q": q, "k": k, "v": v, "do": do, "causal": causal, "lo": lo,
            "keep": keep, "r": r, "p": p, "seed": drop_seed, "ref": ref,
            "base": base,
            "lse_tol": lse_tolerance(q, k, allowed(T, causal, lo=lo), ref[1])}
