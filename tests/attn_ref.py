"""Reference, error floor and acceptance criterion for the attention kernels
(attention.hip), shared by test_attention_ref_cpu.py, test_attention_gpu.py
and the per-switch child processes (``python tests/attn_ref.py --sweep``).

* ``ref64``     the truth: bf16 inputs upcast to fp64, explicit masked softmax.
* ``base_bf16`` the same operation with exactly the roundings the kernels make
                by design (fp32 S and softmax, bf16 P before PV, bf16 O; FA2
                backward with P recomputed from LSE, delta from the rounded O,
                bf16 P and dS before their GEMMs, bf16 results).  Its error
                against ``ref64`` is the floor of a correct bf16 kernel.
* ``close``     max|x - ref| <= 2 max|base - ref| + ulp_bf16(max|ref|).
                The kernel's error is a second draw from the distribution of
                the floor's (same roundings; fast exp/log and fp32 summation
                order are ~1e-6 relative, nothing next to 2^-9), 2x covers the
                spread of a maximum and the ulp a final rounding that tips the
                other way.  The tolerance never looks at the kernel's output.

This is a plain module: no tests, no fixtures.
"""

from __future__ import annotations

import json
import math
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

NAMES = ("out", "lse", "dq", "dk", "dv")
# the whole-tensor bounds of tests/test_ops_gpu.py, kept beside `close`
NORM_TOL_FWD = 4e-2
NORM_TOL_BWD = 5e-2
FACTOR = 2.0


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
# the truth
# ---------------------------------------------------------------------------
def _allowed(T, causal, kv_len, device):
    """[T, T] bool: may q row i see key j?"""
    j = torch.arange(T, device=device)
    ok = (j < kv_len)[None, :].expand(T, T)
    if causal:
        ok = ok & (j[None, :] <= j[:, None])
    return ok


def ref64(q, k, v, causal, do=None):
    """fp64 attention of the bf16-rounded inputs.  GQA by repeat_interleave;
    dk/dv come back summed to the Hkv heads (autograd does the sum)."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    need = do is not None
    q64 = q.double().requires_grad_(need)
    k64 = k.double().requires_grad_(need)
    v64 = v.double().requires_grad_(need)
    kr = k64.repeat_interleave(rep, dim=1)
    vr = v64.repeat_interleave(rep, dim=1)
    s = torch.matmul(q64, kr.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~_allowed(T, causal, T, q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.matmul(torch.exp(s - lse.unsqueeze(-1)), vr)
    if not need:
        return out.detach(), lse.detach()
    dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), do.double())
    return out.detach(), lse.detach(), dq, dk, dv


# ---------------------------------------------------------------------------
# the error floor (and, with `mut`, deliberately broken variants of it)
# ---------------------------------------------------------------------------
def _r16(t):
    return t.bfloat16().float()


def base_bf16(q, k, v, causal, do=None, kv_len=None, mut=None):
    """Attention with the kernels' roundings, composed from fp32 torch ops.

    kv_len < T masks the trailing keys (the kernels' ragged-T contract).
    mut plants one bug for the mutation check:
      ("causal_row", i)     row i masks key >= i instead of key > i
      ("kv_len", d)         keys are masked from kv_len + d
      ("gqa_mod",)          q head h reads kv head h % Hkv instead of h // rep
      ("dk_zero", b, h, t0) dk[b, h, t0:t0+16] = 0
      ("o_swap", c0)        O columns [c0, c0+16) and [c0+16, c0+32) swapped
    """
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    kind = mut[0] if mut else None
    kv_len = T if kv_len is None else kv_len
    if kind == "kv_len":
        kv_len = kv_len + mut[1]
    if kind == "gqa_mod":
        hmap = torch.arange(H, device=q.device) % Hkv
    else:
        hmap = torch.arange(H, device=q.device) // rep
    scale = 1.0 / math.sqrt(D)
    qf, kf, vf = q.float(), k.float()[:, hmap], v.float()[:, hmap]
    ok = _allowed(T, causal, kv_len, q.device)
    if kind == "causal_row":
        ok = ok.clone()
        ok[mut[1], mut[1]:] = False
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale          # fp32 S
    s = s.masked_fill(~ok, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)                                         # fp32 softmax
    l = p.sum(dim=-1, keepdim=True)
    o = (torch.matmul(_r16(p), vf) / l).bfloat16()               # bf16 P, O
    lse = (m + torch.log(l)).squeeze(-1)
    if kind == "o_swap":
        c0 = mut[1]
        o = o.clone()
        o[..., c0:c0 + 32] = torch.cat(
            (o[..., c0 + 16:c0 + 32], o[..., c0:c0 + 16]), dim=-1)
    if do is None:
        return o, lse
    dof = do.float()
    p2 = torch.exp(s - lse.unsqueeze(-1))                        # P from LSE
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)          # rounded O
    ds = _r16(p2 * (dp - delta) * scale)                         # bf16 dS
    p2 = _r16(p2)                                                # bf16 P
    dq = torch.matmul(ds, kf)
    dk_h = torch.matmul(ds.transpose(-1, -2), qf)
    dv_h = torch.matmul(p2.transpose(-1, -2), dof)
    dk = torch.zeros(B, Hkv, T, D, device=q.device).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, device=q.device).index_add_(1, hmap, dv_h)
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


def lse_tolerance(q, k, causal, lse_ref):
    """8 x the error of a plain fp32 torch logsumexp of the fp32 scores
    against fp64 at the same inputs, + 1e-6."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, dim=1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~_allowed(T, causal, T, q.device), float("-inf"))
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


def check_case(got, q, k, v, causal, do, ref=None, every_head=True):
    """Compare a kernel result (out, lse, dq, dk, dv) at the unpadded length
    with ref64 under `close` (floor: base_bf16), the LSE criterion and the
    norm-wise bounds.  Returns (report, failures); never raises.  Each
    failure starts with "<tensor>: <check>" where <check> is one of shape,
    non-finite, dtype, max err (`close`, or the LSE tolerance), tolerance
    (vacuous LSE check), norm-wise."""
    ref = ref64(q, k, v, causal, do) if ref is None else ref
    base = base_bf16(q, k, v, causal, do)
    rep, bad = {}, []
    for i, name in enumerate(NAMES):
        x, r = got[i], ref[i]
        if tuple(x.shape) != tuple(r.shape):
            bad.append(f"{name}: shape {tuple(x.shape)} != {tuple(r.shape)}")
            continue
        if not torch.isfinite(x.float()).all():
            bad.append(f"{name}: non-finite values")
            continue
        if name == "lse":
            tol = lse_tolerance(q, k, causal, r)
            shift = lse_edge_shift(q, k, r, every_head)
            err = max_err(x, r)
            rep[name] = {"err": err, "tol": tol, "shift": shift}
            if x.dtype != torch.float32:
                bad.append(f"lse: dtype {x.dtype}")
            if not tol < shift:
                bad.append(f"lse: tolerance {tol:.3e} not below the "
                           f"one-key shift {shift:.3e} (vacuous check)")
            if not err <= tol:
                bad.append(f"lse: max err {err:.3e} > {tol:.3e}")
            continue
        info = close_info(x, r, base[i])
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


def ratios(rep):
    return {n: round(rep[n]["ratio"], 3) for n in rep if n != "lse"}


# ---------------------------------------------------------------------------
# running the kernels
# ---------------------------------------------------------------------------
def padded_t(T):
    return T + (-T) % 64


device_error = []


def launch_guard(fn):
    """After a device error (they are sticky and surface at the next
    synchronise) nothing more is launched from this process: every later
    call fails at once instead of queueing work on a faulted device."""
    def wrapped(*args, **kw):
        if device_error:
            raise RuntimeError("not launched: earlier device error: "
                               + device_error[0])
        try:
            res = fn(*args, **kw)
            torch.cuda.synchronize()
            return res
        except RuntimeError as e:
            if "HIP error" in str(e) or "hipError" in str(e):
                device_error.append(str(e).splitlines()[0])
            raise
    wrapped.__doc__ = fn.__doc__
    return wrapped


@launch_guard
def kernel_direct(q, k, v, causal, do):
    """ext.attn_fwd / ext.attn_bwd on inputs padded the way the wrapper pads
    them; all five results sliced back to T.  The only route to LSE."""
    from saturn_amd.ops import require_ext
    from saturn_amd.ops.flash import _pad_t64

    ext = require_ext()
    T = q.shape[2]
    qp, kp, vp, dop = (_pad_t64(t) for t in (q, k, v, do))
    o, lse = ext.attn_fwd(qp, kp, vp, causal, T)
    dq, dk, dv = ext.attn_bwd(dop, qp, kp, vp, o, lse, causal, T)
    return tuple(t[:, :, :T] for t in (o, lse, dq, dk, dv))


@launch_guard
def kernel_public(q, k, v, causal, do):
    """flash_attention + autograd on fresh leaves: (out, dq, dk, dv)."""
    from saturn_amd.ops.flash import flash_attention

    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = flash_attention(ql, kl, vl, causal=causal)
    out.backward(do)
    return out.detach(), ql.grad, kl.grad, vl.grad


@launch_guard
def flash_fwd_bwd(q, k, v, causal, do):
    """flash_attention + backward on the caller's own tensors (views of
    leaves, any layout); the gradients land in the caller's leaves."""
    from saturn_amd.ops.flash import flash_attention

    out = flash_attention(q, k, v, causal=causal)
    out.backward(do)
    return out.detach()


@launch_guard
def ext_fwd_bwd(q, k, v, causal, do, kv_len):
    """ext.attn_fwd / ext.attn_bwd as given (T a multiple of 64, explicit
    kv_len), nothing padded or sliced: (out, lse, dq, dk, dv)."""
    from saturn_amd.ops import require_ext

    ext = require_ext()
    o, lse = ext.attn_fwd(q, k, v, causal, kv_len)
    dq, dk, dv = ext.attn_bwd(do, q, k, v, o, lse, causal, kv_len)
    return o, lse, dq, dk, dv


# ---------------------------------------------------------------------------
# --sweep: a compact subset of the path matrix, the ragged and the GQA
# groups, for one setting of the environment switches (they are read once
# per process, so each setting needs a process of its own)
# ---------------------------------------------------------------------------
SWEEP_CASES = [
    # (B, H, Hkv, T, D): a v1-shape T, a v2-shape T and a ragged T per D ...
    *[(1, 3, 3, T, D) for D in (64, 128, 256) for T in (192, 256, 197)],
    # ... and one GQA case (ragged, so kv_len masking and atomics combine)
    (1, 6, 2, 197, 128),
]


def sweep(device="cuda"):
    from saturn_amd.ops import require_ext

    ext = require_ext()
    t0 = time.perf_counter()
    cases, failures, paths, digest = {}, [], {}, 0
    for (B, H, Hkv, T, D) in SWEEP_CASES:
        paths[f"T{padded_t(T)}_D{D}"] = ext.attn_dispatch(padded_t(T), D)
        for causal in (True, False):
            name = f"B{B}H{H}kv{Hkv}T{T}D{D}{'c' if causal else 'n'}"
            q, k, v, do = make_inputs("randn", B, H, Hkv, T, D, device, seed=7)
            got = kernel_direct(q, k, v, causal, do)
            rep, bad = check_case(got, q, k, v, causal, do)
            cases[name] = ratios(rep)
            failures += [f"{name}: {b}" for b in bad]
            if Hkv == H:        # bitwise reproducible outputs only
                for t in got:
                    bits = t.contiguous().view(
                        torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
                    digest = (digest * 31 + int(bits.long().sum())) % (1 << 61)
    torch.cuda.synchronize()
    # digest: informational, shows whether a setting changed any output bit
    return {"cases": cases, "paths": paths, "failures": failures,
            "digest": digest, "seconds": round(time.perf_counter() - t0, 3)}


def main(argv):
    if argv != ["--sweep"]:
        print("usage: attn_ref.py --sweep", file=sys.stderr)
        return 2
    res = sweep()
    print(json.dumps(res), flush=True)
    return 1 if res["failures"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
