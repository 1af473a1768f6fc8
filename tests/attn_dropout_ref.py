"""Reference, error floor and cases for attention dropout (attn_pdrop fused
into the K2 kernels), shared by test_attention_dropout_cpu.py,
test_attention_dropout_gpu.py and the switch child process
(``python tests/attn_dropout_ref.py --child matrix|refuse``).

* ``ref64_drop``      attn_ref.ref64 with a given bool keep mask Z [B,H,T,T]
                      and factor r: out = (r Z o P) V in fp64, autograd grads.
* ``base_bf16_drop``  attn_ref.base_bf16 with the roundings the kernels make
                      by design: softmax statistics from the undropped
                      scores, Z applied to the bf16-rounded P, r folded into
                      the 1/l epilogue; backward dV from bf16 (P o Z) with r in
                      the epilogue, dS = P o (r Z o dP - delta) * scale in fp32
                      then bf16.  With an all-true mask and r = 1 both run the
                      very operations of the originals (multiplications by 1).
                      ``mut`` plants one bug for the mutation check.

The mask is always the Python twin ``saturn_amd.ops.flash.dropout_keep``; the
criterion is attn_ref's ``close`` with the floor measured on
``base_bf16_drop``, never on a kernel.  A plain module: no tests.
"""

from __future__ import annotations

import functools
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

from saturn_amd.ops.flash import dropout_keep, dropout_threshold  # noqa: E402

NAMES = R.NAMES
BH = (1, 2)                       # (B, H) of the numerics matrix
DS = (64, 128, 256)
SEED = 0x5EED_0D20_0F_A77
# group C: D x T x causal x kind x p.  T=192 reaches the v1 forward, T=256
# the v2 forward at D <= 128; both are several kv tiles and q blocks.
MATRIX = [(D, T, causal, kind, p)
          for D in DS for T in (192, 256) for causal in (True, False)
          for kind in ("randn", "peaky") for p in (0.1, 0.5)]
MUTANTS = {
    # name: tensors `close` must reject it on
    "transpose": ("out", "dq", "dk", "dv"),
    "head": ("out", "dq", "dk", "dv"),
    "shift": ("out", "dq", "dk", "dv"),
    "bwd_seed": ("dq", "dk", "dv"),
    "no_r_dp": ("dq", "dk"),
    "no_r_fwd": ("out",),
}


def keep_r(seed, B, H, T, p, device="cpu"):
    """(Z bool [B,H,T,T], r): the twin mask and the kernels' fp32 factor."""
    return dropout_keep(seed, B, H, T, p, device), dropout_threshold(p)[1]


# ---------------------------------------------------------------------------
# the truth
# ---------------------------------------------------------------------------
def ref64_drop(q, k, v, causal, keep, r, do=None):
    """fp64 attention of the bf16-rounded inputs with dropout mask `keep` and
    factor `r`; LSE is that of the undropped scores."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    need = do is not None
    q64 = q.double().requires_grad_(need)
    k64 = k.double().requires_grad_(need)
    v64 = v.double().requires_grad_(need)
    kr = k64.repeat_interleave(rep, dim=1)
    vr = v64.repeat_interleave(rep, dim=1)
    s = torch.matmul(q64, kr.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~R._allowed(T, causal, T, q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1)) * keep.double() * float(r)
    out = torch.matmul(p, vr)
    if not need:
        return out.detach(), lse.detach()
    dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), do.double())
    return out.detach(), lse.detach(), dq, dk, dv


# ---------------------------------------------------------------------------
# the error floor (and, with `mut`, deliberately broken variants of it)
# ---------------------------------------------------------------------------
def base_bf16_drop(q, k, v, causal, keep, r, do=None, kv_len=None, mut=None):
    """attn_ref.base_bf16 with dropout.  mut plants one bug:
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
    kv_len = T if kv_len is None else kv_len
    hmap = torch.arange(H, device=q.device) // rep
    scale = 1.0 / math.sqrt(D)
    r = float(r)
    z = keep
    if kind == "transpose":
        z = z.transpose(-1, -2)
    elif kind == "head":
        z = z.roll(-1, dims=1)
    elif kind == "shift":
        z = z.roll(1, dims=-1)
    zf = z.float()
    zb = mut[1].float() if kind == "bwd_seed" else zf
    qf, kf, vf = q.float(), k.float()[:, hmap], v.float()[:, hmap]
    ok = R._allowed(T, causal, kv_len, q.device)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale          # fp32 S
    s = s.masked_fill(~ok, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)                                         # fp32 softmax
    l = p.sum(dim=-1, keepdim=True)                              # undropped
    r_fwd = 1.0 if kind == "no_r_fwd" else r
    o = (torch.matmul(R._r16(p) * zf, vf) * r_fwd / l).bfloat16()  # bf16 P o Z
    lse = (m + torch.log(l)).squeeze(-1)
    if do is None:
        return o, lse
    dof = do.float()
    p2 = torch.exp(s - lse.unsqueeze(-1))                        # P from LSE
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)          # rounded O
    r_dp = 1.0 if kind == "no_r_dp" else r
    ds = R._r16(p2 * (r_dp * zb * dp - delta) * scale)           # bf16 dS
    p2 = R._r16(p2) * zb                                         # bf16 P o Z
    dq = torch.matmul(ds, kf)
    dk_h = torch.matmul(ds.transpose(-1, -2), qf)
    dv_h = torch.matmul(p2.transpose(-1, -2), dof) * r
    dk = torch.zeros(B, Hkv, T, D, device=q.device).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, device=q.device).index_add_(1, hmap, dv_h)
    return o, lse, dq.bfloat16(), dk.bfloat16(), dv.bfloat16()


# ---------------------------------------------------------------------------
# cases: inputs, mask, truth and floor computed once and shared (read-only)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(kind, B, H, Hkv, T, D, causal, p, seed=SEED):
    q, k, v, do = R.make_inputs(kind, B, H, Hkv, T, D, "cpu", seed=11)
    keep, r = keep_r(seed, B, H, T, p)
    ref = ref64_drop(q, k, v, causal, keep, r, do)
    base = base_bf16_drop(q, k, v, causal, keep, r, do)
    return {"q": q, "k": k, "v": v, "do": do, "keep": keep, "r": r, "p": p,
            "seed": seed, "causal": causal, "ref": ref, "base": base,
            "lse_tol": R.lse_tolerance(q, k, causal, ref[1])}


def check_case_drop(got, c):
    """(out, lse, dq, dk, dv) at the unpadded length against the case's
    ref64_drop under `close` (floor: base_bf16_drop) and the norm-wise
    bounds; LSE against the undropped fp64 LSE under attn_ref's 8x rule.
    lse may be None (the public route has none).  Returns (report,
    failures); never raises."""
    rep, bad = {}, []
    for i, name in enumerate(NAMES):
        x, r = got[i], c["ref"][i]
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
            err = R.max_err(x, r)
            rep[name] = {"err": err, "tol": c["lse_tol"]}
            if x.dtype != torch.float32:
                bad.append(f"lse: dtype {x.dtype}")
            if not err <= c["lse_tol"]:
                bad.append(f"lse: max err {err:.3e} > {c['lse_tol']:.3e}")
            continue
        info = R.close_info(x, r, c["base"][i])
        info["rel"] = R.rel_err(x, r)
        rep[name] = info
        if x.dtype != torch.bfloat16:
            bad.append(f"{name}: dtype {x.dtype}")
        if not info["ok"]:
            bad.append(f"{name}: max err {info['err']:.4e} > tol "
                       f"{info['tol']:.4e} (floor {info['floor']:.4e}, "
                       f"ratio {info['ratio']:.2f})")
        ntol = R.NORM_TOL_FWD if name == "out" else R.NORM_TOL_BWD
        if not info["rel"] < ntol:
            bad.append(f"{name}: norm-wise {info['rel']:.3e} >= {ntol}")
    return rep, bad


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
        b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---------------------------------------------------------------------------
# running the kernels
# ---------------------------------------------------------------------------
@R.launch_guard
def kernel_direct_drop(q, k, v, causal, do, p, seed):
    """ext.attn_fwd / ext.attn_bwd with dropout on inputs padded the way the
    wrapper pads them; all five results sliced back to T."""
    from saturn_amd.ops import require_ext
    from saturn_amd.ops.flash import _pad_t64

    ext = require_ext()
    T = q.shape[2]
    qp, kp, vp, dop = (_pad_t64(t) for t in (q, k, v, do))
    o, lse = ext.attn_fwd(qp, kp, vp, causal, T, dropout_p=p, seed=seed)
    dq, dk, dv = ext.attn_bwd(dop, qp, kp, vp, o, lse, causal, T,
                              dropout_p=p, seed=seed)
    return tuple(t[:, :, :T] for t in (o, lse, dq, dk, dv))


@R.launch_guard
def kernel_public_drop(q, k, v, causal, do, p, seed):
    """flash_attention(dropout_p, seed) + autograd on fresh leaves:
    (out, dq, dk, dv)."""
    from saturn_amd.ops.flash import flash_attention

    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = flash_attention(ql, kl, vl, causal=causal, dropout_p=p, seed=seed)
    out.backward(do)
    return out.detach(), ql.grad, kl.grad, vl.grad


def run_case(c, device="cuda"):
    """Both routes of a case: (direct five, public four)."""
    q, k, v, do = (c[n].to(device) for n in ("q", "k", "v", "do"))
    direct = kernel_direct_drop(q, k, v, c["causal"], do, c["p"], c["seed"])
    public = kernel_public_drop(q, k, v, c["causal"], do, c["p"], c["seed"])
    return direct, public


# ---------------------------------------------------------------------------
# --child MODE: what the GPU tests run under an environment switch (the
# switches are read once per process).  Prints one JSON line.
#   matrix   group C's T=256, D=128 randn cases, both routes, checked
#   refuse   the same backward must be refused; reports the message
# ---------------------------------------------------------------------------
CHILD_CASES = [(128, 256, causal, "randn", 0.1) for causal in (True, False)]


def child_matrix(device="cuda"):
    import time

    from saturn_amd.ops import require_ext

    t0 = time.perf_counter()
    failures = []
    for D, T, causal, kind, p in CHILD_CASES:
        c = case(kind, *BH, BH[1], T, D, causal, p)
        direct, public = run_case(c, device)
        _, bad = check_case_drop(direct, c)
        failures += [f"causal={causal}: {b}" for b in bad]
        for i, j in ((0, 0), (1, 2), (2, 3), (3, 4)):
            if not bits_equal(public[i], direct[j]):
                failures.append(f"causal={causal}: routes differ on {NAMES[j]}")
    return {"failures": failures,
            "path": require_ext().attn_dispatch(256, 128, has_drop=True),
            "seconds": round(time.perf_counter() - t0, 3)}


def child_refuse(device="cuda"):
    D, T, causal, kind, p = CHILD_CASES[0]
    c = case(kind, *BH, BH[1], T, D, causal, p)
    q, k, v, do = (c[n].to(device) for n in ("q", "k", "v", "do"))
    try:
        kernel_direct_drop(q, k, v, causal, do, p, c["seed"])
    except RuntimeError as e:
        return {"refused": True, "message": str(e).splitlines()[0]}
    return {"refused": False, "message": ""}


def main(argv):
    import json

    if len(argv) != 2 or argv[0] != "--child" or argv[1] not in ("matrix", "refuse"):
        print("usage: attn_dropout_ref.py --child matrix|refuse", file=sys.stderr)
        return 2
    res = child_matrix() if argv[1] == "matrix" else child_refuse()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
