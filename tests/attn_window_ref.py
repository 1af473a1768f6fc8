"""Reference, error floor and mutants for attention with a per-row lower key
bound (``kv_lo``: sliding windows and packed documents), shared by
test_attention_window_cpu.py and test_attention_window_gpu.py.

``ref64_lo`` / ``base_bf16_lo`` are ``attn_ref.ref64`` / ``base_bf16`` with
the mask ``lo[b,t] <= j <= t``; the criterion is ``attn_ref``'s own (``close``
with the floor measured on ``base_bf16_lo``, the LSE rule recomputed under
the same mask, the norm-wise bounds).  With ``lo = 0`` both functions run
the very operations of their ``attn_ref`` originals.

This is a plain module: no tests, no fixtures.
"""

from __future__ import annotations

import functools
import math

import torch

import attn_ref as R

# (B, H) of the matrix; every GPU shape has B*H <= 16 and T <= 384
BH = (2, 3)
DS = (64, 128, 256)
KINDS = ("randn", "peaky")
# name -> (T, ("window", W) | ("docs", per-batch document lengths))
BOUNDS = {
    "W17_T192": (192, ("window", 17)),
    "W65_T256": (256, ("window", 65)),
    "W100_T320": (320, ("window", 100)),
    "W200_T384": (384, ("window", 200)),
    "docs_T256": (256, ("docs", ([70, 1, 129, 56], [256]))),
    "docs_T192": (192, ("docs", ([33, 95, 64], [1, 190, 1]))),
}
MATRIX = [(D, bn, kind) for D in DS for bn in BOUNDS for kind in KINDS]


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


def allowed_lo(lo, T, device):
    """bool [T, T] or [B, 1, T, T]: lo[b,t] <= j <= t."""
    ok = R._allowed(T, True, T, device)
    j = torch.arange(T, device=device)
    band = j >= lo.to(device).long().unsqueeze(-1)
    if band.dim() == 3:
        band = band.unsqueeze(1)
    return ok & band


# ---------------------------------------------------------------------------
# the truth and the floor
# ---------------------------------------------------------------------------
def ref64_lo(q, k, v, lo, do=None):
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    need = do is not None
    q64 = q.double().requires_grad_(need)
    k64 = k.double().requires_grad_(need)
    v64 = v.double().requires_grad_(need)
    kr = k64.repeat_interleave(rep, dim=1)
    vr = v64.repeat_interleave(rep, dim=1)
    s = torch.matmul(q64, kr.transpose(-1, -2)) / math.sqrt(D)
    s = s.masked_fill(~allowed_lo(lo, T, q.device), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    out = torch.matmul(torch.exp(s - lse.unsqueeze(-1)), vr)
    if not need:
        return out.detach(), lse.detach()
    dq, dk, dv = torch.autograd.grad(out, (q64, k64, v64), do.double())
    return out.detach(), lse.detach(), dq, dk, dv


def fwd_block_rows(T, D):
    """q rows per forward block under the default dispatch."""
    return 128 if (T % 128 == 0 and D <= 128) else 64


def base_bf16_lo(q, k, v, lo, do=None, mut=None):
    """attn_ref.base_bf16(causal=True) under the bound.  mut plants one bug:
      ("lo_plus",)     lo + 1 on every row, clamped to t
      ("lo_minus",)    lo - 1 on every row, clamped to 0
      ("round_up",)    the forward's first key tile rounded UP from the bound
                       of each block's first row: the keys between are lost
                       to every row of the block (out, lse)
      ("early_stop",)  the dK/dV q loop of each 64-key block stops one
                       32-row tile early (dk, dv)
    """
    B, H, T, D = q.shape
    Hkv = k.shape[1]
    rep = H // Hkv
    kind = mut[0] if mut else None
    dev = q.device
    lo = lo.to(dev)
    t_idx = torch.arange(T, device=dev, dtype=lo.dtype)
    if kind == "lo_plus":
        lo = torch.minimum(lo + 1, t_idx)
    elif kind == "lo_minus":
        lo = (lo - 1).clamp(min=0)
    hmap = torch.arange(H, device=dev) // rep
    scale = 1.0 / math.sqrt(D)
    qf, kf, vf = q.float(), k.float()[:, hmap], v.float()[:, hmap]
    ok = allowed_lo(lo, T, dev)
    ok_fwd = ok
    if kind == "round_up":
        rows = fwd_block_rows(T, D)
        first = (t_idx.long() // rows) * rows                 # block's row 0
        begin = (lo.long()[..., first] + 31) // 32 * 32       # [T] or [B,T]
        late = torch.arange(T, device=dev) >= begin.unsqueeze(-1)
        ok_fwd = ok & (late.unsqueeze(1) if late.dim() == 3 else late)
    s = torch.matmul(qf, kf.transpose(-1, -2)) * scale          # fp32 S
    s_b = s.masked_fill(~ok, float("-inf"))
    s = s.masked_fill(~ok_fwd, float("-inf"))
    m = s.max(dim=-1, keepdim=True).values
    p = torch.exp(s - m)                                         # fp32 softmax
    l = p.sum(dim=-1, keepdim=True)
    o = (torch.matmul(R._r16(p), vf) / l).bfloat16()             # bf16 P, O
    lse = (m + torch.log(l)).squeeze(-1)
    if do is None:
        return o, lse
    dof = do.float()
    p2 = torch.exp(s_b - lse.unsqueeze(-1))                      # P from LSE
    dp = torch.matmul(dof, vf.transpose(-1, -2))
    delta = (dof * o.float()).sum(dim=-1, keepdim=True)          # rounded O
    ds = R._r16(p2 * (dp - delta) * scale)                       # bf16 dS
    p2 = R._r16(p2)                                              # bf16 P
    dq = torch.matmul(ds, kf)
    ds_k, p2_k = ds, p2
    if kind == "early_stop":
        lo2 = (lo if lo.dim() == 2 else lo.unsqueeze(0)).long()  # [B|1, T]
        tiles = torch.arange(0, T, 32, device=dev)               # q tile rows
        kv0 = torch.arange(0, T, 64, device=dev)                 # key blocks
        # stop[b, kb]: first q tile >= kv0 whose first row starts past the
        # block's last key, T if none does
        past = (lo2[:, tiles][:, None, :] > (kv0 + 63)[None, :, None]) & (
            tiles[None, None, :] >= kv0[None, :, None])
        stop = torch.where(past, tiles[None, None, :], T).min(dim=-1).values
        stop = stop - 32                                         # the bug
        q_tile = (torch.arange(T, device=dev) // 32) * 32
        key_blk = torch.arange(T, device=dev) // 64
        seen = q_tile[None, :, None] < stop[:, key_blk][:, None, :]
        seen = seen.unsqueeze(1)                                 # [B|1,1,T,T]
        ds_k, p2_k = ds * seen, p2 * seen
    dk_h = torch.matmul(ds_k.transpose(-1, -2), qf)
    dv_h = torch.matmul(p2_k.transpose(-1, -2), dof)
    dk = torch.zeros(B, Hkv, T, D, device=dev).index_add_(1, hmap, dk_h)
    dv = torch.zeros(B, Hkv, T, D, device=dev).index_add_(1, hmap, dv_h)
    return o, lse, dq.bfloat16(), dk.bfloat16(), dv.bfloat16()


# ---------------------------------------------------------------------------
# the criterion
# ---------------------------------------------------------------------------
def lse_tolerance_lo(q, k, lo, lse_ref):
    """attn_ref.lse_tolerance under the bound: 8 x the error of a plain fp32
    torch logsumexp of the fp32 scores against fp64, + 1e-6."""
    B, H, T, D = q.shape
    rep = H // k.shape[1]
    kf = k.float().repeat_interleave(rep, dim=1)
    s = torch.matmul(q.float(), kf.transpose(-1, -2)) * (1.0 / math.sqrt(D))
    s = s.masked_fill(~allowed_lo(lo, T, q.device), float("-inf"))
    e = (torch.logsumexp(s, dim=-1).double() - lse_ref).abs().max().item()
    return 8.0 * e + 1e-6


def check_case_lo(got, ref, base, lse_tol):
    """A result (out, lse, dq, dk, dv) against ref64_lo under `close` (floor:
    base_bf16_lo), the LSE rule and the norm-wise bounds.  Returns (report,
    failures) like attn_ref.check_case; never raises."""
    rep, bad = {}, []
    for i, name in enumerate(R.NAMES):
        x, r = got[i], ref[i]
        if tuple(x.shape) != tuple(r.shape):
            bad.append(f"{name}: shape {tuple(x.shape)} != {tuple(r.shape)}")
            continue
        if not torch.isfinite(x.float()).all():
            bad.append(f"{name}: non-finite values")
            continue
        if name == "lse":
            err = R.max_err(x, r)
            rep[name] = {"err": err, "tol": lse_tol}
            if x.dtype != torch.float32:
                bad.append(f"lse: dtype {x.dtype}")
            if not err <= lse_tol:
                bad.append(f"lse: max err {err:.3e} > {lse_tol:.3e}")
            continue
        info = R.close_info(x, r, base[i])
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


def rejected(bad):
    """The tensors a failure list names."""
    return {b.split(":", 1)[0] for b in bad}


@functools.lru_cache(maxsize=None)
def case(kind, B, H, Hkv, T, D, bound_key, seed=0):
    """Inputs, bound, truth, floor and LSE tolerance of one case, on the CPU,
    computed once per process and shared (treat as read-only).  bound_key is
    a BOUNDS name, ("window", W) or ("docs", per-batch tuples of lengths)."""
    q, k, v, do = R.make_inputs(kind, B, H, Hkv, T, D, "cpu", seed)
    if isinstance(bound_key, str):
        assert BOUNDS[bound_key][0] == T
        lo = make_bound(bound_key)
    elif bound_key[0] == "window":
        lo = window_bound(T, bound_key[1])
    else:
        lo = docs_bound(bound_key[1], T)
    ref = ref64_lo(q, k, v, lo, do)
    base = base_bf16_lo(q, k, v, lo, do)
    return {"q": q, "k": k, "v": v, "do": do, "lo": lo, "ref": ref,
            "base": base, "lse_tol": lse_tolerance_lo(q, k, lo, ref[1])}


# ---------------------------------------------------------------------------
# running the kernels
# ---------------------------------------------------------------------------
@R.launch_guard
def kernel_direct_lo(q, k, v, do, lo):
    """ext.attn_fwd / ext.attn_bwd with kv_lo, padded the way the wrapper
    pads; all five results sliced back to T.  The only route to LSE."""
    from saturn_amd.ops import require_ext
    from saturn_amd.ops.flash import _pad_t64

    ext = require_ext()
    T = q.shape[2]
    qp, kp, vp, dop = (_pad_t64(t) for t in (q, k, v, do))
    lop = torch.nn.functional.pad(lo, (0, (-T) % 64), value=T - 1).contiguous()
    o, lse = ext.attn_fwd(qp, kp, vp, True, T, kv_lo=lop)
    dq, dk, dv = ext.attn_bwd(dop, qp, kp, vp, o, lse, True, T, kv_lo=lop)
    return tuple(t[:, :, :T] for t in (o, lse, dq, dk, dv))


@R.launch_guard
def kernel_public_lo(q, k, v, do, window=None, kv_lo=None):
    """flash_attention + autograd on fresh leaves: (out, dq, dk, dv)."""
    from saturn_amd.ops.flash import flash_attention

    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = flash_attention(ql, kl, vl, causal=True, window=window, kv_lo=kv_lo)
    out.backward(do)
    return out.detach(), ql.grad, kl.grad, vl.grad


def run_case(c, device="cuda"):
    """Both routes for a `case`: (direct five, public four), on the CPU."""
    q, k, v, do = (c[n].to(device) for n in ("q", "k", "v", "do"))
    lo = c["lo"].to(device)
    direct = kernel_direct_lo(q, k, v, do, lo)
    public = kernel_public_lo(q, k, v, do, kv_lo=lo)
    return (tuple(t.cpu() for t in direct), tuple(t.cpu() for t in public))


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int16 if a.element_size() == 2 else torch.int32),
        b.contiguous().view(torch.int16 if b.element_size() == 2 else torch.int32))


# ---------------------------------------------------------------------------
# --child MODE: what the GPU tests run under an environment switch (the
# switches are read once per process).  Prints one JSON line.
#   matrix   the T=256, D=128 cases of the matrix, both routes, checked
#   refuse   the same call must be refused by attn_bwd; reports the message
# ---------------------------------------------------------------------------
CHILD_CASES = [(128, b, "randn") for b in ("W65_T256", "docs_T256")]


def child_matrix(device="cuda"):
    import time

    from saturn_amd.ops import require_ext

    t0 = time.perf_counter()
    failures = []
    for D, bound, kind in CHILD_CASES:
        T = BOUNDS[bound][0]
        c = case(kind, *BH, BH[1], T, D, bound)
        direct, public = run_case(c, device)
        _, bad = check_case_lo(direct, c["ref"], c["base"], c["lse_tol"])
        failures += [f"{bound}: {b}" for b in bad]
        for i, j in ((0, 0), (1, 2), (2, 3), (3, 4)):
            if not bits_equal(public[i], direct[j]):
                failures.append(f"{bound}: routes differ on {R.NAMES[j]}")
    return {"failures": failures,
            "path": require_ext().attn_dispatch(256, 128, has_lo=True),
            "seconds": round(time.perf_counter() - t0, 3)}


def child_refuse(device="cuda"):
    D, bound, kind = CHILD_CASES[0]
    c = case(kind, *BH, BH[1], BOUNDS[bound][0], D, bound)
    q, k, v, do = (c[n].to(device) for n in ("q", "k", "v", "do"))
    try:
        kernel_direct_lo(q, k, v, do, c["lo"].to(device))
    except RuntimeError as e:
        return {"refused": True, "message": str(e).splitlines()[0]}
    return {"refused": False, "message": ""}


def main(argv):
    import json
    import sys

    if len(argv) != 2 or argv[0] != "--child" or argv[1] not in ("matrix", "refuse"):
        print("usage: attn_window_ref.py --child matrix|refuse", file=sys.stderr)
        return 2
    res = child_matrix() if argv[1] == "matrix" else child_refuse()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    import sys

    sys.exit(main(sys.argv[1:]))
