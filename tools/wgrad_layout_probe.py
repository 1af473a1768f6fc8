"""Probe: does a GPT-J MLP weight gradient run faster as a TN GEMM?

Usage (on the GPU box):
    python tools/wgrad_layout_probe.py [repeats]

For M = B*T = 8192 and the two MLP weight shapes it times, alternating in
one process,

    NT  dy.t() @ x              today's weight gradient
    TN  F.linear(dyT, xT)       the same product on pre-materialised transposes

and the kernels of mlp_bwd.hip that produce the transposed operands, against
the kernels they replace (gelu_bwd and the two bf16 bias reductions).

Decision per shape: TN is taken only if  t_NT - t_TN  exceeds the extra cost
of producing that shape's transposed operands by more than the min-max spread
of the two GEMM arms.

Then the three sites of the block backward (gptj_block_bwd.hip), by the same
rule:

    QKV    three NT calls dy.t() @ h at [E,E]  against one TN F.linear at
           [3E,M].[E,M]; the TN side pays rope_bwd_t minus the rope_apply
           backward, twice, and one transpose of dV into its slice
           (h^T is shared with fc_in)
    OUT    NT against TN at [E,E]; the TN side pays one transpose of o
           (g^T is shared with fc_out)
    ACCUM  mm + add_  against  addmm_ with beta = 1 at [M,E].[E,E]
"""

from __future__ import annotations

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

M = 8192
E = 4096
FF = 16384
# site, N (rows of dW), K (cols of dW)
SHAPES = [("fc_in ", FF, E), ("fc_out", E, FF)]


def main() -> None:
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    assert repeats >= 10

    import torch
    import torch.nn.functional as F

    from saturn_amd.ops import require_ext

    ext = require_ext()
    torch.manual_seed(0)
    dev = "cuda"

    def once(fn, iters=4):
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters * 1e3  # us per call

    def arms(fns, iters=4):
        """Alternate the arms: warm up, then `repeats` timed rounds."""
        for _ in range(3):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(repeats):
            for k, fn in fns.items():
                t[k].append(once(fn, iters))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}

    def show(name, r):
        med, lo, hi = r
        print(f"  {name:34s} median {med:8.1f} us   min-max {lo:8.1f} - {hi:8.1f}")

    print(f"M={M} E={E} F={FF} bf16, {repeats} alternating repeats")

    # ---- kernels that produce the operands -------------------------------
    pre = (2 * torch.randn(M, FF, device=dev)).bfloat16()
    d_act = torch.randn(M, FF, device=dev).bfloat16()
    g = torch.randn(M, E, device=dev).bfloat16()
    h = torch.randn(M, E, device=dev).bfloat16()
    d_pre = ext.gelu_bwd(d_act, pre)
    k = arms({
        "gelu_bwd (old)": lambda: ext.gelu_bwd(d_act, pre),
        "d_pre.sum(0) bf16 (old db_in)": lambda: d_pre.sum(0),
        "g.sum(0) bf16 (old db_out)": lambda: g.sum(0),
        "mlp_act_bwd dT=0 aT=0": lambda: ext.mlp_act_bwd(d_act, pre, False, False),
        "mlp_act_bwd dT=1 aT=0": lambda: ext.mlp_act_bwd(d_act, pre, True, False),
        "mlp_act_bwd dT=0 aT=1": lambda: ext.mlp_act_bwd(d_act, pre, False, True),
        "mlp_act_bwd dT=1 aT=1": lambda: ext.mlp_act_bwd(d_act, pre, True, True),
        "transpose_colsum(g, sum)": lambda: ext.transpose_colsum(g, True),
        "transpose_colsum(h, no sum)": lambda: ext.transpose_colsum(h, False),
    })
    print("operand kernels:")
    for name, r in k.items():
        show(name, r)
    base = k["mlp_act_bwd dT=0 aT=0"][0]
    extra = {
        "fc_in ": k["mlp_act_bwd dT=1 aT=0"][0] - base
        + k["transpose_colsum(h, no sum)"][0],
        "fc_out": k["mlp_act_bwd dT=0 aT=1"][0] - base
        + k["transpose_colsum(g, sum)"][0],
    }
    old = (k["gelu_bwd (old)"][0] + k["d_pre.sum(0) bf16 (old db_in)"][0]
           + k["g.sum(0) bf16 (old db_out)"][0])
    print(f"  old gelu_bwd + both bias reduces: {old:.1f} us; "
          f"fused pass without transposed stores: {base:.1f} us")
    del pre, d_act, d_pre
    torch.cuda.empty_cache()

    # ---- the two GEMM layouts --------------------------------------------
    gain = 0.0
    for site, n, kk in SHAPES:
        dy = torch.randn(M, n, device=dev).bfloat16()
        x = torch.randn(M, kk, device=dev).bfloat16()
        dyT = dy.t().contiguous()
        xT = x.t().contiguous()
        r = arms({"NT": lambda: dy.t() @ x, "TN": lambda: F.linear(dyT, xT)})
        fl = 2.0 * M * n * kk
        print(f"{site} dW[{n},{kk}]:")
        for name in ("NT", "TN"):
            show(f"{name}  ({fl / r[name][0] / 1e6:6.0f} TF/s)", r[name])
        diff = r["NT"][0] - r["TN"][0]
        spread = max(r["NT"][2] - r["NT"][1], r["TN"][2] - r["TN"][1])
        take = diff - extra[site] > spread
        print(f"  t_NT - t_TN = {diff:.1f} us, extra operand cost "
              f"{extra[site]:.1f} us, spread {spread:.1f} us -> "
              f"{'TN' if take else 'keep NT'}")
        if take:
            gain += diff - extra[site]
        del dy, x, dyT, xT
        torch.cuda.empty_cache()
    print(f"per layer: fused pass saves {old - base:.1f} us over gelu_bwd + "
          f"bias reduces; TN sites net {gain:.1f} us more")

    # ---- the attention sites of the block backward -------------------------
    from saturn_amd.ops.functional import rope_tables

    B, T, H, D, ROT = 16, 512, 16, 256, 64
    assert B * T == M and H * D == E
    cos, sin = rope_tables(T, ROT, device=dev)
    dq_r = torch.randn(B, T, H, D, device=dev).bfloat16()
    dv = torch.randn(M, E, device=dev).bfloat16()
    dqkvT = torch.empty(3 * E, M, device=dev, dtype=torch.bfloat16)
    dx = torch.empty_like(dq_r)
    k = arms({
        "rope_apply backward (old)":
            lambda: ext.rope_apply(dx, dq_r, cos, sin, T, 0, False, True),
        "rope_bwd_t into a slice":
            lambda: ext.rope_bwd_t(dq_r, cos, sin, T, 0, D, dqkvT[:E]),
        "transpose_into a slice (dV, o)":
            lambda: ext.transpose_into(dv, dqkvT[2 * E:]),
    })
    print(f"attention operand kernels (B={B} T={T} H={H} D={D} rot={ROT}):")
    for name, r in k.items():
        show(name, r)
    rope_extra = k["rope_bwd_t into a slice"][0] - k["rope_apply backward (old)"][0]
    tr = k["transpose_into a slice (dV, o)"][0]
    extra_qkv = 2 * rope_extra + tr
    extra_out = tr
    del dq_r, dx

    def verdict(site, old_t, new_t, extra_cost, on, off):
        diff = old_t[0] - new_t[0]
        spread = max(old_t[2] - old_t[1], new_t[2] - new_t[1])
        take = diff - extra_cost > spread
        print(f"  saving {diff:.1f} us, extra operand cost {extra_cost:.1f} us, "
              f"spread {spread:.1f} us -> {site} {on if take else off}")
        return diff - extra_cost if take else 0.0

    # 16 calls per sample here: at 4, one sample of these sub-millisecond
    # arms is a window of 1-3 ms, and a single host hiccup in it sets the
    # min-max spread the rule compares against
    GEMM_ITERS = 16
    hh = torch.randn(M, E, device=dev).bfloat16()
    hT = hh.t().contiguous()
    dys = [torch.randn(M, E, device=dev).bfloat16() for _ in range(3)]
    dqkvT.copy_(torch.cat([d.t() for d in dys]))

    def nt3():
        for d in dys:
            d.t() @ hh

    r = arms({"NT": nt3, "TN": lambda: F.linear(dqkvT, hT)}, GEMM_ITERS)
    fl = 2.0 * M * 3 * E * E
    print(f"QKV dW[3x{E},{E}]:")
    show(f"NT x3      ({fl / r['NT'][0] / 1e6:6.0f} TF/s)", r["NT"])
    show(f"TN [3E,M]  ({fl / r['TN'][0] / 1e6:6.0f} TF/s)", r["TN"])
    net = verdict("QKV", r["NT"], r["TN"], extra_qkv, "TN", "keep NT")
    del dqkvT

    gT = dys[0].t().contiguous()
    r = arms({"NT": lambda: dys[0].t() @ hh, "TN": lambda: F.linear(gT, hT)},
             GEMM_ITERS)
    fl = 2.0 * M * E * E
    print(f"OUT dW[{E},{E}]:")
    for name in ("NT", "TN"):
        show(f"{name}  ({fl / r[name][0] / 1e6:6.0f} TF/s)", r[name])
    net += verdict("OUT", r["NT"], r["TN"], extra_out, "TN", "keep NT")

    W = torch.randn(E, E, device=dev).bfloat16()
    acc = torch.zeros(M, E, device=dev, dtype=torch.bfloat16)
    r = arms({
        "mm + add_": lambda: acc.add_(torch.mm(dys[1], W)),
        "addmm_ beta=1": lambda: acc.addmm_(dys[1], W),
    }, GEMM_ITERS)
    print(f"ACCUM dh[{M},{E}] += dy[{M},{E}] W[{E},{E}]:")
    for name in r:
        show(name, r[name])
    net += 3 * verdict("ACCUM", r["mm + add_"], r["addmm_ beta=1"], 0.0,
                       "addmm_", "keep mm + add_")
    print(f"per layer: the sites that pay net {net:.1f} us "
          f"(ACCUM counted three times)")


if __name__ == "__main__":
    main()
