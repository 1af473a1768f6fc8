"""The torch fallback of moe_grouped_linear against the fp64 reference, and
dispatch="grouped" against dispatch="fused", on the CPU; an unknown dispatch
string is an error."""

import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import moe_grouped_ref as gr  # noqa: E402


def test_grouped_linear_fallback_matches_fp64():
    xs, ws, dy, ref, base = gr.problem(gr.COUNTS, 96, 160)
    got = gr.run(xs, gr.COUNTS, ws, dy, "cpu")
    for i, (g, r, b) in enumerate(zip(got, ref, base)):
        assert ar.close(g, r, b), i
    # an empty expert's gradient is exactly zero
    assert not any(d.any() for c, d in zip(gr.COUNTS, got[2:]) if not c)


def test_grouped_dispatch_matches_fused_on_cpu():
    from saturn_amd.models import mixtral as mx

    torch.manual_seed(0)
    cfg = mx.MixtralConfig(n_embd=64, ffn_dim=96, n_expert=4, top_k=2)
    mlp = mx.MoEMLP(cfg).bfloat16()
    x = torch.randn(67, 64).bfloat16()
    w, ids = mx.route(mlp.router, x, 2)
    res = {}
    for dispatch in ("grouped", "fused"):
        xi = x.clone().requires_grad_(True)
        params = list(mlp.experts.parameters())
        out = mx.moe_experts_forward(xi, w.detach(), ids, mlp.experts,
                                     dispatch)
        grads = torch.autograd.grad(out, [xi] + params, torch.ones_like(out))
        res[dispatch] = (out.detach(),) + grads
    for got, want in zip(res["grouped"], res["fused"]):
        # fused IS the base here: the same fp32 sums rounded at the same places
        assert ar.close(got, want.double(), want)
    with pytest.raises(ValueError, match="unknown MoE dispatch 'bogus'"):
        mx.moe_experts_forward(x, w, ids, mlp.experts, "bogus")
