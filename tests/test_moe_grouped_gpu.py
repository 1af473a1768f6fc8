"""The grouped expert GEMMs (moe_gemm.hip, K17) and dispatch="grouped":
numerics against fp64 under the attention tests' criterion, bitwise segment
isolation, hipGraph capture, the fused path, a model step, refusals."""

import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import moe_grouped_ref as gr  # noqa: E402
from test_moe_ops_gpu import _run_stage, rel_err, tie_free_logits  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(gr.COUNTS, 96, 160), (gr.COUNTS, 256, 128), ((300,), 96, 160),
         ((0, 0, 0, 70), 96, 160)]
TINY = dict(n_embd=64, ffn_dim=96, n_expert=4, top_k=2, n_head=2, n_kv_head=1,
            n_layer=1, vocab_size=128, n_ctx=32)


@pytest.mark.parametrize("counts,K,Nout", CASES)
def test_grouped_gemms_match_fp64(counts, K, Nout):
    xs, ws, dy, ref, base = gr.problem(counts, K, Nout)
    got = gr.run(xs, counts, ws, dy, "cuda")
    for i, (g, r, b) in enumerate(zip(got, ref, base)):  # y, dx, dw_0, ...
        info = ar.close_info(g.cpu(), r, b)
        print(f"{counts} K{K} N{Nout} [{i}]: {info}")
        assert info["ok"], i
    # an empty expert's gradient is exactly zero
    assert not any(d.any() for c, d in zip(counts, got[2:]) if not c)


def test_segments_are_isolated_bitwise():
    counts, K, Nout = CASES[0]
    xs, ws, dy, _, _ = gr.problem(counts, K, Nout)
    xs, dy = xs.cuda(), dy.cuda()
    full = gr.run(xs, counts, ws, dy, "cuda")
    again = gr.run(xs, counts, ws, dy, "cuda")
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    off = 0
    for e, c in enumerate(counts):
        if c:
            seg = slice(off, off + c)
            ye, dxe, dwe = gr.run(xs[seg], (c,), [ws[e]], dy[seg], "cuda")
            assert torch.equal(ye, full[0][seg]), e
            assert torch.equal(dxe, full[1][seg]), e
            assert torch.equal(dwe, full[2 + e]), e
        off += c


def _stage_setup(empty):
    from saturn_amd.models.mixtral import MixtralConfig, MoEMLP
    from saturn_amd.ops import moe_route

    torch.manual_seed(0)
    mlp = MoEMLP(MixtralConfig(**TINY)).to(device="cuda", dtype=torch.bfloat16)
    x = torch.randn(67, 64, device="cuda").to(torch.bfloat16)
    gout = torch.randn(67, 64, device="cuda").to(torch.bfloat16)
    logits = tie_free_logits(67, 4, torch.bfloat16, seed=7)
    if empty is not None:
        logits[:, empty] = -100.0
    w, ids = moe_route(logits, 2)
    assert empty is None or not (ids == empty).any()
    return mlp.experts, x, gout, w, ids


def test_grouped_stage_captures_into_a_graph():
    from saturn_amd.models.mixtral import moe_experts_forward

    experts, x, gout, w1, ids1 = _stage_setup(None)
    _, _, _, w2, ids2 = _stage_setup(1)
    params = list(experts.parameters())
    x.requires_grad_(True)
    s_w, s_ids = w1.clone(), ids1.clone()

    def step(w, ids):
        out = moe_experts_forward(x, w, ids, experts, "grouped")
        return (out,) + torch.autograd.grad(out, [x] + params, gout)

    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step(s_w, s_ids)  # the eager call itself never synchronises
    finally:
        torch.cuda.set_sync_debug_mode(mode)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(s_w, s_ids)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = step(s_w, s_ids)
    s_w.copy_(w2)
    s_ids.copy_(ids2)
    graph.replay()
    torch.cuda.synchronize()
    eager = step(w2, ids2)
    assert len(eager) == len(static) == 2 + 3 * 4
    for i, (a, b) in enumerate(zip(static, eager)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize("empty", [None, 1], ids=["all_used", "one_empty"])
def test_expert_stage_grouped_no_worse_than_fused(empty):
    experts, x, gout, w, ids = _stage_setup(empty)
    experts32 = copy.deepcopy(experts).float()
    a = _run_stage(experts, x, w, ids, "grouped", gout)
    b = _run_stage(experts, x, w, ids, "fused", gout)
    c = _run_stage(experts32, x.float(), w.float(), ids, "loop", gout.float())
    # the loop and fused paths leave an unused expert without a gradient;
    # grouped gives it one, exactly zero
    assert b[2].keys() == c[2].keys() and len(a[2]) == 12 >= len(c[2]) >= 9
    assert not any(a[2][n].any() for n in a[2].keys() - c[2].keys())
    named = [("out", a[0], b[0], c[0]), ("dx", a[1], b[1], c[1])]
    named += [(n, a[2][n], b[2][n], c[2][n]) for n in c[2]]
    for name, fa, fb, fc in named:
        ea, eb = rel_err(fa, fc), rel_err(fb, fc)
        print(f"stage[{empty}] {name}: grouped {ea:.3g} fused {eb:.3g}")
        assert ea <= eb + 2.0 ** -9, name


def test_mixtral_tiny_bf16_train_step_grouped():
    from saturn_amd.models.mixtral import get_mixtral_model, mixtral_loss
    from saturn_amd.ops.optim import FusedSGD

    model = get_mixtral_model(dict(TINY, n_layer=2)).to("cuda", torch.bfloat16)
    x = torch.randint(0, 128, (2, 32), device="cuda")
    with torch.no_grad():
        fused = mixtral_loss(model(x), x).item()
    for block in model.h:
        block.mlp.dispatch = "grouped"
    opt = FusedSGD(model.parameters(), lr=1e-3)
    loss = mixtral_loss(model(x), x)
    loss.backward()
    rg = model.h[0].mlp.router.weight.grad
    assert torch.isfinite(loss.detach()).item() and torch.isfinite(rg).all()
    assert rg.float().abs().sum().item() > 0
    assert abs(loss.item() - fused) <= 2.0 ** -7 * abs(fused)
    opt.step()
    torch.cuda.synchronize()


@pytest.mark.parametrize("what,named", [
    ("fp32_weight", "weights must be bf16"), ("k40", r"weights: K \(40\)"),
    ("unequal", "weights must all have the same shape"),
    ("counts_int64", "counts must be int32")])
def test_launcher_refuses_by_name(what, named):
    from saturn_amd.ops import require_ext

    K = 40 if what == "k40" else 64
    xs = torch.randn(8, K, device="cuda").bfloat16()
    ws = [torch.randn(32, K, device="cuda").bfloat16() for _ in range(2)]
    counts = torch.tensor([3, 5], dtype=torch.int32, device="cuda")
    bad = {"fp32_weight": ws[1].float(), "unequal": ws[1][:16]}
    ws[1] = bad.get(what, ws[1])
    counts = counts.long() if what == "counts_int64" else counts
    with pytest.raises(RuntimeError, match=named):
        require_ext().moe_gemm_fwd(xs, counts, ws)

