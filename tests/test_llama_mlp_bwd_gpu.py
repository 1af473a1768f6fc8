"""Llama SwiGLU MLP fused backward (llama_mlp_bwd.hip): `swiglu_bwd_t` bit for
bit against the kernels it replaces and against the formulas in fp64, and the
autograd node / model switch built on it against the unfused path.

Weight gradients change summation order only, so each must sit within twice
the unfused path's own error against fp32 and under tests/test_mlp_bwd_gpu.py's
GEMM bound."""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from attn_ref import close  # noqa: E402

pytestmark = pytest.mark.gpu

# (M, F): one vector; one full tile; ragged both ways; a block walks 4 row
# tiles, so 264 = 256 + 8 gives a second row block of 8 live rows, and 72 a
# second column block of 8 live columns
SHAPES = [(8, 8), (64, 64), (200, 328), (264, 72)]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]
GEMM_TOL = 4e-2
ENV = "SAMD_LLAMA_MLP_"


def _ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _formulas(go, g, u):
    sig = torch.sigmoid(g)
    return go * u * sig * (1 + g * (1 - sig)), go * g * sig, g * sig * u


@pytest.mark.parametrize("want_guT,want_aT", FLAGS)
@pytest.mark.parametrize("M,Fd", SHAPES)
def test_swiglu_bwd_t(M, Fd, want_guT, want_aT):
    ext = _ext()
    gen = torch.Generator(device="cuda").manual_seed(1000 * M + Fd)
    # 2 * randn reaches the zero of silu' near -1.28; +-30 saturates exp
    gate = 2.0 * torch.randn(M, Fd, device="cuda", generator=gen)
    gate[0, 0], gate[-1, -1], gate[M // 2, Fd // 2], gate[-1, 0] = 30, -30, 30, -30
    gate = gate.bfloat16()
    up = torch.randn(M, Fd, device="cuda", generator=gen).bfloat16()
    d_act = torch.randn(M, Fd, device="cuda", generator=gen).bfloat16()

    d_gate, d_up, dguT, act = ext.swiglu_bwd_t(d_act, gate, up, want_guT, want_aT)
    ref_dg, ref_du = ext.swiglu_bwd(d_act, gate, up)
    ref_a = ext.swiglu_fwd(gate, up)
    assert _same_bits(d_gate, ref_dg) and _same_bits(d_up, ref_du)
    assert _same_bits(act, ref_a.t().contiguous() if want_aT else ref_a)
    if want_guT:
        assert _same_bits(dguT, torch.cat((ref_dg, ref_du), 1).t().contiguous())
    else:
        assert dguT.numel() == 0
    again = ext.swiglu_bwd_t(d_act, gate, up, want_guT, want_aT)
    for a, b in zip((d_gate, d_up, dguT, act), again):
        assert _same_bits(a, b)

    ref = _formulas(d_act.double(), gate.double(), up.double())
    floor = [t.bfloat16() for t in _formulas(d_act.float(), gate.float(), up.float())]
    got = (d_gate, d_up, act.t() if want_aT else act)
    for name, x, r, b in zip(("d_gate", "d_up", "act"), got, ref, floor):
        assert torch.isfinite(x.float()).all(), name
        assert close(x, r, b), name
    assert torch.isfinite(dguT.float()).all()


def _make_mlp(E, Fd):
    from saturn_amd.models.llama import LlamaConfig, LlamaMLP

    torch.manual_seed(0)
    mlp = LlamaMLP(LlamaConfig(n_embd=E, ffn_dim=Fd))
    with torch.no_grad():
        for p in mlp.parameters():
            p.normal_(std=0.1)
    return mlp.to(device="cuda", dtype=torch.bfloat16)


def _run_mlp(mlp, x, g):
    x = x.clone().requires_grad_(True)
    mlp.zero_grad(set_to_none=True)
    out = mlp(x)
    node = type(out.grad_fn).__name__
    out.backward(g)
    grads = {n: p.grad.clone() for n, p in mlp.named_parameters()}
    return out.detach(), x.grad.clone(), grads, node


def test_node_matches_unfused_path(monkeypatch):
    _ext()
    M, E, Fd = 136, 64, 200
    mlp = _make_mlp(E, Fd)
    torch.manual_seed(1)
    x = torch.randn(M, E, device="cuda").bfloat16()
    g = torch.randn(M, E, device="cuda").bfloat16()
    monkeypatch.setenv(ENV + "FUSED", "0")
    out_u, dx_u, grads_u, node_u = _run_mlp(mlp, x, g)
    assert "LlamaMlpFn" not in node_u

    x32 = x.float().requires_grad_(True)
    p32 = {n: p.detach().float().requires_grad_(True)
           for n, p in mlp.named_parameters()}
    h32 = F.silu(F.linear(x32, p32["gate_proj.weight"])) * F.linear(
        x32, p32["up_proj.weight"])
    F.linear(h32, p32["down_proj.weight"]).backward(g.float())
    assert len(grads_u) == 3

    monkeypatch.setenv(ENV + "FUSED", "1")
    for tn_gu, tn_down in [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")]:
        monkeypatch.setenv(ENV + "TN_GU", tn_gu)
        monkeypatch.setenv(ENV + "TN_DOWN", tn_down)
        out_f, dx_f, grads_f, node_f = _run_mlp(mlp, x, g)
        assert "LlamaMlpFn" in node_f
        assert _same_bits(out_f, out_u) and _same_bits(dx_f, dx_u)
        for n in sorted(grads_u):
            e_u = rel_err(grads_u[n], p32[n].grad)
            e_f = rel_err(grads_f[n], p32[n].grad)
            print(f"gu={tn_gu} down={tn_down} {n}: unfused {e_u:.3e} fused {e_f:.3e}")
            assert e_f <= min(2.0 * e_u, GEMM_TOL), (tn_gu, tn_down, n, e_u, e_f)
        _, dx_2, grads_2, _ = _run_mlp(mlp, x, g)
        assert _same_bits(dx_2, dx_f)
        assert all(_same_bits(grads_2[n], grads_f[n]) for n in grads_f)


def test_saved_tensors_hold_gate_and_up_only(monkeypatch):
    _ext()
    monkeypatch.setenv(ENV + "FUSED", "1")
    M, E, Fd = 136, 64, 200
    mlp = _make_mlp(E, Fd)
    x = torch.randn(M, E, device="cuda").bfloat16().requires_grad_(True)
    out = mlp(x)
    assert "LlamaMlpFn" in type(out.grad_fn).__name__
    big = [t for t in out.grad_fn.saved_tensors if t.numel() == M * Fd]
    assert len(big) == 2
    assert _same_bits(big[0], F.linear(x.detach(), mlp.gate_proj.weight))
    assert _same_bits(big[1], F.linear(x.detach(), mlp.up_proj.weight))


def _llama_step(fused, ids, device, dtype, hook=False):
    from saturn_amd.models.llama import LlamaConfig, LlamaForCausalLM, llama_loss

    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, n_ctx=64, n_embd=256, n_head=4,
                      n_kv_head=2, n_layer=2, ffn_dim=328, fused_mlp_bwd=fused)
    # every run starts from the same bf16-rounded weights
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).to(device=device, dtype=dtype)
    nodes = []
    model.h[0].mlp.register_forward_hook(
        lambda m, i, o: nodes.append(type(o.grad_fn).__name__))
    if hook:
        for blk in model.h:
            blk.mlp.down_proj.register_forward_hook(lambda m, i, o: None)
    ids = ids.to(device)
    loss = llama_loss(model(ids), ids)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    return loss.detach(), grads, nodes[0]


def test_model_step_matches_unfused(monkeypatch):
    _ext()
    monkeypatch.delenv(ENV + "FUSED", raising=False)
    ids = torch.randint(0, 512, (2, 64), generator=torch.Generator().manual_seed(3))
    loss_u, g_u, node_u = _llama_step(False, ids, "cuda", torch.bfloat16)
    loss_f, g_f, node_f = _llama_step(True, ids, "cuda", torch.bfloat16)
    loss_r, g_r, _ = _llama_step(False, ids, "cpu", torch.float32)
    assert "LlamaMlpFn" not in node_u and "LlamaMlpFn" in node_f
    assert torch.isfinite(loss_f).all() and torch.equal(loss_f, loss_u)
    assert set(g_f) == set(g_u) == set(g_r)
    worst = []
    for n in sorted(g_f):
        ref = g_r[n].cuda()
        e_u, e_f = rel_err(g_u[n], ref), rel_err(g_f[n], ref)
        print(f"{n}: unfused {e_u:.3e} fused {e_f:.3e}")
        if not e_f <= min(2.0 * e_u, GEMM_TOL):
            worst.append((n, e_u, e_f))
    assert not worst, worst


@pytest.mark.parametrize("case", ["hook_on_down_proj", "M12"])
def test_model_fallbacks_take_the_unfused_path(monkeypatch, case):
    _ext()
    monkeypatch.delenv(ENV + "FUSED", raising=False)
    shape, hook = ((1, 12), False) if case == "M12" else ((2, 64), True)
    ids = torch.randint(0, 512, shape, generator=torch.Generator().manual_seed(3))
    loss_u, g_u, _ = _llama_step(False, ids, "cuda", torch.bfloat16, hook)
    loss_f, g_f, node_f = _llama_step(True, ids, "cuda", torch.bfloat16, hook)
    assert "LlamaMlpFn" not in node_f
    assert torch.equal(loss_f, loss_u)
    assert all(_same_bits(g_f[n], g_u[n]) for n in g_u)
