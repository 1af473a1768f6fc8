"""GPT-J MLP fused backward (mlp_bwd.hip): the activation backward that also
writes the transposed GEMM operands and the bias gradient, the bf16
transpose-with-column-sum, and the autograd path built on them.

The kernels are checked bit for bit against the kernels they replace
(gelu_fwd / gelu_bwd / .t().contiguous()); the fp32 column sums against the
worst-case bound of an fp32 sum in any order, M * 2^-24 * sum|x|; the weight
and bias gradients, whose summation order changes, against an fp32 reference
with a bound measured on the unfused path in the same test.
"""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (M, F): one vector; one full tile; ragged tiles both ways; many row blocks
SHAPES = [(8, 8), (64, 64), (200, 328), (1024, 512)]
GEMM_TOL = 4e-2  # tests/test_ops_gpu.py's bound for bf16 GEMM-bearing ops


def _ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _act_inputs(M, Fd):
    g = torch.Generator(device="cuda").manual_seed(1000 * M + Fd)
    pre = (2.0 * torch.randn(M, Fd, device="cuda", generator=g)).bfloat16()
    d_act = torch.randn(M, Fd, device="cuda", generator=g).bfloat16()
    return d_act, pre


def _check_colsum(colsum, x):
    """fp32 sum of M terms, any order: |err| <= M * 2^-24 * sum|x| per column."""
    M = x.shape[0]
    x64 = x.double()
    err = (colsum.double() - x64.sum(0)).abs()
    bound = M * 2.0 ** -24 * x64.abs().sum(0)
    worst = (err - bound).max().item()
    print(f"colsum M={M}: max err {err.max().item():.3e}, "
          f"min bound {bound.min().item():.3e}")
    assert colsum.dtype == torch.float32 and colsum.shape == (x.shape[1],)
    assert worst <= 0.0, f"column-sum error exceeds the fp32 bound by {worst}"


@pytest.mark.parametrize("M,Fd", SHAPES)
def test_act_bwd_matches_the_kernels_it_replaces(M, Fd):
    ext = _ext()
    d_act, pre = _act_inputs(M, Fd)
    d_pre, d_preT, actT, db = ext.mlp_act_bwd(d_act, pre)
    ref_d = ext.gelu_bwd(d_act, pre)
    ref_a = ext.gelu_fwd(pre)
    assert _same_bits(d_pre, ref_d)
    assert _same_bits(d_preT, ref_d.t().contiguous())
    assert _same_bits(actT, ref_a.t().contiguous())
    _check_colsum(db, d_pre)
    # deterministic: no atomics anywhere
    again = ext.mlp_act_bwd(d_act, pre)
    for a, b in zip((d_pre, d_preT, actT), again[:3]):
        assert _same_bits(a, b)
    assert torch.equal(db.view(torch.int32), again[3].view(torch.int32))


@pytest.mark.parametrize("M,Fd", SHAPES)
@pytest.mark.parametrize("want_dT,want_aT",
                         [(False, False), (True, False), (False, True)])
def test_act_bwd_without_transposed_stores(M, Fd, want_dT, want_aT):
    """A site that keeps the NT weight gradient gets no transposed store:
    d_preT is empty, and gelu(pre) comes back row-major."""
    ext = _ext()
    d_act, pre = _act_inputs(M, Fd)
    d_pre, d_preT, act, db = ext.mlp_act_bwd(d_act, pre, want_dT, want_aT)
    ref_d = ext.gelu_bwd(d_act, pre)
    ref_a = ext.gelu_fwd(pre)
    assert _same_bits(d_pre, ref_d)
    if want_dT:
        assert _same_bits(d_preT, ref_d.t().contiguous())
    else:
        assert d_preT.numel() == 0
    assert _same_bits(act, ref_a.t().contiguous() if want_aT else ref_a)
    _check_colsum(db, d_pre)


@pytest.mark.parametrize("M,N", SHAPES)
def test_transpose_colsum(M, N):
    ext = _ext()
    g = torch.Generator(device="cuda").manual_seed(7 * M + N)
    x = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    xT, colsum = ext.transpose_colsum(x, True)
    assert _same_bits(xT, x.t().contiguous())
    _check_colsum(colsum, x)
    xT2, colsum2 = ext.transpose_colsum(x, True)
    assert _same_bits(xT, xT2)
    assert torch.equal(colsum.view(torch.int32), colsum2.view(torch.int32))
    xT3, none = ext.transpose_colsum(x, False)
    assert _same_bits(xT3, xT) and none.numel() == 0


def _fp32_mlp(x, w_in, b_in, w_out, b_out):
    pre = F.linear(x, w_in, b_in)
    return F.linear(F.gelu(pre, approximate="tanh"), w_out, b_out)


def _make_mlp(E, seed=0):
    from saturn_amd.models.gptj import GPTJConfig, GPTJMLP

    torch.manual_seed(seed)
    mlp = GPTJMLP(GPTJConfig(n_embd=E))
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


def test_unsupported_shape_is_rejected_and_runs_unfused():
    ext = _ext()
    d_act, pre = _act_inputs(12, 100)
    with pytest.raises(RuntimeError):
        ext.mlp_act_bwd(d_act, pre)
    with pytest.raises(RuntimeError):
        ext.transpose_colsum(pre, True)
    # M = 12, E = 25, F = 100 through the module: old path, right answer
    mlp = _make_mlp(25)
    x = torch.randn(1, 12, 25, device="cuda").bfloat16()
    g = torch.randn(1, 12, 25, device="cuda").bfloat16()
    out, dx, grads, node = _run_mlp(mlp, x, g)
    assert "GPTJMlpFn" not in node
    x32 = x.float().requires_grad_(True)
    p32 = {n: p.detach().float().requires_grad_(True)
           for n, p in mlp.named_parameters()}
    ref = _fp32_mlp(x32, p32["fc_in.weight"], p32["fc_in.bias"],
                    p32["fc_out.weight"], p32["fc_out.bias"])
    ref.backward(g.float())
    assert rel_err(out, ref) < GEMM_TOL
    assert rel_err(dx, x32.grad) < GEMM_TOL
    for n in grads:
        assert rel_err(grads[n], p32[n].grad) < GEMM_TOL, n


def test_function_matches_unfused_path(monkeypatch):
    """M=128, E=64, F=256, both TN flags on.  Output and dh are bit-equal;
    the four parameter gradients change summation order only, so each must
    sit within twice the unfused path's own error against fp32 (and under
    the file-wide GEMM bound)."""
    _ext()
    M, E = 128, 64
    mlp = _make_mlp(E)
    torch.manual_seed(1)
    x = torch.randn(M, E, device="cuda").bfloat16()
    g = torch.randn(M, E, device="cuda").bfloat16()

    monkeypatch.setenv("SAMD_MLP_FUSED", "0")
    out_u, dx_u, grads_u, node_u = _run_mlp(mlp, x, g)
    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    monkeypatch.setenv("SAMD_MLP_TN_IN", "1")
    monkeypatch.setenv("SAMD_MLP_TN_OUT", "1")
    out_f, dx_f, grads_f, node_f = _run_mlp(mlp, x, g)
    assert "GPTJMlpFn" not in node_u and "GPTJMlpFn" in node_f

    assert _same_bits(out_f, out_u)
    assert _same_bits(dx_f, dx_u)

    x32 = x.float().requires_grad_(True)
    p32 = {n: p.detach().float().requires_grad_(True)
           for n, p in mlp.named_parameters()}
    _fp32_mlp(x32, p32["fc_in.weight"], p32["fc_in.bias"],
              p32["fc_out.weight"], p32["fc_out.bias"]).backward(g.float())
    assert set(grads_f) == {"fc_in.weight", "fc_in.bias",
                            "fc_out.weight", "fc_out.bias"}
    for n in sorted(grads_f):
        e_u = rel_err(grads_u[n], p32[n].grad)
        e_f = rel_err(grads_f[n], p32[n].grad)
        print(f"{n}: unfused {e_u:.3e} fused {e_f:.3e}")
        assert e_f <= min(2.0 * e_u, GEMM_TOL), (n, e_u, e_f)

    # every mix of the per-site flags computes the same thing
    for tn_in, tn_out in [("0", "0"), ("1", "0"), ("0", "1")]:
        monkeypatch.setenv("SAMD_MLP_TN_IN", tn_in)
        monkeypatch.setenv("SAMD_MLP_TN_OUT", tn_out)
        out_m, dx_m, grads_m, _ = _run_mlp(mlp, x, g)
        assert _same_bits(out_m, out_u) and _same_bits(dx_m, dx_u)
        for n in sorted(grads_m):
            e_u = rel_err(grads_u[n], p32[n].grad)
            e_m = rel_err(grads_m[n], p32[n].grad)
            assert e_m <= min(2.0 * e_u, GEMM_TOL), (tn_in, tn_out, n, e_u, e_m)


def test_saved_tensors_hold_only_pre(monkeypatch):
    _ext()
    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    M, E = 128, 64
    mlp = _make_mlp(E)
    x = torch.randn(M, E, device="cuda").bfloat16().requires_grad_(True)
    out = mlp(x)
    assert "GPTJMlpFn" in type(out.grad_fn).__name__
    big = [t for t in out.grad_fn.saved_tensors if t.numel() == M * 4 * E]
    assert len(big) == 1
    pre = F.linear(x.detach(), mlp.fc_in.weight, mlp.fc_in.bias)
    assert _same_bits(big[0].view(M, 4 * E), pre)


def _gptj_step(fused, monkeypatch, ids, device, dtype):
    from saturn_amd.models.gptj import (GPTJConfig, GPTJForCausalLM,
                                        pretraining_loss)

    monkeypatch.setenv("SAMD_MLP_FUSED", "1" if fused else "0")
    torch.manual_seed(0)
    cfg = GPTJConfig(vocab_size=512, n_ctx=64, n_embd=256, n_head=4, n_layer=2)
    # every run starts from the same bf16-rounded weights
    model = GPTJForCausalLM(cfg).to(torch.bfloat16).to(device=device, dtype=dtype)
    ids = ids.to(device)
    loss = pretraining_loss(model(ids), ids)
    loss.backward()
    return loss.detach(), {n: p.grad.detach() for n, p in model.named_parameters()}


def test_model_step_matches_unfused(monkeypatch):
    """GPT-J 2 layers, n_embd 256, B=2, T=64, one step.  The fp32 reference
    is the same model on the CPU's pure-PyTorch paths."""
    _ext()
    ids = torch.randint(0, 512, (2, 64), generator=torch.Generator().manual_seed(3))
    loss_u, g_u = _gptj_step(False, monkeypatch, ids, "cuda", torch.bfloat16)
    loss_f, g_f = _gptj_step(True, monkeypatch, ids, "cuda", torch.bfloat16)
    loss_r, g_r = _gptj_step(False, monkeypatch, ids, "cpu", torch.float32)
    assert torch.isfinite(loss_f).all() and torch.equal(loss_f, loss_u)
    assert abs(loss_f.item() - loss_r.item()) < 0.05
    assert set(g_f) == set(g_u) == set(g_r)
    worst = []
    for n in sorted(g_f):
        ref = g_r[n].cuda()
        e_u = rel_err(g_u[n], ref)
        e_f = rel_err(g_f[n], ref)
        print(f"{n}: unfused {e_u:.3e} fused {e_f:.3e}")
        if not e_f <= min(2.0 * e_u, GEMM_TOL):
            worst.append((n, e_u, e_f))
    assert not worst, worst


class _Wrapped(nn.Module):
    """Stands in for a tensor-parallel replacement of fc_in."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def test_non_linear_children_and_hooks_take_the_unfused_path(monkeypatch):
    _ext()
    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    M, E = 128, 64
    mlp = _make_mlp(E)
    x = torch.randn(M, E, device="cuda").bfloat16()
    g = torch.randn(M, E, device="cuda").bfloat16()
    out_f, dx_f, _, node_f = _run_mlp(mlp, x, g)
    assert "GPTJMlpFn" in node_f

    calls = []
    handle = mlp.fc_out.register_forward_hook(lambda m, i, o: calls.append(1))
    out_h, dx_h, _, node_h = _run_mlp(mlp, x, g)
    handle.remove()
    assert "GPTJMlpFn" not in node_h and calls == [1]
    assert _same_bits(out_h, out_f) and _same_bits(dx_h, dx_f)

    mlp.fc_in = _Wrapped(mlp.fc_in)
    out_w, dx_w, _, node_w = _run_mlp(mlp, x, g)
    assert "GPTJMlpFn" not in node_w
    assert _same_bits(out_w, out_f) and _same_bits(dx_w, dx_f)
