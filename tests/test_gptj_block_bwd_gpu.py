"""GPT-J block backward as one node (gptj_block_bwd.hip): the RoPE backward
that also stores its result transposed, the transpose into a row slice, and
the autograd function that shares g^T and h^T between the attention and MLP
branches.

The two kernels are checked bit for bit against the kernels they replace
(rope_apply backward, .t().contiguous()).  The function's forward is checked
bit for bit against the unfused block; its gradients, which change summation
order or the number of roundings only, against an fp32 reference (the same
block on the CPU's pure-PyTorch path) with the rule and bound of
test_mlp_bwd_gpu.py: rel_err <= min(2 * e_unfused, 4e-2).
"""

import itertools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

GEMM_TOL = 4e-2  # tests/test_mlp_bwd_gpu.py's bound
SENTINEL = 0x7B7B  # bf16 bit pattern the kernels must leave alone
# (M, N) of tests/test_mlp_bwd_gpu.py
SHAPES = [(8, 8), (64, 64), (200, 328), (1024, 512)]
# (B, T, H, D, rot): one vector, all rotary; one full tile with a copied
# tail; M = 200, E = 72 ragged both ways with the position wrapping at the
# batch edge; many row blocks
ROPE_SHAPES = [(1, 8, 1, 8, 8), (1, 64, 1, 64, 16), (2, 100, 3, 24, 8),
               (2, 512, 4, 64, 64)]
SITE_FLAGS = ("SAMD_ATTN_TN_QKV", "SAMD_ATTN_TN_OUT", "SAMD_DH_ACCUM")


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


def _sentinel_buffer(rows, M):
    buf = torch.empty(rows, M, device="cuda", dtype=torch.bfloat16)
    buf.view(torch.int16).fill_(SENTINEL)
    return buf


def _untouched(t):
    return bool((t.view(torch.int16) == SENTINEL).all())


def _rope_case(B, T, H, D, rot, t_off=0, extra=0):
    from saturn_amd.ops.functional import rope_tables

    g = torch.Generator(device="cuda").manual_seed(B * 1000 + T * 10 + D)
    dy = torch.randn(B, T, H, D, device="cuda", generator=g).bfloat16()
    cos, sin = rope_tables(t_off + T + extra, rot, device="cuda")
    return dy, cos.contiguous(), sin.contiguous()


def _check_rope_bwd_t(B, T, H, D, rot, t_off=0, extra=0):
    ext = _ext()
    dy, cos, sin = _rope_case(B, T, H, D, rot, t_off, extra)
    M, E = B * T, H * D
    ref = torch.empty_like(dy)
    ext.rope_apply(ref, dy, cos, sin, T, t_off, False, True)
    # destination: the middle row slice of a larger sentinel-filled buffer
    buf = _sentinel_buffer(3 * E, M)
    dx = ext.rope_bwd_t(dy, cos, sin, T, t_off, D, buf[E:2 * E])
    assert dx.shape == dy.shape and _same_bits(dx, ref)
    assert _same_bits(buf[E:2 * E], ref.view(M, E).t().contiguous())
    assert _untouched(buf[:E]) and _untouched(buf[2 * E:])
    # deterministic
    buf2 = _sentinel_buffer(3 * E, M)
    dx2 = ext.rope_bwd_t(dy, cos, sin, T, t_off, D, buf2[E:2 * E])
    assert _same_bits(dx2, dx) and _same_bits(buf2, buf)


@pytest.mark.parametrize("B,T,H,D,rot", ROPE_SHAPES)
def test_rope_bwd_t_matches_rope_apply(B, T, H, D, rot):
    _check_rope_bwd_t(B, T, H, D, rot)


def test_rope_bwd_t_with_position_offset():
    # rows t_off .. t_off+T of a longer table
    _check_rope_bwd_t(2, 100, 3, 24, 8, t_off=37, extra=19)


def test_rope_bwd_t_rejects_unsupported_shapes():
    ext = _ext()
    # M = 12: no whole 16-B vector along M
    dy, cos, sin = _rope_case(1, 12, 1, 8, 8)
    with pytest.raises(RuntimeError):
        ext.rope_bwd_t(dy, cos, sin, 12, 0, 8,
                       torch.empty(8, 12, device="cuda", dtype=torch.bfloat16))
    # D = 20: vectors would straddle heads
    dy, cos, sin = _rope_case(1, 8, 2, 20, 8)
    with pytest.raises(RuntimeError):
        ext.rope_bwd_t(dy, cos, sin, 8, 0, 20,
                       torch.empty(40, 8, device="cuda", dtype=torch.bfloat16))


@pytest.mark.parametrize("M,N", SHAPES)
def test_transpose_into_a_row_slice(M, N):
    ext = _ext()
    g = torch.Generator(device="cuda").manual_seed(7 * M + N)
    x = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    buf = _sentinel_buffer(3 * N, M)
    ext.transpose_into(x, buf[N:2 * N])
    assert _same_bits(buf[N:2 * N], x.t().contiguous())
    assert _untouched(buf[:N]) and _untouched(buf[2 * N:])
    with pytest.raises(RuntimeError):
        ext.transpose_into(x, buf[: N + 8])


# ---------------------------------------------------------------------------
# the function against the unfused block
# ---------------------------------------------------------------------------
E_, H_, ROT_, B_, T_ = 128, 2, 16, 2, 64


def _make_block(resid_pdrop=0.0, n_ctx=128, seed=0):
    """Weights drawn as test_mlp_bwd_gpu._make_mlp draws them; the fp32
    master copy is rounded to bf16 first so every run starts from the same
    values."""
    from saturn_amd.models.gptj import GPTJBlock, GPTJConfig

    torch.manual_seed(seed)
    cfg = GPTJConfig(n_embd=E_, n_head=H_, rotary_dim=ROT_, n_ctx=n_ctx,
                     resid_pdrop=resid_pdrop)
    blk = GPTJBlock(cfg)
    with torch.no_grad():
        for n, p in blk.named_parameters():
            if not n.startswith("ln_1"):
                p.normal_(std=0.1)
    return blk.to(torch.bfloat16)


def _inputs(T=T_):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B_, T, E_, generator=g).bfloat16()
    gy = torch.randn(B_, T, E_, generator=g).bfloat16()
    return x, gy


def _branch_node(out):
    """Name of the node that feeds the add3's attention input."""
    return type(out.grad_fn.next_functions[1][0]).__name__


def _run_block(blk, x, gy):
    """Returns block output, attention and MLP branch outputs (captured at
    the add3), dx, parameter grads and the branch node's name."""
    from saturn_amd.models import gptj

    x = x.clone().requires_grad_(True)
    blk.zero_grad(set_to_none=True)
    seen = {}
    orig = gptj.fused_add3

    def spy(a, b, c):
        seen["attn"], seen["mlp"] = b.detach().clone(), c.detach().clone()
        return orig(a, b, c)

    gptj.fused_add3 = spy
    try:
        out = blk(x)
    finally:
        gptj.fused_add3 = orig
    node = _branch_node(out)
    out.backward(gy)
    grads = {n: p.grad.clone() for n, p in blk.named_parameters()}
    grads["x"] = x.grad.clone()
    return out.detach(), seen["attn"], seen["mlp"], grads, node


@pytest.fixture(scope="module")
def block_reference():
    """The block, its inputs, the SAMD_BLOCK_FUSED=0 run and the fp32 CPU
    reference, computed once and left unchanged."""
    import os

    _ext()
    blk = _make_block()
    x, gy = _inputs()
    blk32 = _make_block().float()
    x32 = x.float().requires_grad_(True)
    blk32(x32).backward(gy.float())
    ref = {n: p.grad.clone() for n, p in blk32.named_parameters()}
    ref["x"] = x32.grad.clone()

    blk = blk.cuda()
    old = os.environ.get("SAMD_BLOCK_FUSED")
    os.environ["SAMD_BLOCK_FUSED"] = "0"
    try:
        unfused = _run_block(blk, x.cuda(), gy.cuda())
    finally:
        if old is None:
            del os.environ["SAMD_BLOCK_FUSED"]
        else:
            os.environ["SAMD_BLOCK_FUSED"] = old
    assert "GPTJBranchesFn" not in unfused[4]
    return blk, x.cuda(), gy.cuda(), unfused, ref


def _check_grads(grads, grads_u, ref, tag):
    assert set(grads) == set(grads_u) == set(ref)
    bad = []
    for n in sorted(grads):
        r = ref[n].cuda()
        e_u = rel_err(grads_u[n], r)
        e_f = rel_err(grads[n], r)
        print(f"{tag} {n}: unfused {e_u:.3e} fused {e_f:.3e}")
        if not e_f <= min(2.0 * e_u, GEMM_TOL):
            bad.append((n, e_u, e_f))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("flags", list(itertools.product("01", repeat=3)))
def test_block_matches_unfused(block_reference, monkeypatch, flags):
    blk, x, gy, unfused, ref = block_reference
    out_u, attn_u, mlp_u, grads_u, _ = unfused
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    for name, v in zip(SITE_FLAGS, flags):
        monkeypatch.setenv(name, v)
    out_f, attn_f, mlp_f, grads_f, node = _run_block(blk, x, gy)
    assert "GPTJBranchesFn" in node
    assert _same_bits(attn_f, attn_u)
    assert _same_bits(mlp_f, mlp_u)
    assert _same_bits(out_f, out_u)
    # six weights, two biases, the LayerNorm's pair and dx (which carries dh)
    assert len(grads_f) == 11
    _check_grads(grads_f, grads_u, ref, "".join(flags))
    if flags[2] == "0":
        # without in-GEMM accumulation dh is summed in autograd's order and
        # keeps the unfused path's bits, and with it everything upstream
        same = {n: _same_bits(grads_f[n], grads_u[n])
                for n in ("x", "ln_1.weight", "ln_1.bias")}
        print("bit-equal to unfused:", same)
        assert all(same.values()), same


def test_distinct_branch_gradients(block_reference, monkeypatch):
    """g_a != g_m: the function called directly, two different gradients."""
    from saturn_amd.ops.functional import gptj_branches

    blk, x, gy, _, _ = block_reference
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    g = torch.Generator().manual_seed(5)
    g_a = torch.randn(B_, T_, E_, generator=g).bfloat16()
    g_m = torch.randn(B_, T_, E_, generator=g).bfloat16()
    names = ["attn.q_proj.weight", "attn.k_proj.weight", "attn.v_proj.weight",
             "attn.out_proj.weight", "mlp.fc_in.weight", "mlp.fc_in.bias",
             "mlp.fc_out.weight", "mlp.fc_out.bias"]

    def run(block, h, ga, gm, fused):
        h = h.clone().requires_grad_(True)
        block.zero_grad(set_to_none=True)
        if fused:
            p = dict(block.named_parameters())
            cos, sin = block.attn._rope(h.device)
            a, m = gptj_branches(h, *(p[n] for n in names), cos, sin,
                                 block.attn.n_head)
            assert "GPTJBranchesFn" in type(a.grad_fn).__name__
        else:
            a, m = block.attn(h), block.mlp(h)
        torch.autograd.backward([a, m], [ga, gm])
        p = dict(block.named_parameters())
        out = {n: p[n].grad.clone() for n in names}
        out["h"] = h.grad.clone()
        return out

    h = x  # any [B, T, E] input will do
    blk32 = _make_block().float()
    ref = run(blk32, h.cpu().float(), g_a.float(), g_m.float(), False)
    monkeypatch.setenv("SAMD_MLP_FUSED", "0")
    grads_u = run(blk, h, g_a.cuda(), g_m.cuda(), False)
    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    grads_f = run(blk, h, g_a.cuda(), g_m.cuda(), True)
    _check_grads(grads_f, grads_u, ref, "distinct")


class _Wrapped(nn.Module):
    """Stands in for a tensor-parallel replacement of out_proj."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        return self.inner(x)


def _old_path_bits(blk, x, gy, monkeypatch):
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "0")
    ref = _run_block(blk, x, gy)
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    return ref


def _assert_old_path(run, ref):
    out, attn, mlp, grads, node = run
    assert "GPTJBranchesFn" not in node
    assert _same_bits(out, ref[0])
    assert _same_bits(attn, ref[1]) and _same_bits(mlp, ref[2])
    for n in grads:
        assert _same_bits(grads[n], ref[3][n]), n


def test_hook_takes_the_old_path(block_reference, monkeypatch):
    _, x, gy, unfused, _ = block_reference
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    blk = _make_block().cuda()
    calls = []
    handle = blk.attn.q_proj.register_forward_hook(
        lambda m, i, o: calls.append(1))
    run = _run_block(blk, x, gy)
    handle.remove()
    assert calls == [1]
    _assert_old_path(run, unfused)
    assert "GPTJBranchesFn" in _run_block(blk, x, gy)[4]


def test_wrapped_out_proj_takes_the_old_path(block_reference, monkeypatch):
    _, x, gy, unfused, _ = block_reference
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    blk = _make_block().cuda()
    blk.attn.out_proj = _Wrapped(blk.attn.out_proj)
    run = _run_block(blk, x, gy)
    grads = {n.replace("out_proj.inner.", "out_proj."): g
             for n, g in run[3].items()}
    _assert_old_path(run[:3] + (grads, run[4]), unfused)


def test_resid_dropout_takes_the_old_path(monkeypatch):
    _ext()
    x, gy = _inputs()
    blk = _make_block(resid_pdrop=0.1).cuda()

    def run():
        torch.manual_seed(123)  # the dropout seeds come from this stream
        return _run_block(blk, x.cuda(), gy.cuda())

    monkeypatch.setenv("SAMD_BLOCK_FUSED", "0")
    ref = run()
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1")
    _assert_old_path(run(), ref)


def test_ragged_T_takes_the_old_path(monkeypatch):
    _ext()
    x, gy = _inputs(T=100)
    blk = _make_block().cuda()
    ref = _old_path_bits(blk, x.cuda(), gy.cuda(), monkeypatch)
    _assert_old_path(_run_block(blk, x.cuda(), gy.cuda()), ref)


# ---------------------------------------------------------------------------
# model step: the recipe of test_mlp_bwd_gpu.test_model_step_matches_unfused
# ---------------------------------------------------------------------------
def _gptj_step(fused, monkeypatch, ids, device, dtype):
    from saturn_amd.models.gptj import (GPTJConfig, GPTJForCausalLM,
                                        pretraining_loss)

    monkeypatch.setenv("SAMD_MLP_FUSED", "1")
    monkeypatch.setenv("SAMD_BLOCK_FUSED", "1" if fused else "0")
    torch.manual_seed(0)
    cfg = GPTJConfig(vocab_size=512, n_ctx=64, n_embd=256, n_head=4, n_layer=2)
    model = GPTJForCausalLM(cfg).to(torch.bfloat16).to(device=device, dtype=dtype)
    ids = ids.to(device)
    x = model.wte(ids)
    blk_out = model.h[0](x)
    node = (_branch_node(blk_out) if device == "cuda" else "")
    saved = []
    if "GPTJBranchesFn" in node:
        saved = list(blk_out.grad_fn.next_functions[1][0].saved_tensors)
    loss = pretraining_loss(model(ids), ids)
    loss.backward()
    grads = {n: p.grad.detach() for n, p in model.named_parameters()}
    return loss.detach(), grads, node, saved


def test_model_step_matches_block_unfused(monkeypatch):
    """GPT-J 2 layers, n_embd 256, B=2, T=64, one step.  The fp32 reference
    is the same model on the CPU's pure-PyTorch paths."""
    _ext()
    ids = torch.randint(0, 512, (2, 64), generator=torch.Generator().manual_seed(3))
    loss_u, g_u, node_u, _ = _gptj_step(False, monkeypatch, ids, "cuda",
                                        torch.bfloat16)
    loss_f, g_f, node_f, saved = _gptj_step(True, monkeypatch, ids, "cuda",
                                            torch.bfloat16)
    loss_r, g_r, _, _ = _gptj_step(False, monkeypatch, ids, "cpu",
                                   torch.float32)
    assert "GPTJBranchesFn" in node_f and "GPTJBranchesFn" not in node_u
    assert torch.isfinite(loss_f).all() and torch.equal(loss_f, loss_u)
    _check_grads(g_f, g_u, g_r, "model")
    # the node keeps no [M, 4E] tensor besides pre
    M, E = 2 * 64, 256
    big = [t for t in saved if t.numel() == M * 4 * E]
    assert len(big) == 1 and big[0].shape[-1] == 4 * E
