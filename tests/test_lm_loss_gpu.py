"""Fused lm_head + cross-entropy (lm_loss.hip, K18): numerics against fp64
under the attention tests' criterion, bitwise independence of the chunking,
no host sync and the memory bound, the model flag, refusals."""

import copy
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import lm_loss_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu

# (B, T, K, V, bias, shift, chunk)
CASES = [
    (2, 67, 96, 203, True, True, None),
    (2, 67, 96, 203, True, True, 128),
    (1, 128, 64, 384, False, False, 128),
    (3, 50, 160, 1000, False, True, 256),
]


@pytest.mark.parametrize("B,T,K,V,bias,shift,chunk", CASES)
def test_matches_fp64(B, T, K, V, bias, shift, chunk):
    from saturn_amd.ops import require_ext

    p = lr.problem(B, T, K, V, bias, shift)
    got = lr.run(p, chunk)
    _, lse = require_ext().lce_fwd(
        p.h.view(-1, K).cuda(), p.w.cuda(), None if p.b is None else p.b.cuda(),
        p.tg.cuda(), lr.IGNORE)
    e_loss = abs(got[0].double().item() - p.ref[0].item())
    e_lse = ar.max_err(lse.cpu(), p.ref[1])
    print(f"loss err {e_loss:.3e} tol {p.loss_tol:.3e}; "
          f"lse err {e_lse:.3e} tol {p.lse_tol:.3e}")
    assert got[0].dtype == lse.dtype == torch.float32
    assert e_loss <= p.loss_tol and e_lse <= p.lse_tol
    for name, g, r, b in zip(("dh", "dW", "dbias"), got[1:], p.ref[2:],
                             p.base[2:]):
        info = ar.close_info(g.cpu().reshape(r.shape), r, b)
        print(f"{name}: {info}")
        assert g.dtype == torch.bfloat16 and info["ok"], name
    # ignored rows, the last position under shift among them: dh exactly 0
    dead = p.tg == lr.IGNORE
    assert dead[T - 1] or not shift
    assert not got[1].cpu().view(-1, K)[dead].any()


def test_chunks_and_reruns_bitwise():
    p = lr.problem(*CASES[1][:6])
    first = lr.run(p, None)
    for chunk in (128, 256, None):
        for a, b in zip(first[1:], lr.run(p, chunk)[1:]):
            assert torch.equal(a, b), chunk


def test_no_sync_and_peak_memory():
    from saturn_amd.ops import fused_linear_cross_entropy

    N, K, V = 1024, 128, 8192
    g = torch.Generator().manual_seed(3)
    h = torch.randn(N, K, generator=g).bfloat16().cuda().requires_grad_(True)
    w = (torch.randn(V, K, generator=g) * 0.2).bfloat16().cuda()
    w.requires_grad_(True)
    tg = torch.randint(0, V, (N,), generator=g).cuda()

    def step():
        fused_linear_cross_entropy(h, w, None, tg, chunk=1024).backward()
        h.grad = w.grad = None

    step()  # warm-up: code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak above baseline {peak} B, one logits tensor {N * V * 2} B")
    assert peak < N * V * 2


def _model_step(model, x, loss_fn):
    model.zero_grad(set_to_none=True)
    loss = loss_fn(model(x), x)
    loss.backward()
    return loss.detach().float().cpu()


def _rel(a, b):
    return ar.rel_err(a.detach().cpu().float(), b.detach().cpu().float())


@pytest.mark.parametrize("family", ["gptj", "llama"])
def test_model_flag(family):
    if family == "gptj":
        from saturn_amd.models.gptj import (GPTJConfig, GPTJForCausalLM,
                                            pretraining_loss as loss_fn)
        torch.manual_seed(0)
        model = GPTJForCausalLM(GPTJConfig(
            vocab_size=203, n_ctx=64, n_embd=128, n_head=2, n_layer=2,
            rotary_dim=32))
        torch.nn.init.normal_(model.lm_head.bias, std=0.5)
        norm = lambda m: m.h[0].ln_1.weight  # noqa: E731
    else:
        from saturn_amd.models.llama import (LlamaConfig, LlamaForCausalLM,
                                             llama_loss as loss_fn)
        torch.manual_seed(0)
        model = LlamaForCausalLM(LlamaConfig(
            vocab_size=203, n_ctx=64, n_embd=128, n_head=2, n_kv_head=1,
            n_layer=2, ffn_dim=256))
        norm = lambda m: m.h[0].input_layernorm.weight  # noqa: E731
    model32 = copy.deepcopy(model).float()           # the fp32 truth, on CPU
    model = model.to("cuda", torch.bfloat16)
    x = torch.randint(0, 203, (2, 64), generator=torch.Generator().manual_seed(1))
    _model_step(model32, x, loss_fn)
    want = [model32.lm_head.weight.grad, norm(model32).grad]
    x = x.cuda()
    off = _model_step(model, x, loss_fn)
    e_off = [_rel(model.lm_head.weight.grad, want[0]),
             _rel(norm(model).grad, want[1])]
    model.cfg.fused_lm_loss = True
    on = _model_step(model, x, loss_fn)
    e_on = [_rel(model.lm_head.weight.grad, want[0]),
            _rel(norm(model).grad, want[1])]
    print(f"{family}: loss off {off.item():.6f} on {on.item():.6f}; "
          f"rel err off {e_off} on {e_on}")
    assert abs(on.item() - off.item()) <= 2.0 ** -7 * abs(off.item())
    assert all(a <= b + 2.0 ** -9 for a, b in zip(e_on, e_off))
    model.eval()
    with torch.no_grad():
        flagged = model(x)
        model.cfg.fused_lm_loss = False
        assert isinstance(flagged, torch.Tensor)
        assert torch.equal(flagged, model(x))


@pytest.mark.parametrize("what,named", [
    ("fp32_weight", "weight must be bf16"), ("k40", r"hidden: K \(40\)"),
    ("targets_int32", "targets must be Long"),
    ("lse_short", "lse must be a contiguous 1-D tensor of 8 elements"),
    ("chunk100", r"chunk \(100\)")])
def test_launcher_refuses_by_name(what, named):
    from saturn_amd.ops import require_ext

    K = 40 if what == "k40" else 64
    h = torch.randn(8, K, device="cuda").bfloat16()
    w = torch.randn(32, K, device="cuda").bfloat16()
    w = w.float() if what == "fp32_weight" else w
    tg = torch.zeros(8, dtype=torch.int64, device="cuda")
    tg = tg.int() if what == "targets_int32" else tg
    lse = torch.zeros(7 if what == "lse_short" else 8, device="cuda")
    gscale = torch.ones(1, device="cuda")
    with pytest.raises(RuntimeError, match=named):
        require_ext().lce_bwd(h, w, None, tg, lse, gscale, -100,
                              100 if what == "chunk100" else 0)
