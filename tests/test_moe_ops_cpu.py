"""CPU tests for the MoE ops' torch fallbacks (saturn_amd.ops.moe) and the
fused-vs-loop expert stage (models/mixtral.moe_experts_forward).  The GPU
kernels carry the same contract; tests/test_moe_ops_gpu.py checks them."""

import torch

from saturn_amd.models.mixtral import (
    MixtralConfig,
    MoEMLP,
    moe_experts_forward,
    route,
)
from saturn_amd.ops import moe_combine, moe_permute, moe_route, moe_sort

TINY = {"n_layer": 2, "n_embd": 64, "n_head": 2, "n_kv_head": 1,
        "vocab_size": 128, "n_ctx": 32, "ffn_dim": 96, "n_expert": 4,
        "top_k": 2}


def _tiny_cfg():
    return MixtralConfig(**TINY)


def _check_sort_contract(ids, n_expert):
    order, pos, counts = moe_sort(ids, n_expert)
    flat = ids.reshape(-1).long()
    assert order.dtype == pos.dtype == counts.dtype == torch.int32
    assert torch.equal(order.long(), torch.argsort(flat, stable=True))
    assert torch.equal(counts.long(), torch.bincount(flat, minlength=n_expert))
    assert pos.shape == ids.shape
    # pos is the inverse of order
    assert torch.equal(order.long()[pos.reshape(-1).long()],
                       torch.arange(flat.numel()))
    return order, pos, counts


def test_route_fallback_matches_route_maths():
    torch.manual_seed(0)
    logits = torch.randn(257, 8)
    # tie-free by construction of randn in fp32; make sure of it
    srt = logits.sort(dim=-1)[0]
    assert (srt[:, 1:] - srt[:, :-1]).min() > 0
    w, ids = moe_route(logits, 2)
    probs = torch.softmax(logits.float(), dim=-1)
    topv, topi = probs.topk(2, dim=-1)
    topv = topv / topv.sum(dim=-1, keepdim=True)
    assert ids.dtype == torch.int32
    assert torch.equal(ids.long(), topi)
    assert torch.allclose(w, topv, atol=1e-7)

    # and it equals route() itself through a router
    router = torch.nn.Linear(64, 8, bias=False)
    x = torch.randn(33, 64)
    w0, i0 = route(router, x, 2)
    w1, i1 = moe_route(router(x), 2)
    assert torch.equal(i1.long(), i0)
    assert torch.allclose(w1, w0, atol=1e-7)


def test_route_fallback_ties_pick_lower_index():
    logits = torch.tensor([
        [1.0, 3.0, 3.0, 3.0, 0.0, 3.0, -1.0, 2.0],   # 4-way tie at the top
        [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5],    # all equal
        [0.0, 2.0, 1.0, 1.0, 1.0, -3.0, 1.0, 0.0],   # tie at the boundary
    ])
    w, ids = moe_route(logits, 2)
    assert ids.tolist() == [[1, 2], [0, 1], [1, 2]]
    assert torch.allclose(w[0], torch.tensor([0.5, 0.5]))
    assert torch.allclose(w.sum(-1), torch.ones(3))
    _, ids3 = moe_route(logits, 3)
    assert ids3.tolist() == [[1, 2, 3], [0, 1, 2], [1, 2, 3]]


def test_route_fallback_gradient_formula():
    """dlogits of the fallback (autograd) equals the closed form the kernel
    implements: dlogit_e = p_e (g_e - sum_f p_f g_f)."""
    torch.manual_seed(1)
    logits = torch.randn(19, 8, requires_grad=True)
    w, ids = moe_route(logits, 2)
    dw = torch.randn_like(w)
    (w * dw).sum().backward()
    p = torch.softmax(logits.detach(), dim=-1)
    S = p.gather(-1, ids.long()).sum(-1, keepdim=True)
    wj = p.gather(-1, ids.long()) / S
    gj = (dw - (dw * wj).sum(-1, keepdim=True)) / S
    g = torch.zeros_like(p).scatter(-1, ids.long(), gj)
    ref = p * (g - (p * g).sum(-1, keepdim=True))
    assert torch.allclose(logits.grad, ref, atol=1e-6)


def test_sort_fallback_contract():
    torch.manual_seed(0)
    ids = torch.stack([torch.randperm(8)[:2] for _ in range(300)])
    _, _, counts = _check_sort_contract(ids.to(torch.int32), 8)
    assert int(counts.sum()) == 600
    # int64 ids (what topk returns) are accepted too
    _check_sort_contract(ids, 8)


def test_sort_fallback_empty_expert_and_single_expert():
    torch.manual_seed(0)
    # expert 2 never chosen
    pool = torch.tensor([0, 1, 3])
    ids = torch.stack([pool[torch.randperm(3)[:2]] for _ in range(67)])
    _, _, counts = _check_sort_contract(ids.to(torch.int32), 4)
    assert counts[2] == 0
    # every token goes to one expert (top-1)
    ids = torch.full((129, 1), 3, dtype=torch.int32)
    order, _, counts = _check_sort_contract(ids, 4)
    assert counts.tolist() == [0, 0, 0, 129]
    assert torch.equal(order.long(), torch.arange(129))


def test_permute_combine_fallback():
    torch.manual_seed(0)
    N, k, H = 37, 2, 16
    ids = torch.stack([torch.randperm(4)[:k] for _ in range(N)]).int()
    order, pos, _ = moe_sort(ids, 4)
    x = torch.randn(N, H)
    xs = moe_permute(x, order, pos)
    assert torch.equal(xs, x[order.long() // k])
    w = torch.rand(N, k)
    y = torch.randn(N * k, H)
    out = moe_combine(y, w, pos)
    ref = torch.zeros(N, H)
    for j in range(k):
        ref += w[:, j:j + 1] * y[pos[:, j].long()]
    assert torch.allclose(out, ref, atol=1e-6)


def _expert_stage(dispatch, mlp, xf, empty_expert=None):
    for p in mlp.parameters():
        p.grad = None
    x = xf.clone().requires_grad_(True)
    logits = mlp.router(x)
    if empty_expert is not None:
        logits = logits.clone()
        logits[:, empty_expert] = -1e4
    w, ids = moe_route(logits, mlp.top_k)
    w = w.detach().requires_grad_(True)
    out = moe_experts_forward(x, w, ids, mlp.experts, dispatch)
    g = torch.Generator().manual_seed(5)
    (out * torch.randn(out.shape, generator=g)).sum().backward()
    grads = {n: p.grad.clone() for n, p in mlp.experts.named_parameters()
             if p.grad is not None}
    return out.detach(), x.grad.clone(), w.grad.clone(), grads, ids


def test_experts_forward_fused_matches_loop():
    torch.manual_seed(0)
    mlp = MoEMLP(_tiny_cfg())
    xf = torch.randn(64, TINY["n_embd"])
    for empty in (None, 1):
        o1, dx1, dw1, g1, ids = _expert_stage("loop", mlp, xf, empty)
        o2, dx2, dw2, g2, _ = _expert_stage("fused", mlp, xf, empty)
        if empty is not None:
            assert not (ids == empty).any()
        assert torch.allclose(o1, o2, atol=1e-5)
        assert torch.allclose(dx1, dx2, atol=1e-5)
        assert torch.allclose(dw1, dw2, atol=1e-5)
        assert g1.keys() == g2.keys() and len(g1) > 0
        for n in g1:
            assert torch.allclose(g1[n], g2[n], atol=1e-5), n


def test_moemlp_cpu_auto_dispatch_is_loop(monkeypatch):
    import saturn_amd.models.mixtral as mx

    seen = []
    real = mx.moe_experts_forward

    def spy(xf, weights, ids, experts, dispatch):
        seen.append(dispatch)
        return real(xf, weights, ids, experts, dispatch)

    monkeypatch.setattr(mx, "moe_experts_forward", spy)
    torch.manual_seed(0)
    mlp = MoEMLP(_tiny_cfg())
    assert mlp.dispatch is None
    x = torch.randn(2, 8, TINY["n_embd"])
    ref = mlp(x)
    assert seen == ["loop"]
    mlp.dispatch = "fused"
    out = mlp(x)
    assert seen == ["loop", "fused"]
    assert torch.allclose(out, ref, atol=1e-5)


def test_ep_world1_takes_same_helper():
    from saturn_amd.parallel.expert import DistributedMoE

    torch.manual_seed(0)
    mlp = MoEMLP(_tiny_cfg())
    ep = DistributedMoE(mlp)
    x = torch.randn(2, 8, TINY["n_embd"])
    ref = mlp(x)
    assert torch.equal(ep(x), ref)
    ep.dispatch = "fused"
    assert torch.allclose(ep(x), ref, atol=1e-5)
