"""GPU numerics tests for the MoE routing / dispatch kernels (moe.hip, K13)
against fp32 torch references, and the fused expert stage against the loop
path it replaces.

Logits are tie-free by construction (each row a random permutation of E
levels `step` apart plus noise of +-step/8, fp32 then cast), so expert ids
must match the reference exactly on every row.
"""

import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

# (N, E, k, hidden)
SHAPES = [
    (1, 8, 2, 64),        # a single token
    (67, 8, 2, 136),      # N not a multiple of a wave; hidden % 64 != 0
    (129, 4, 1, 64),      # top-1
    (257, 16, 2, 1032),   # a row longer than one wave pass of 64 x 8
    (300, 64, 4, 64),     # the largest supported expert count
    (3000, 8, 2, 64),     # the pair count spans several sort blocks
]
DTYPES = [torch.bfloat16, torch.float32]
BOUND = {torch.bfloat16: 2.0 ** -8, torch.float32: 1e-6}


def ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def tie_free_logits(N, E, dtype, seed=0):
    step = 0.5 if E <= 8 else (0.25 if E == 16 else 0.125)
    g = torch.Generator().manual_seed(seed)
    levels = (torch.arange(E, dtype=torch.float32) - E / 2) * step
    perm = torch.stack([torch.randperm(E, generator=g) for _ in range(N)])
    noise = (torch.rand(N, E, generator=g) * 2 - 1) * (step / 8)
    logits = (levels[perm] + noise).to(dtype)
    srt = logits.float().sort(dim=-1)[0]
    assert (srt[:, 1:] - srt[:, :-1]).min() > step / 2  # still tie-free
    return logits.cuda()


def route_reference(logits, k):
    """fp32 torch routing (today's route() maths) with autograd."""
    lf = logits.float().detach().requires_grad_(True)
    probs = torch.softmax(lf, dim=-1)
    topv, topi = probs.topk(k, dim=-1)
    w = topv / topv.sum(dim=-1, keepdim=True)
    return lf, w, topi


_ROUTING = {}


def routing(N, E, k):
    """Reference ids (int32, on GPU) shared by the dispatch tests."""
    key = (N, E, k)
    if key not in _ROUTING:
        _, _, topi = route_reference(tie_free_logits(N, E, torch.float32), k)
        _ROUTING[key] = topi.to(torch.int32).contiguous()
    return _ROUTING[key]


def sort_reference(ids):
    flat = ids.reshape(-1).long().cpu()
    order = torch.argsort(flat, stable=True)
    pos = torch.empty_like(order)
    pos[order] = torch.arange(order.numel())
    return order, pos.view(ids.shape), flat


# ---------------------------------------------------------------------------
# moe_route
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,E,k,H", SHAPES)
def test_moe_route(N, E, k, H, dtype):
    from saturn_amd.ops import moe_route

    ext()
    logits = tie_free_logits(N, E, dtype).requires_grad_(True)
    w, ids = moe_route(logits, k)
    lf, w_ref, ids_ref = route_reference(logits, k)
    assert ids.dtype == torch.int32 and w.dtype == dtype
    assert torch.equal(ids.long(), ids_ref), "ids must match on every row"
    if N >= 64:
        assert torch.bincount(ids.reshape(-1).long(), minlength=E).min() > 0

    # the incoming gradient has the dtype of the weights; the reference gets
    # the same (possibly 16-bit) values in fp32
    dw = torch.randn(N, k, generator=torch.Generator().manual_seed(1))
    dw = dw.to(dtype).cuda()
    w.backward(dw)
    w_ref.backward(dw.float())
    bound = 1e-5 if dtype == torch.float32 else 2.0 ** -8
    e_w = rel_err(w, w_ref)
    if k == 1:
        # top-1: w == 1 whatever the logits, so dlogits is identically zero
        # and the fp32 reference holds only its own rounding noise; measure
        # both against the size of the incoming gradient instead
        scale = dw.float().norm().item()
        assert lf.grad.norm().item() < 1e-5 * scale
        e_d = logits.grad.float().norm().item() / scale
    else:
        e_d = rel_err(logits.grad, lf.grad)
    print(f"route {N,E,k} {dtype}: weights {e_w:.3g} dlogits {e_d:.3g}")
    assert logits.grad.dtype == dtype
    assert e_w < bound
    assert e_d < bound


def test_moe_route_ties_pick_lower_index():
    from saturn_amd.ops import moe_route

    ext()
    logits = torch.tensor([
        [1.0, 3.0, 3.0, 3.0, 0.0, 3.0, -1.0, 2.0],
        [0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5],
        [0.0, 2.0, 1.0, 1.0, 1.0, -3.0, 1.0, 0.0],
    ], device="cuda")
    for dtype in DTYPES:
        w, ids = moe_route(logits.to(dtype), 2)
        assert ids.tolist() == [[1, 2], [0, 1], [1, 2]]
        assert torch.equal(w[:2].float().cpu(), torch.full((2, 2), 0.5))
        _, ids3 = moe_route(logits.to(dtype), 3)
        assert ids3.tolist() == [[1, 2, 3], [0, 1, 2], [1, 2, 3]]


# ---------------------------------------------------------------------------
# moe_sort
# ---------------------------------------------------------------------------
def check_sort(ids, E):
    from saturn_amd.ops import moe_sort

    ext()
    order, pos, counts = moe_sort(ids, E)
    o_ref, p_ref, flat = sort_reference(ids)
    assert order.dtype == pos.dtype == counts.dtype == torch.int32
    assert torch.equal(order.cpu().long(), o_ref)
    assert torch.equal(pos.cpu().long(), p_ref)
    assert torch.equal(counts.cpu().long(), torch.bincount(flat, minlength=E))
    again = moe_sort(ids, E)
    for a, b in zip((order, pos, counts), again):
        assert torch.equal(a, b)
    return counts


@pytest.mark.parametrize("N,E,k,H", SHAPES)
def test_moe_sort(N, E, k, H):
    check_sort(routing(N, E, k), E)


@pytest.mark.parametrize("N,E,k", [(67, 8, 2), (3000, 8, 2), (300, 64, 4)])
def test_moe_sort_empty_expert(N, E, k):
    ids = routing(N, E, k).clone()
    hole = 2
    # re-point every pair of the hole expert at a neighbour
    ids[ids == hole] = hole + 1
    counts = check_sort(ids, E)
    assert counts[hole] == 0


@pytest.mark.parametrize("N,E,k", [(1, 8, 2), (129, 4, 1), (3000, 8, 2)])
def test_moe_sort_single_expert(N, E, k):
    ids = torch.full((N, k), E - 1, dtype=torch.int32, device="cuda")
    counts = check_sort(ids, E)
    assert counts.tolist() == [0] * (E - 1) + [N * k]


# ---------------------------------------------------------------------------
# moe_permute
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,E,k,H", SHAPES)
def test_moe_permute(N, E, k, H, dtype):
    from saturn_amd.ops import moe_permute, moe_sort

    ext()
    order, pos, _ = moe_sort(routing(N, E, k), E)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(N, H, generator=g).to(dtype).cuda().requires_grad_(True)
    xs = moe_permute(x, order, pos)
    assert torch.equal(xs, x.detach()[order.long() // k])

    dxs = torch.randn(N * k, H, generator=g).to(dtype).cuda()
    xs.backward(dxs)
    ref = dxs.float()[pos.reshape(-1).long()].view(N, k, H).sum(dim=1)
    err = rel_err(x.grad, ref)
    print(f"permute bwd {N,E,k,H} {dtype}: {err:.3g}")
    assert err < BOUND[dtype]

    dx1 = x.grad.clone()
    x.grad = None
    xs2 = moe_permute(x, order, pos)
    xs2.backward(dxs)
    assert torch.equal(xs2, xs) and torch.equal(x.grad, dx1)


# ---------------------------------------------------------------------------
# moe_combine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("N,E,k,H", SHAPES)
def test_moe_combine(N, E, k, H, dtype):
    from saturn_amd.ops import moe_combine, moe_sort

    e = ext()
    _, pos, _ = moe_sort(routing(N, E, k), E)
    g = torch.Generator().manual_seed(3)
    y = torch.randn(N * k, H, generator=g).to(dtype).cuda()
    w = torch.rand(N, k, generator=g)
    w = (w / w.sum(-1, keepdim=True)).to(dtype).cuda()
    dout = torch.randn(N, H, generator=g).to(dtype).cuda()

    # fp32 reference from the same (possibly 16-bit) inputs
    yf = y.float().clone().requires_grad_(True)
    wf = w.float().clone().requires_grad_(True)
    rows = yf[pos.reshape(-1).long()].view(N, k, H)
    ref = (rows * wf.unsqueeze(-1)).sum(dim=1)
    ref.backward(dout.float())

    out = moe_combine(y, w, pos)
    dy, dwts = e.moe_combine_bwd(dout, y, w, pos)
    assert out.dtype == dtype and dy.dtype == dtype
    assert dwts.dtype == torch.float32
    errs = (rel_err(out, ref), rel_err(dy, yf.grad), rel_err(dwts, wf.grad))
    print(f"combine {N,E,k,H} {dtype}: out {errs[0]:.3g} dy {errs[1]:.3g} "
          f"dweights {errs[2]:.3g}")
    assert errs[0] < BOUND[dtype]
    assert errs[1] < BOUND[dtype]
    assert errs[2] < 1e-4

    # autograd wrapper returns the same gradients, and runs are bitwise equal
    y2 = y.clone().requires_grad_(True)
    w2 = w.clone().requires_grad_(True)
    out2 = moe_combine(y2, w2, pos)
    out2.backward(dout)
    assert torch.equal(out2, out)
    assert torch.equal(y2.grad, dy)
    assert torch.equal(w2.grad, dwts.to(dtype))


# ---------------------------------------------------------------------------
# expert stage: fused vs the loop path it replaces, both against fp32
# ---------------------------------------------------------------------------
def _run_stage(experts, x, w, ids, dispatch, gout):
    from saturn_amd.models.mixtral import moe_experts_forward

    for p in experts.parameters():
        p.grad = None
    x = x.clone().requires_grad_(True)
    out = moe_experts_forward(x, w, ids, experts, dispatch)
    out.backward(gout.to(out.dtype))
    grads = {n: p.grad.clone() for n, p in experts.named_parameters()
             if p.grad is not None}
    return out.detach(), x.grad.clone(), grads


@pytest.mark.parametrize("empty", [None, 1], ids=["all_used", "one_empty"])
def test_expert_stage_fused_no_worse_than_loop(empty):
    from saturn_amd.models.mixtral import MixtralConfig, MoEMLP
    from saturn_amd.ops import moe_route

    ext()
    torch.manual_seed(0)
    cfg = MixtralConfig(n_embd=64, ffn_dim=96, n_expert=4, top_k=2,
                        n_head=2, n_kv_head=1, n_layer=1, vocab_size=128,
                        n_ctx=32)
    N = 67
    mlp = MoEMLP(cfg).to(device="cuda", dtype=torch.bfloat16)
    experts32 = copy.deepcopy(mlp.experts).float()
    x = torch.randn(N, 64, device="cuda").to(torch.bfloat16)
    logits = tie_free_logits(N, 4, torch.bfloat16, seed=7)
    if empty is not None:
        logits[:, empty] = -100.0
    w, ids = moe_route(logits, 2)  # one routing result for every path
    if empty is not None:
        assert not (ids == empty).any()
    gout = torch.randn(N, 64, device="cuda").to(torch.bfloat16)

    a = _run_stage(mlp.experts, x, w, ids, "fused", gout)
    b = _run_stage(mlp.experts, x, w, ids, "loop", gout)
    c = _run_stage(experts32, x.float(), w.float(), ids, "loop", gout.float())

    slack = 2.0 ** -9
    for name, fa, fb, fc in (("out", a[0], b[0], c[0]),
                             ("dx", a[1], b[1], c[1])):
        ea, eb = rel_err(fa, fc), rel_err(fb, fc)
        print(f"stage[{empty}] {name}: fused {ea:.3g} loop {eb:.3g}")
        assert ea <= eb + slack, name
    assert a[2].keys() == b[2].keys() == c[2].keys() and len(c[2]) > 0
    for n in c[2]:
        ea, eb = rel_err(a[2][n], c[2][n]), rel_err(b[2][n], c[2][n])
        print(f"stage[{empty}] {n}: fused {ea:.3g} loop {eb:.3g}")
        assert ea <= eb + slack, n


# ---------------------------------------------------------------------------
# full model
# ---------------------------------------------------------------------------
def test_mixtral_tiny_bf16_train_step_uses_fused_dispatch():
    from saturn_amd.models.mixtral import (
        get_mixtral_model,
        mixtral_loss,
        resolve_dispatch,
    )
    from saturn_amd.ops.optim import FusedSGD

    e = ext()
    for name in ("moe_route_fwd", "moe_sort", "moe_permute_fwd",
                 "moe_combine_fwd"):
        assert hasattr(e, name), f"extension lacks {name}"

    tiny = {"n_layer": 2, "n_embd": 64, "n_head": 2, "n_kv_head": 1,
            "vocab_size": 128, "n_ctx": 32, "ffn_dim": 96, "n_expert": 4,
            "top_k": 2}
    model = get_mixtral_model(tiny).to(device="cuda", dtype=torch.bfloat16)
    mlp = model.h[0].mlp
    probe = torch.empty(1, 64, device="cuda", dtype=torch.bfloat16)
    assert resolve_dispatch(mlp.dispatch, probe) == "fused"

    opt = FusedSGD(model.parameters(), lr=1e-3)
    x = torch.randint(0, 128, (2, 32), device="cuda")
    loss = mixtral_loss(model(x), x)
    loss.backward()
    assert torch.isfinite(loss.detach()).item()
    rg = mlp.router.weight.grad
    assert rg is not None and torch.isfinite(rg).all()
    assert rg.float().abs().sum().item() > 0
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(mlp.router.weight.detach().float()).all()
