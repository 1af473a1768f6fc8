"""Global gradient-norm clipping on the GPU: the grad_sqsum reduction, the
clip coefficient, and the fused optimizer kernels' grad_scale path."""

import copy
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def partials_for(n_tensors):
    return torch.empty(ext().grad_sqsum_slots(n_tensors), dtype=torch.float32,
                       device="cuda")


def sqsum(tensors):
    return ext().grad_sqsum(list(tensors), partials_for(len(tensors)))


def grid_cap():
    # the launch rule caps the grid; a huge tensor shows the cap
    return ext().grad_sqsum_plan([1 << 40])[0][0]


def chain_length(numels):
    """Elements one thread accumulates serially, from the launcher's plan."""
    plan = ext().grad_sqsum_plan(list(numels))
    longest = 0
    for li, (blocks, threads) in enumerate(plan):
        groups = sum((n + 7) // 8 for n in numels[li * 32:(li + 1) * 32])
        trips = -(-groups // (blocks * threads))
        longest = max(longest, trips * 8)
    return longest


def check_sqsum(tensors):
    got = float(sqsum(tensors))
    want = sum(float(t.double().pow(2).sum()) for t in tensors)
    bound = (chain_length([t.numel() for t in tensors]) + 64) * 2.0 ** -24
    err = abs(got - want) / want if want else abs(got)
    print(f"sqsum n={len(tensors)} got {got!r} want {want!r} "
          f"rel {err:.3e} bound {bound:.3e}")
    assert err <= bound


def randn(n, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(n, device="cuda", generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def large(dtype):
    # cap * 256 threads * 8 elements + 5: the grid-stride loop runs twice
    return randn(grid_cap() * 256 * 8 + 5, dtype, 1)


# ------------------------------------------------------------- grad_sqsum


@pytest.mark.parametrize("dtype", DTYPES)
def test_sqsum_small_sizes(dtype):
    # tail only, one group, group + tail, many groups
    for i, n in enumerate((1, 7, 8, 43, 4096)):
        check_sqsum([randn(n, dtype, 10 + i)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_sqsum_with_empty_tensor(dtype):
    ts = [randn(43, dtype, 2), torch.empty(0, dtype=dtype, device="cuda"),
          randn(9, dtype, 3)]
    check_sqsum(ts)
    assert float(sqsum([ts[1]])) == 0.0
    assert float(sqsum(ts)) == float(sqsum([ts[0], ts[2]]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("count", [33, 65])
def test_sqsum_many_tensors(dtype, count):
    # more than 32 tensors: a second (33) and a third (65) launch
    sizes = [1, 7, 8, 43, 100, 257, 1024, 3]
    ts = [randn(sizes[i % len(sizes)] + i, dtype, 100 + i)
          for i in range(count)]
    assert len(ext().grad_sqsum_plan([t.numel() for t in ts])) == -(-count // 32)
    check_sqsum(ts)


@pytest.mark.parametrize("dtype", DTYPES)
def test_sqsum_grid_stride(dtype):
    t = large(dtype)
    assert chain_length([t.numel()]) == 16
    check_sqsum([t])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("offset", [3, 4])
def test_sqsum_unaligned_view_equals_aligned_clone(dtype, offset):
    flat = randn(offset + 4096 + 43, dtype, 5)
    view = flat[offset:]
    # (4 fp32 elements are 16 B: that view is aligned, the others are not)
    assert (view.data_ptr() % 16 != 0) == (offset * flat.element_size() % 16 != 0)
    clone = view.clone()
    assert clone.data_ptr() % 16 == 0
    a, b = sqsum([view]), sqsum([clone])
    assert torch.equal(a, b), (float(a), float(b))
    check_sqsum([view])


def test_sqsum_is_deterministic():
    t = large(torch.bfloat16)
    a, b = sqsum([t]), sqsum([t])
    assert torch.equal(a, b)


def test_clip_coef_formula_and_flag():
    out = torch.zeros(3, device="cuda")
    sq = torch.tensor([16.0], device="cuda")
    ext().clip_coef(sq, 2.0, out)
    norm, coef, skipped = out.tolist()
    assert norm == 4.0 and skipped == 0.0
    assert abs(coef - 2.0 / (4.0 + 1e-6)) < 1e-7
    ext().clip_coef(sq, 100.0, out)
    assert out[1].item() == 1.0
    for bad in (float("inf"), float("nan")):
        ext().clip_coef(torch.tensor([bad], device="cuda"), 2.0, out)
        assert not math.isfinite(out[0].item()) and out[1].item() == 0.0
    assert out[2].item() == 2.0
    ext().clip_coef(sq, 2.0, out)  # a finite norm clears the flag
    assert out[0].item() == 4.0 and out[2].item() == 2.0


# ------------------------------------------------------ clipped optimizers

# the shapes of test_fused_sgd_matches_reference plus one with a tail
SHAPES = [(128, 64), (1000,), (33, 7), (4096,), (43,)]
STEPS = 3
MAX_NORM = 50.0


@functools.lru_cache(maxsize=None)
def problem():
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=g).to(torch.bfloat16) for s in SHAPES]
    grads = [[torch.randn(s, generator=g).to(torch.bfloat16) for s in SHAPES]
             for _ in range(STEPS)]
    return params, grads


def make_opt(kind, ps, momentum, master, max_grad_norm):
    from saturn_amd.ops.optim import FusedAdam, FusedSGD

    if kind == "sgd":
        return FusedSGD(ps, lr=0.1, momentum=momentum, weight_decay=0.01,
                        master_weights=master, max_grad_norm=max_grad_norm)
    return FusedAdam(ps, lr=1e-2, weight_decay=0.01, master_weights=master,
                     max_grad_norm=max_grad_norm)


def run(kind, device, momentum, master, max_grad_norm, poison=None):
    """STEPS steps from the shared problem; (params, optimizer)."""
    params, grads = problem()
    # clone: on the CPU .to() would alias the shared problem's tensors
    ps = [torch.nn.Parameter(p.clone().to(device)) for p in params]
    opt = make_opt(kind, ps, momentum, master, max_grad_norm)
    for k in range(STEPS):
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(device)
        if poison is not None and k == poison[0]:
            ps[1].grad[5] = poison[1]
        opt.step()
    return ps, opt


def state_of(opt, ps):
    out = [p.detach().float().cpu() for p in ps]
    for p in ps:
        for v in opt.state[p].values():
            if torch.is_tensor(v):
                out.append(v.float().cpu())
    return out


def max_diff(a, b):
    return max(float((x.detach().float().cpu() - y.detach().float().cpu())
                     .abs().max()) for x, y in zip(a, b))


def bf16_ulp(ps):
    top = max(float(p.detach().float().abs().max()) for p in ps)
    return 2.0 ** (math.floor(math.log2(top)) - 7)


CASES = [("sgd", 0.0, False), ("sgd", 0.9, False), ("sgd", 0.0, True),
         ("sgd", 0.9, True), ("adam", 0.0, False), ("adam", 0.0, True)]


@pytest.mark.parametrize("kind,momentum,master", CASES)
def test_clipped_steps_match_cpu_fallback(kind, momentum, master):
    gpu_c, opt = run(kind, "cuda", momentum, master, MAX_NORM)
    cpu_c, _ = run(kind, "cpu", momentum, master, MAX_NORM)
    gpu_u, _ = run(kind, "cuda", momentum, master, None)
    cpu_u, _ = run(kind, "cpu", momentum, master, None)
    # randn gradients of ~13.5k elements: every step's norm is above 100
    assert float(opt.last_grad_norm) > MAX_NORM
    assert float(opt.skipped_steps) == 0.0
    e_clip, e_plain = max_diff(gpu_c, cpu_c), max_diff(gpu_u, cpu_u)
    tol = 4 * e_plain + bf16_ulp(cpu_c)
    print(f"{kind} mom={momentum} master={master}: clipped {e_clip:.3e} "
          f"unclipped {e_plain:.3e} tol {tol:.3e}")
    assert e_clip <= tol


@pytest.mark.parametrize("kind,momentum,master",
                         [("sgd", 0.9, True), ("sgd", 0.0, False),
                          ("adam", 0.0, True), ("adam", 0.0, False)])
def test_coef_one_is_bit_identical_to_unclipped(kind, momentum, master):
    a, oa = run(kind, "cuda", momentum, master, 1e30)
    b, ob = run(kind, "cuda", momentum, master, None)
    sa, sb = state_of(oa, a), state_of(ob, b)
    assert len(sa) == len(sb)
    for x, y in zip(sa, sb):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_clipped_step_is_deterministic(kind):
    a, oa = run(kind, "cuda", 0.9, True, MAX_NORM)
    b, ob = run(kind, "cuda", 0.9, True, MAX_NORM)
    for x, y in zip(state_of(oa, a), state_of(ob, b)):
        assert torch.equal(x, y)
    assert torch.equal(oa.last_grad_norm, ob.last_grad_norm)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step(kind, bad):
    params, grads = problem()
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    opt = make_opt(kind, ps, 0.9, True, MAX_NORM)

    def step(k, poison):
        for p, g in zip(ps, grads[k]):
            p.grad = g.cuda()
        if poison:
            ps[1].grad[5] = bad
        opt.step()

    step(0, False)
    before = state_of(opt, ps)
    step(1, True)
    after = state_of(opt, ps)
    assert len(after) == len(before) > len(ps)
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    assert float(opt.skipped_steps) == 1.0
    assert not math.isfinite(float(opt.last_grad_norm))
    step(2, False)
    moved = state_of(opt, ps)
    n = len(ps)  # masters, momentum and moments all move on a finite step
    assert all(not torch.equal(x, y) for x, y in zip(after[n:], moved[n:]))
    assert float(opt.skipped_steps) == 1.0
    assert math.isfinite(float(opt.last_grad_norm))


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_norm_and_skip_counter_live_on_the_device(kind):
    ps, opt = run(kind, "cuda", 0.0, False, MAX_NORM)
    assert opt.last_grad_norm.is_cuda and opt.skipped_steps.is_cuda
    want = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
    assert abs(float(opt.last_grad_norm) - want) <= 1e-5 * want


def test_clip_grads_on_device():
    from saturn_amd.ops.clip import clip_grads_

    params, grads = problem()
    ps = [torch.nn.Parameter(p.cuda()) for p in params]
    for p, g in zip(ps, grads[0]):
        p.grad = g.cuda()
    want = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
    norm = clip_grads_(ps, MAX_NORM)
    assert norm.is_cuda and abs(float(norm) - want) <= 1e-5 * want
    after = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
    assert abs(after - MAX_NORM) < 1e-2 * MAX_NORM  # bf16 gradients
    ps[1].grad[5] = float("inf")
    clip_grads_(ps, MAX_NORM)
    assert all(float(p.grad.float().abs().max()) == 0.0 for p in ps)


# ------------------------------------------------------------------ hipGraph


def test_hipgraph_clipped_step_matches_eager():
    """Scheme of test_hipgraph_step_matches_eager with clipping active: the
    step never synchronises, and the coefficient is recomputed at every
    replay rather than baked in at capture."""
    from saturn_amd.models.gptj import get_gptj_model, pretraining_loss
    from saturn_amd.ops.optim import FusedSGD
    from saturn_amd.utils.graph_step import graphed_train_step

    torch.manual_seed(0)
    cfg = {"n_layer": 2, "n_embd": 256, "n_head": 4, "vocab_size": 512,
           "n_ctx": 64, "rotary_dim": 16}
    max_norm = 0.25
    m1 = get_gptj_model(cfg).to("cuda", torch.bfloat16)
    m2 = copy.deepcopy(m1)
    o1 = FusedSGD(m1.parameters(), lr=1e-3, max_grad_norm=max_norm)
    o2 = FusedSGD(m2.parameters(), lr=1e-3, max_grad_norm=max_norm)

    g = torch.Generator().manual_seed(9)
    batches = [torch.randint(0, 512, (2, 64), generator=g).cuda()
               for _ in range(3)]

    eager_losses, eager_norms = [], []
    for b in batches:
        o1.zero_grad(set_to_none=False)
        loss = pretraining_loss(m1(b), b)
        loss.backward()
        o1.step()
        eager_losses.append(float(loss))
        eager_norms.append(float(o1.last_grad_norm))
    assert all(n > max_norm for n in eager_norms), eager_norms
    assert len(set(eager_norms)) == 3  # a baked-in norm could not follow

    m3 = copy.deepcopy(m2)  # pristine values; warm-up mutates m2
    graphed, static_x = graphed_train_step(
        m2, pretraining_loss, o2, batches[0], warmup=2
    )
    with torch.no_grad():
        for p2, p3 in zip(m2.parameters(), m3.parameters()):
            p2.copy_(p3)
    graph_losses, graph_norms = [], []
    for b in batches:
        static_x.copy_(b)
        graph_losses.append(float(graphed.replay()))
        graph_norms.append(float(o2.last_grad_norm))

    assert eager_losses == graph_losses, (eager_losses, graph_losses)
    assert eager_norms == graph_norms, (eager_norms, graph_norms)
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        assert torch.equal(p1, p2)
    assert float(o2.skipped_steps) == 0.0
