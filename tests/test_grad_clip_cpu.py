"""Global gradient-norm clipping on CPU: HParams, the fused optimizers' CPU
fallback, ``clip_grads_``, and world-2 gloo gangs of every technique against
a dense single-process clipped run."""

import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from saturn_amd import HParams, Strategy, Task
from saturn_amd.executors.ddp import (
    DDPExecutor,
    _make_optimizer,
    grad_clip_stats,
    make_norm_reduce,
)
from saturn_amd.executors.launch import gang_spawn
from saturn_amd.models import get_mlp_dataloader, get_mlp_model, mse_loss
from saturn_amd.ops.clip import clip_grads_
from saturn_amd.ops.optim import FusedAdam, FusedSGD

# ---------------------------------------------------------------- interface


def test_hparams_max_grad_norm():
    hp = HParams(lr=1e-3, batch_count=2, max_grad_norm=1.0)
    assert hp.max_grad_norm == 1.0
    assert hp.kwargs == {}
    assert hp.as_dict()["max_grad_norm"] == 1.0
    assert "max_grad_norm=1.0" in repr(hp)
    plain = HParams(lr=1e-3, batch_count=2)
    assert plain.max_grad_norm is None
    assert plain.as_dict()["max_grad_norm"] is None
    assert "max_grad_norm" not in repr(plain)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            HParams(lr=1e-3, batch_count=2, max_grad_norm=bad)


@pytest.mark.parametrize("cls", [FusedSGD, FusedAdam])
def test_optimizer_rejects_bad_max_grad_norm(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            cls(p, lr=0.1, max_grad_norm=bad)
    with pytest.raises(ValueError):
        clip_grads_(p, 0.0)
    # without max_grad_norm there is nothing to configure
    with pytest.raises(ValueError):
        cls(p, lr=0.1).set_norm_reduce(lambda s: s)


# ------------------------------------------------------- optimizer numerics

SHAPES = [(33, 17), (64,), (5, 7, 3), (1,)]
STEPS = 3
MAX_NORM = 0.5


def _problem(seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g) for s in SHAPES]
    grads = [
        [torch.randn(s, generator=g) * (1.0 + k) for s in SHAPES]
        for k in range(STEPS)
    ]
    return params, grads


def _clip64(grads64):
    norm = math.sqrt(sum(float((g * g).sum()) for g in grads64))
    coef = min(1.0, MAX_NORM / (norm + 1e-6))
    return [g * coef for g in grads64], coef


def _sgd64(params, grads, lr, mom, wd):
    p = [x.double() for x in params]
    buf = [torch.zeros_like(x) for x in p]
    coefs = []
    for k in range(STEPS):
        gs, c = _clip64([g.double() for g in grads[k]])
        coefs.append(c)
        for i in range(len(p)):
            g = gs[i] + wd * p[i]
            buf[i] = mom * buf[i] + g
            p[i] = p[i] - lr * buf[i]
    return p, coefs


def _adamw64(params, grads, lr, b1, b2, eps, wd):
    p = [x.double() for x in params]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    for k in range(STEPS):
        gs, _ = _clip64([g.double() for g in grads[k]])
        t = k + 1
        for i in range(len(p)):
            m[i] = b1 * m[i] + (1 - b1) * gs[i]
            v[i] = b2 * v[i] + (1 - b2) * gs[i] * gs[i]
            upd = (m[i] / (1 - b1**t)) / ((v[i] / (1 - b2**t)).sqrt() + eps)
            p[i] = p[i] * (1 - lr * wd) - lr * upd
    return p


def _run(opt_factory, params, grads, torch_clip):
    ps = [torch.nn.Parameter(x.clone()) for x in params]
    opt = opt_factory(ps)
    for k in range(STEPS):
        for p, g in zip(ps, grads[k]):
            p.grad = g.clone()
        if torch_clip:
            torch.nn.utils.clip_grad_norm_(ps, MAX_NORM)
        opt.step()
    return [p.detach() for p in ps], opt


def _max_err(ps, ref64):
    return max(float((p.double() - r).abs().max()) for p, r in zip(ps, ref64))


def _ulp32(ref64):
    top = max(float(r.abs().max()) for r in ref64)
    return float(np.spacing(np.float32(top)))


def test_fused_sgd_clipped_matches_fp64():
    params, grads = _problem()
    lr, mom, wd = 0.1, 0.9, 0.01
    ref, coefs = _sgd64(params, grads, lr, mom, wd)
    assert all(c < 1.0 for c in coefs), coefs  # clipping is active
    ours, opt = _run(
        lambda ps: FusedSGD(ps, lr=lr, momentum=mom, weight_decay=wd,
                            max_grad_norm=MAX_NORM),
        params, grads, False,
    )
    theirs, _ = _run(
        lambda ps: torch.optim.SGD(ps, lr=lr, momentum=mom, weight_decay=wd),
        params, grads, True,
    )
    e_ours, e_torch = _max_err(ours, ref), _max_err(theirs, ref)
    print(f"sgd: ours {e_ours:.3e} torch {e_torch:.3e} ulp {_ulp32(ref):.3e}")
    assert e_ours <= 4 * e_torch + _ulp32(ref)
    assert float(opt.skipped_steps) == 0.0


def test_fused_adam_clipped_matches_fp64():
    params, grads = _problem(1)
    lr, betas, eps, wd = 1e-2, (0.9, 0.999), 1e-8, 0.01
    ref = _adamw64(params, grads, lr, betas[0], betas[1], eps, wd)
    ours, _ = _run(
        lambda ps: FusedAdam(ps, lr=lr, betas=betas, eps=eps, weight_decay=wd,
                             max_grad_norm=MAX_NORM),
        params, grads, False,
    )
    theirs, _ = _run(
        lambda ps: torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps,
                                     weight_decay=wd),
        params, grads, True,
    )
    e_ours, e_torch = _max_err(ours, ref), _max_err(theirs, ref)
    print(f"adam: ours {e_ours:.3e} torch {e_torch:.3e} ulp {_ulp32(ref):.3e}")
    assert e_ours <= 4 * e_torch + _ulp32(ref)


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_far_above_norm_equals_unclipped(kind):
    params, grads = _problem(2)

    def make(max_grad_norm):
        if kind == "sgd":
            return lambda ps: FusedSGD(ps, lr=0.1, momentum=0.9,
                                       weight_decay=0.01,
                                       max_grad_norm=max_grad_norm)
        return lambda ps: FusedAdam(ps, lr=1e-2, weight_decay=0.01,
                                    max_grad_norm=max_grad_norm)

    clipped, opt = _run(make(1e30), params, grads, False)
    plain, _ = _run(make(None), params, grads, False)
    for a, b in zip(clipped, plain):
        assert torch.equal(a, b)
    assert float(opt.last_grad_norm) > 0.0


# ------------------------------------------------------ non-finite gradients


def _state_snapshot(opt, ps):
    snap = [p.detach().clone() for p in ps]
    for p in ps:
        for k, v in opt.state[p].items():
            if torch.is_tensor(v):
                snap.append(v.clone())
    return snap


@pytest.mark.parametrize("kind", ["sgd", "adam"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step(kind, bad):
    params, grads = _problem(3)
    # bf16 parameters with fp32 masters: the fallback keeps masters on CPU too
    ps = [torch.nn.Parameter(x.to(torch.bfloat16)) for x in params]
    if kind == "sgd":
        opt = FusedSGD(ps, lr=0.1, momentum=0.9, master_weights=True,
                       max_grad_norm=MAX_NORM)
    else:
        opt = FusedAdam(ps, lr=1e-2, master_weights=True,
                        max_grad_norm=MAX_NORM)

    def step(k, poison):
        for p, g in zip(ps, grads[k]):
            p.grad = g.to(torch.bfloat16)
        if poison:
            ps[1].grad[5] = bad
        opt.step()

    step(0, False)  # creates momentum / moments / masters
    before = _state_snapshot(opt, ps)
    step(1, True)
    after = _state_snapshot(opt, ps)
    assert len(before) == len(after) and len(before) > len(ps)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    assert float(opt.skipped_steps) == 1.0
    assert not math.isfinite(float(opt.last_grad_norm))
    step(2, False)  # the next finite step updates again
    moved = _state_snapshot(opt, ps)
    # (a bf16 parameter may round back to itself; its fp32 master cannot)
    n = len(ps)
    assert all(not torch.equal(a, b) for a, b in zip(after[n:], moved[n:]))
    assert float(opt.skipped_steps) == 1.0
    assert math.isfinite(float(opt.last_grad_norm))


def test_clip_grads_scales_and_zeroes():
    params, grads = _problem(4)
    ps = [torch.nn.Parameter(x.clone()) for x in params]
    for p, g in zip(ps, grads[0]):
        p.grad = g.clone()
    want, coef = _clip64([g.double() for g in grads[0]])
    assert coef < 1.0
    norm = clip_grads_(ps, MAX_NORM)
    assert abs(float(norm) - MAX_NORM / coef) < 1e-4 * float(norm)
    for p, w in zip(ps, want):
        assert torch.allclose(p.grad.double(), w, rtol=1e-6, atol=1e-7)
    ps[2].grad[0, 0, 0] = float("inf")
    norm = clip_grads_(ps, MAX_NORM)
    assert not math.isfinite(float(norm))
    for p in ps:
        assert torch.equal(p.grad, torch.zeros_like(p.grad))


# -------------------------------------------- world-2 equivalence, per technique

W2_STEPS = 3
W2_LR = 0.5
W2_MAX_NORM = 0.05

GPTJ_TINY = {"n_layer": 4, "n_embd": 64, "n_head": 2, "vocab_size": 128,
             "n_ctx": 32, "rotary_dim": 8}
MIXTRAL_TINY = {"n_layer": 2, "n_embd": 64, "n_head": 2, "n_kv_head": 1,
                "vocab_size": 128, "n_ctx": 32, "ffn_dim": 96, "n_expert": 4,
                "top_k": 2}


def _w2_batch():
    return torch.randint(0, 128, (4, 32),
                         generator=torch.Generator().manual_seed(23))


def _w2_task():
    # what _make_optimizer reads of a task
    return SimpleNamespace(
        hparams=HParams(lr=W2_LR, batch_count=W2_STEPS,
                        max_grad_norm=W2_MAX_NORM)
    )


def _train(step_fn, optimizer):
    """Three clipped steps; (losses, norms, coefs) as floats."""
    losses, norms, coefs = [], [], []
    for _ in range(W2_STEPS):
        losses.append(step_fn())
        norm, _ = grad_clip_stats(optimizer)
        norms.append(float(norm))
        coefs.append(min(1.0, W2_MAX_NORM / (float(norm) + 1e-6)))
    return losses, norms, coefs


@functools.lru_cache(maxsize=None)
def _dense(model_kind):
    """Single-process clipped run; computed once and shared."""
    if model_kind == "gptj":
        from saturn_amd.models.gptj import get_gptj_model, pretraining_loss

        model, loss_fn = get_gptj_model(GPTJ_TINY), pretraining_loss
    else:
        from saturn_amd.models.mixtral import get_mixtral_model, mixtral_loss

        model, loss_fn = get_mixtral_model(MIXTRAL_TINY), mixtral_loss
    x = _w2_batch()
    opt = _make_optimizer(_w2_task(), model)

    def step():
        loss = loss_fn(model(x), x)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return float(loss.detach())

    losses, norms, coefs = _train(step, opt)
    # the comparison shows nothing unless every step is really clipped
    assert all(c < 1.0 for c in coefs), coefs
    assert float(opt.skipped_steps) == 0.0
    return losses, norms


def _w2_worker(rank, world, technique):
    import torch
    import torch.distributed as dist

    from saturn_amd.executors.launch import (
        destroy_process_group,
        init_process_group,
    )

    init_process_group(rank, world)
    try:
        gx = _w2_batch()
        task = _w2_task()
        if technique == "ep":
            from saturn_amd.models.mixtral import (
                get_mixtral_model,
                mixtral_loss,
            )
            from saturn_amd.parallel.ddp import BucketedDDP
            from saturn_amd.parallel.expert import (
                ep_expert_parameters,
                ep_scale_expert_grads,
                ep_shard_model,
            )

            model = ep_shard_model(get_mixtral_model(MIXTRAL_TINY))
            experts = ep_expert_parameters(model)
            ids = {id(p) for p in experts}
            ddp = BucketedDDP(model, exclude=experts)
            opt = _make_optimizer(
                task, model, norm_reduce=make_norm_reduce(),
                replicated=[p for p in model.parameters() if id(p) not in ids],
            )
            x = gx[rank * 2:(rank + 1) * 2]

            def step():
                loss = mixtral_loss(ddp(x), x)
                loss.backward()
                ddp.grad_sync()
                ep_scale_expert_grads(model)
                opt.step()
                opt.zero_grad(set_to_none=True)
                ddp.zero_grad_buffers()
                # the dense loss is the mean over the global batch
                l = loss.detach().clone()
                dist.all_reduce(l)
                return float(l) / world
        else:
            from saturn_amd.models.gptj import (
                get_gptj_model,
                pretraining_loss,
            )

            model = get_gptj_model(GPTJ_TINY)
            if technique == "ddp":
                from saturn_amd.parallel.ddp import BucketedDDP

                ddp = BucketedDDP(model, bucket_mb=0.05)
                opt = _make_optimizer(task, model)

                def step():
                    loss = pretraining_loss(ddp(gx), gx)
                    loss.backward()
                    ddp.grad_sync()
                    opt.step()
                    ddp.zero_grad_buffers()
                    return float(loss.detach())
            elif technique == "zero3":
                from saturn_amd.parallel.zero3 import Zero3Model

                z3 = Zero3Model(model, prefetch=False)
                holder = torch.nn.Module()
                holder.ps = torch.nn.ParameterList(z3.sharded_parameters())
                opt = _make_optimizer(task, holder,
                                      norm_reduce=make_norm_reduce())

                def step():
                    loss = pretraining_loss(z3(gx), gx)
                    loss.backward()
                    z3.grad_sync()
                    opt.step()
                    z3.zero_grad_shards()
                    return float(loss.detach())
            elif technique == "tp":
                from saturn_amd.parallel.tensor import (
                    tp_replicated_parameters,
                    tp_shard_model,
                )

                model = tp_shard_model(model)
                opt = _make_optimizer(
                    task, model, norm_reduce=make_norm_reduce(),
                    replicated=tp_replicated_parameters(model),
                )

                def step():
                    loss = pretraining_loss(model(gx), gx)
                    loss.backward()
                    opt.step()
                    opt.zero_grad(set_to_none=True)
                    return float(loss.detach())
            else:
                raise ValueError(technique)

        losses, norms, _ = _train(step, opt)
        # every rank's norms, gathered so rank 0 can hand them all back
        mine = torch.tensor(norms, dtype=torch.float64)
        every = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(every, mine)
        skipped = float(grad_clip_stats(opt)[1])
        if rank == 0:
            return losses, [e.tolist() for e in every], skipped
        return None
    finally:
        destroy_process_group()


def _check_against_dense(model_kind, losses, norms_per_rank):
    d_losses, d_norms = _dense(model_kind)
    for a, b in zip(d_losses, losses):
        assert abs(a - b) < 1e-4, (d_losses, losses)
    for rank_norms in norms_per_rank:
        assert len(rank_norms) == W2_STEPS
        for a, b in zip(d_norms, rank_norms):
            assert abs(a - b) <= 1e-4 * a, (d_norms, norms_per_rank)


@pytest.mark.parametrize(
    "technique,tid,model_kind",
    [("ddp", 971, "gptj"), ("zero3", 972, "gptj"), ("tp", 973, "gptj"),
     ("ep", 974, "mixtral")],
)
def test_world2_clipped_matches_dense(technique, tid, model_kind):
    losses, norms, skipped = gang_spawn(_w2_worker, 2, tid, technique,
                                        timeout=300)
    assert len(norms) == 2 and skipped == 0.0
    _check_against_dense(model_kind, losses, norms)


def test_pipeline_two_stages_clipped_matches_dense():
    from saturn_amd.models.gptj import (
        as_sequential,
        get_gptj_model,
        pretraining_loss,
    )
    from saturn_amd.parallel.pipeline import PipelinedModel

    model = get_gptj_model(GPTJ_TINY)
    pipe = PipelinedModel(as_sequential(model), ["cpu", "cpu"], chunks=2)
    opt = _make_optimizer(_w2_task(), pipe)
    gx = _w2_batch()

    def step():
        loss = pretraining_loss(pipe(gx), gx)
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=True)
        return float(loss.detach())

    losses, norms, _ = _train(step, opt)
    _check_against_dense("gptj", losses, [norms])


# ------------------------------------------------------- executor end to end


@pytest.mark.parametrize("optimizer_cls", [None, torch.optim.Adam])
def test_ddp_executor_with_max_grad_norm(save_dir, library_path,
                                         optimizer_cls):
    t = Task(
        get_mlp_model,
        get_mlp_dataloader,
        mse_loss,
        HParams(lr=1e-2, batch_count=4, optimizer_cls=optimizer_cls,
                max_grad_norm=0.1),
        gpu_range=[1, 2],
        name="clip_mlp_" + ("sgd" if optimizer_cls is None else "adam"),
        save_dir=save_dir,
    )
    params, bt = DDPExecutor.search(t, [0, 1], 975)
    assert params is not None and bt > 0
    t.strategies[2] = Strategy(DDPExecutor, 2, params, bt * 4, batch_time=bt)
    t.select_strategy(t.strategies[2])
    DDPExecutor.execute(t, [0, 1], 975, 2)
    assert t.has_ckpt()


def test_make_optimizer_torch_route_clips():
    """A user-given optimizer class clips through the step pre-hook."""
    model = get_mlp_model()
    task = SimpleNamespace(
        hparams=HParams(lr=0.0, batch_count=1, optimizer_cls=torch.optim.SGD,
                        max_grad_norm=1e-3)
    )
    opt = _make_optimizer(task, model)
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    total = math.sqrt(sum(float((p.grad ** 2).sum())
                          for p in model.parameters()))
    assert abs(total - 1e-3) < 1e-6
    norm, skipped = grad_clip_stats(opt)
    assert float(norm) > 1.0 and float(skipped) == 0.0
    assert grad_clip_stats(
        _make_optimizer(SimpleNamespace(hparams=HParams(lr=0.1, batch_count=1)),
                        model)
    ) is None
