"""FSDP/ZeRO-3 executor on the framework's own shard manager.

Capability parity with the reference FSDP example UDP
(``examples/wikitext103/executors/FSDP.py:57-245``): per-block shard units,
{activation-checkpoint x cpu-offload} first-fit autotune (FSDP.py:72-98 —
the first configuration that does not OOM wins), full-state-dict
checkpointing to rank 0.  The sharding itself is
``saturn_amd.parallel.zero3`` (RCCL all-gather / reduce-scatter per block
with one-block-ahead prefetch) instead of torch FSDP.
"""

from __future__ import annotations

from timeit import default_timer as timer
from typing import Any, Dict, List, Optional, Tuple

from saturn_amd.core.technique import BaseTechnique
from saturn_amd.executors.launch import (
    destroy_process_group,
    gang_spawn,
    init_process_group,
)

TRIAL_BATCHES = 3


def _fsdp_worker(
    rank: int,
    world: int,
    task,
    tid: int,
    batch_count: int,
    params: Optional[Dict[str, Any]],
    trial: bool,
):
    import torch

    from saturn_amd.executors.ddp import _make_optimizer, make_norm_reduce
    from saturn_amd.parallel.zero3 import Zero3Model

    params = params or {}
    backend = init_process_group(rank, world)
    try:
        device = (
            torch.device("cuda", rank) if backend == "nccl" else torch.device("cpu")
        )
        dtype = torch.bfloat16 if backend == "nccl" else torch.float32

        from saturn_amd.executors.ddp import build_model_on

        model = build_model_on(task, device, dtype)
        model.train()
        z3 = Zero3Model(
            model,
            device=device,
            offload=bool(params.get("offload", False)),
            checkpoint_activations=bool(params.get("checkpoint", False)),
        )

        import torch.nn as nn

        class _ShardHolder(nn.Module):
            def __init__(self, shards):
                super().__init__()
                self.ps = nn.ParameterList(shards)

        holder = _ShardHolder(z3.sharded_parameters())
        if task.hparams.max_grad_norm is None:
            optimizer = _make_optimizer(task, holder)
        else:
            # every parameter is a shard: the global norm is the all-reduced
            # squared sum
            optimizer = _make_optimizer(
                task, holder, norm_reduce=make_norm_reduce()
            )

        # Sharded optimizer-state resume (the reference loses optimizer
        # moments at every interval; full-state ckpts carry
        # them for DDP — here each rank reloads its own shard state when
        # the solver kept the same world size, the common case under plan
        # hysteresis).
        import os as _os

        opt_path = _os.path.join(
            task.save_dir, f"{task.name}.optshard.w{world}.r{rank}.pt"
        )
        if not trial and _os.path.isfile(opt_path):
            try:
                optimizer.load_state_dict(
                    torch.load(opt_path, map_location="cpu", weights_only=False)
                )
            except Exception:
                pass  # layout changed; fresh moments

        it = task.get_iterator() if not trial else task.get_fresh_iterator()

        def next_batch():
            nonlocal it
            try:
                return next(it)
            except StopIteration:
                it = task.get_fresh_iterator()
                return next(it)

        def step(batch):
            x, y = batch
            # ZeRO-3 is still data parallelism: shard the global batch
            # across ranks (same slicing as the DDP executor) so per-step
            # time actually drops with more GPUs; the reduce-scatter
            # averages the shard gradients.  Round 1 fed every rank the
            # full batch — memory savings but zero DP speedup.
            n = x.shape[0]
            if world > 1 and n >= world:
                lo = rank * n // world
                hi = (rank + 1) * n // world
                x, y = x[lo:hi], y[lo:hi]
            x = x.to(device, non_blocking=True)
            y = y.to(device, non_blocking=True)
            if x.is_floating_point():
                x = x.to(dtype)
            loss = task.loss_function(z3(x), y)
            loss.backward()
            z3.grad_sync()
            optimizer.step()
            z3.zero_grad_shards()

        result = None
        if trial:
            step(next_batch())
            if device.type == "cuda":
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
            t0 = timer()
            for _ in range(TRIAL_BATCHES - 1):
                step(next_batch())
            if device.type == "cuda":
                torch.cuda.synchronize()
            hbm = (
                torch.cuda.max_memory_allocated() / 2**30
                if device.type == "cuda"
                else 0.0
            )
            result = ((timer() - t0) / (TRIAL_BATCHES - 1), hbm)
        else:
            for _ in range(batch_count):
                step(next_batch())
            if device.type == "cuda":
                torch.cuda.synchronize()
            sd = z3.full_state_dict()
            if rank == 0 and sd is not None:
                task.save_checkpoint(sd, None)
            # every rank persists its optimizer shard state (skipped
            # when the engine marked this task completing — see Task)
            if _os.environ.get("SATURN_SKIP_CKPT") != "1":
                tmp = opt_path + ".tmp"
                torch.save(optimizer.state_dict(), tmp)
                _os.replace(tmp, opt_path)
            import torch.distributed as dist

            if world > 1:
                dist.barrier()
        return result
    finally:
        destroy_process_group()


class FSDPExecutor(BaseTechnique):
    """ZeRO-3 sharded data parallelism."""

    name = "fsdp"

    #: first-fit order, cheapest memory footprint last (reference
    #: FSDP.py:72-78 walks the same grid)
    GRID = [
        {"checkpoint": False, "offload": False},
        {"checkpoint": True, "offload": False},
        {"checkpoint": True, "offload": True},
    ]

    @staticmethod
    def execute(task, gpus: List[int], tid: int, batch_count: int) -> None:
        params = (
            task.selected_strategy.parameters
            if task.selected_strategy is not None
            else {}
        )
        gang_spawn(
            _fsdp_worker, len(gpus), tid, task, tid, batch_count, params, False
        )

    @staticmethod
    def search(
        task, gpus: List[int], tid: int
    ) -> Tuple[Optional[Dict[str, Any]], float]:
        world = len(gpus)
        for cfg in FSDPExecutor.GRID:
            try:
                out = gang_spawn(
                    _fsdp_worker, world, tid, task, tid, TRIAL_BATCHES, cfg, True
                )
            except Exception:
                continue
            if out is not None:
                bt, hbm = out
                return dict(cfg, hbm_peak_gb=round(hbm, 2)), bt
        return None, float("inf")
