"""Engine + forecast + end-to-end orchestration on CPU (gloo).

BASELINE.json config 1: "2-job MLP lr-sweep on CPU/gloo" — the plumbing test
the reference never had.  Exercises: subprocess gangs,
torch.distributed over gloo with world_size 2, the bucketed DDP engine,
dependency-ordered interval execution, checkpoint/resume across intervals,
and the full orchestrate() loop.
"""

import os

import pytest
import torch

from saturn_amd import HParams, Strategy, Task, orchestrate, register, search
from saturn_amd.engine import call_in_subprocess, forecast
from saturn_amd.executors.ddp import DDPExecutor, _ddp_worker
from saturn_amd.executors.launch import gang_spawn
from saturn_amd.models import get_mlp_dataloader, get_mlp_model, mse_loss
from saturn_amd.solver import solve


def make_mlp_task(name, save_dir, lr=1e-2, batch_count=6, gpu_range=None):
    return Task(
        get_mlp_model,
        get_mlp_dataloader,
        mse_loss,
        HParams(lr=lr, batch_count=batch_count),
        gpu_range=gpu_range or [1, 2],
        name=name,
        save_dir=save_dir,
    )


def test_call_in_subprocess_roundtrip():
    assert call_in_subprocess(sorted, [3, 1, 2], timeout=120) == [1, 2, 3]


def test_call_in_subprocess_error_propagates():
    def boom():
        raise ValueError("inner detail 42")

    with pytest.raises(RuntimeError, match="inner detail 42"):
        call_in_subprocess(boom, timeout=120)


def test_gang_spawn_world2():
    def f(rank, world, x):
        return (rank, world, x) if rank == 0 else None

    assert gang_spawn(f, 2, 900, 7, timeout=120) == (0, 2, 7)


def test_ddp_worker_world2_gloo(save_dir):
    """Two gloo ranks train the MLP; rank 0 checkpoints; weights identical
    to a single-process run with the same effective data order is not
    required — just finite loss + ckpt exists."""
    t = make_mlp_task("g2", save_dir, batch_count=4)
    gang_spawn(_ddp_worker, 2, 901, t, 901, 4, {"bucket_mb": 1.0}, False, timeout=300)
    assert t.has_ckpt()
    ck = t.load_checkpoint()
    assert ck["optimizer"] is not None


def test_ddp_search_returns_params(save_dir, library_path):
    t = make_mlp_task("s1", save_dir)
    params, bt = DDPExecutor.search(t, [0], 902)
    assert params is not None and "bucket_mb" in params
    assert 0 < bt < 60


def test_trial_runner_search_fills_strategies(save_dir, library_path):
    register("ddp", DDPExecutor)
    a = make_mlp_task("tr_a", save_dir)
    b = make_mlp_task("tr_b", save_dir, lr=1e-3)
    search([a, b], log_level=False, n_gpus=2, isolate=False)
    for t in (a, b):
        for g in (1, 2):
            assert g in t.strategies
            s = t.strategies[g]
            assert s.feasible, f"cell ({t.name},{g}) should be feasible"
            assert s.batch_time > 0


def test_forecast_quota_and_completion(save_dir):
    t = make_mlp_task("f1", save_dir, batch_count=10)
    t.strategies[1] = Strategy(DDPExecutor, 1, {"bucket_mb": 1}, 10.0, batch_time=1.0)
    plan = solve([t], n_gpus=1, timeout=5)
    t.select_strategy(t.strategies[1])
    relevant, batches, completing = forecast([t], 5.0, plan)
    assert relevant == [t]
    assert batches == [5]
    assert not completing
    assert t.batches_completed == 5
    relevant, batches, completing = forecast([t], 50.0, plan)
    assert batches == [5]
    assert completing == {t}


def test_forecast_slow_task_still_progresses(save_dir):
    # per-batch time longer than the interval: must still run >= 1 batch
    t = make_mlp_task("f2", save_dir, batch_count=3)
    t.strategies[1] = Strategy(DDPExecutor, 1, {"bucket_mb": 1}, 300.0, batch_time=100.0)
    plan = solve([t], n_gpus=1, timeout=5)
    t.select_strategy(t.strategies[1])
    relevant, batches, _ = forecast([t], 10.0, plan)
    assert batches == [1]


def test_orchestrate_end_to_end_cpu(save_dir, library_path):
    """The full loop: register -> search -> orchestrate, 2-job MLP lr sweep
    on a fake 2-GPU node over gloo.  Models must checkpoint and every task
    must complete its batch quota."""
    register("ddp", DDPExecutor)
    tasks = [
        make_mlp_task("sweep_lr_a", save_dir, lr=1e-2, batch_count=6),
        make_mlp_task("sweep_lr_b", save_dir, lr=1e-3, batch_count=6),
    ]
    search(tasks, n_gpus=2, isolate=False)
    # short intervals so multiple solve/execute cycles happen
    max_bt = max(s.batch_time for t in tasks for s in t.strategies.values() if s.batch_time)
    orchestrate(tasks, interval=max_bt * 4, n_gpus=2, solver_timeout=5)
    for t in tasks:
        assert t.remaining_batches == 0
        assert t.has_ckpt()


def test_orchestrate_respects_gpu_range(save_dir, library_path):
    register("ddp", DDPExecutor)
    t = make_mlp_task("one_gpu", save_dir, batch_count=3, gpu_range=[1])
    search([t], n_gpus=2, isolate=False)
    assert t.strategies[1].feasible
    orchestrate([t], interval=1e6, n_gpus=2, solver_timeout=5)
    assert t.remaining_batches == 0


class FlakyExecutor(DDPExecutor):
    """Fails its first execute() call per task (via a marker file), then
    behaves like DDP — exercises elastic retry-from-checkpoint."""

    name = "flaky"

    @staticmethod
    def execute(task, gpus, tid, batch_count):
        marker = os.path.join(task.save_dir, f"{task.name}.failed_once")
        if not os.path.exists(marker):
            with open(marker, "w") as f:
                f.write("x")
            raise RuntimeError("injected interval failure")
        DDPExecutor.execute(task, gpus, tid, batch_count)


def test_orchestrate_retries_failed_task(save_dir, library_path):
    """A task whose launch crashes retries next interval from its ckpt;
    the batch still completes (the reference aborts the whole batch)."""
    register("flaky", FlakyExecutor)
    t = make_mlp_task("flaky_t", save_dir, batch_count=4, gpu_range=[1])
    search([t], executor_names=["flaky"], n_gpus=1, isolate=False)
    assert t.strategies[1].feasible
    orchestrate([t], interval=1e6, n_gpus=1, solver_timeout=5)
    assert t.remaining_batches == 0
    assert t.has_ckpt()


def test_orchestrate_gives_up_after_max_retries(save_dir, library_path):
    class AlwaysFails(DDPExecutor):
        name = "always_fails"

        @staticmethod
        def execute(task, gpus, tid, batch_count):
            raise RuntimeError("boom")

    register("always_fails", AlwaysFails)
    t = make_mlp_task("doomed", save_dir, batch_count=4, gpu_range=[1])
    search([t], executor_names=["always_fails"], n_gpus=1, isolate=False)
    # search also fails -> infeasible; force a strategy so orchestrate runs
    t.strategies[1] = Strategy(AlwaysFails, 1, {"p": 1}, 4.0, batch_time=1.0)
    with pytest.raises(RuntimeError, match="giving up"):
        orchestrate([t], interval=1e6, n_gpus=1, solver_timeout=5,
                    max_task_retries=1)


def test_orchestrate_four_gpu_gang(save_dir, library_path, machine_gpu_count):
    """A 4-process gloo gang through the full pipeline (the driver's scale
    bench runs world 4/8 on hardware; this pins the rendezvous + gang
    binding shape beyond world 2)."""
    if 0 < machine_gpu_count < 4:
        # the engine's launcher hands each gang its devices itself, so on a
        # GPU machine the ranks bind one device each
        pytest.skip(f"needs 4 GPUs (or none), found {machine_gpu_count}")
    from saturn_amd import HParams, Strategy, Task, orchestrate
    from saturn_amd.executors.ddp import DDPExecutor
    from saturn_amd.models import get_mlp_dataloader, get_mlp_model, mse_loss

    t = Task(
        get_mlp_model,
        get_mlp_dataloader,
        mse_loss,
        HParams(lr=1e-2, batch_count=4),
        gpu_range=[4],
        name="gang4",
        save_dir=save_dir,
    )
    t.strategies[4] = Strategy(DDPExecutor, 4, {"bucket_mb": 32.0}, 4.0,
                               batch_time=1.0)
    t.select_strategy(t.strategies[4])
    orchestrate([t], interval=120, n_gpus=4)
    assert t.has_ckpt()


def test_search_profile_attaches_kernel_evidence(save_dir, library_path, monkeypatch):
    """profile=True must attach rocprof kernel rows + rocm-smi samples to
    the fastest feasible Strategy's params (north-star rocprof-fed trials;
    mocked here — the real rocprofv3 path needs a GPU)."""
    import torch

    import saturn_amd.trial_runner.profiler as prof

    register("ddp", DDPExecutor)
    t = make_mlp_task("prof_a", save_dir)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(
        prof, "rocprof_stats",
        lambda cmd, **kw: [
            {"Name": "samd::fused_sgd_kernel", "TotalDurationNs": "1200",
             "Calls": "4"},
            {"Name": "Cijk_gemm", "TotalDurationNs": "900", "Calls": "12"},
        ],
    )
    monkeypatch.setattr(
        prof, "rocm_smi_sample",
        lambda: [{"card": "card0", "VRAM Total Used Memory (B)": "123"}],
    )
    search([t], log_level=False, n_gpus=2, isolate=False, profile=True)
    best = min(
        (s for s in t.strategies.values() if s.feasible),
        key=lambda s: s.batch_time,
    )
    assert "kernels" in best.parameters, best.parameters
    assert best.parameters["kernels"][0]["name"].startswith("samd::")
    assert "rocm_smi" in best.parameters


def test_execute_serializes_shared_gpu_tasks(save_dir, tmp_path):
    """Engine invariant: tasks sharing a GPU must run strictly in plan
    order; disjoint-GPU tasks may overlap.  Verified with a file-logging
    executor (the subprocess boundary is real)."""
    import json
    import time

    from saturn_amd.core.technique import BaseTechnique
    from saturn_amd.engine.gang import execute
    from saturn_amd.solver.milp import Plan

    logf = str(tmp_path / "exec_log.jsonl")

    class Logger(BaseTechnique):
        name = "logger"

        @staticmethod
        def execute(task, gpus, tid, batch_count):
            t0 = time.monotonic()
            time.sleep(0.4)
            with open(logf, "a") as fh:
                fh.write(json.dumps(
                    {"task": task.name, "start": t0,
                     "end": time.monotonic()}) + "\n")

        @staticmethod
        def search(task, gpus, tid):
            return {"x": 1}, 0.1

    tasks = [make_mlp_task(nm, save_dir) for nm in ("ea", "eb", "ec")]
    for t in tasks:
        t.strategies[1] = Strategy(Logger, 1, {"x": 1}, 1.0, batch_time=0.1)
        t.select_strategy(t.strategies[1])
    # ea then eb share GPU 0 (eb depends on ea); ec alone on GPU 1
    plan = Plan(
        task_names=["ea", "eb", "ec"],
        chosen_option=[0, 0, 0],
        gpu_counts=[1, 1, 1],
        gpu_sets=[[0], [0], [1]],
        start_times=[0.0, 1.0, 0.0],
        runtimes=[1.0, 1.0, 1.0],
        makespan=2.0,
    )
    execute(tasks, [1, 1, 1], 2.0, plan)
    rows = {r["task"]: r for r in map(json.loads,
                                      open(logf).read().splitlines())}
    assert set(rows) == {"ea", "eb", "ec"}
    # ea fully precedes eb (shared GPU)
    assert rows["ea"]["end"] <= rows["eb"]["start"] + 1e-3
    # ec overlaps ea (disjoint GPUs, both start at 0): it must NOT have
    # waited for the whole ea+eb chain
    assert rows["ec"]["start"] < rows["eb"]["start"]


def test_forecast_runtime_only_strategy(save_dir):
    """A Strategy without batch_time falls back to runtime/total_batches
    (cells imported from a plan dump may only carry whole-job runtime)."""
    t = make_mlp_task("fr", save_dir, batch_count=10)
    t.strategies[1] = Strategy(DDPExecutor, 1, {"bucket_mb": 1}, 20.0)
    plan = solve([t], n_gpus=1, timeout=5)
    t.select_strategy(t.strategies[1])
    relevant, batches, _ = forecast([t], 10.0, plan)
    # 10 s interval at 2 s/batch -> 5 batches
    assert batches == [5]


def test_execute_dependent_fails_when_dependency_fails(save_dir, tmp_path):
    """A task whose shared-GPU predecessor crashed must fail (not run on a
    half-trained checkpoint) and be reported for elastic retry."""
    from saturn_amd.core.technique import BaseTechnique
    from saturn_amd.engine.gang import execute
    from saturn_amd.solver.milp import Plan

    marker = str(tmp_path / "ran_b.txt")

    class Boom(BaseTechnique):
        name = "boom"

        @staticmethod
        def execute(task, gpus, tid, batch_count):
            if task.name == "da":
                raise RuntimeError("injected failure")
            with open(marker, "w") as fh:
                fh.write("ran")

        @staticmethod
        def search(task, gpus, tid):
            return {"x": 1}, 0.1

    tasks = [make_mlp_task(nm, save_dir) for nm in ("da", "db")]
    for t in tasks:
        t.strategies[1] = Strategy(Boom, 1, {"x": 1}, 1.0, batch_time=0.1)
        t.select_strategy(t.strategies[1])
    plan = Plan(
        task_names=["da", "db"], chosen_option=[0, 0], gpu_counts=[1, 1],
        gpu_sets=[[0], [0]], start_times=[0.0, 1.0], runtimes=[1.0, 1.0],
        makespan=2.0,
    )
    failed = execute(tasks, [1, 1], 2.0, plan, raise_on_failure=False)
    assert {t.name for t in failed} == {"da", "db"}
    import os as _os

    assert not _os.path.exists(marker)  # db never ran


def test_gpu_pool_never_oversubscribes():
    """Trial-runner GPU-slot allocator: concurrent cells must never hold
    overlapping device ids and blocked acquires proceed after release."""
    import threading
    import time

    from saturn_amd.trial_runner.evaluator import _GpuPool

    pool = _GpuPool(4)
    held, errors = [], []
    lock = threading.Lock()

    def worker(g):
        ids = pool.acquire(g)
        with lock:
            for other in held:
                if set(ids) & set(other):
                    errors.append((ids, other))
            held.append(ids)
        time.sleep(0.05)
        with lock:
            held.remove(ids)
        pool.release(ids)

    threads = [threading.Thread(target=worker, args=(g,))
               for g in (2, 2, 1, 3, 4, 1, 2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert pool.free == set(range(4))
