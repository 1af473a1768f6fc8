"""Guard the driver's bench.py contract: the round-end scale run launches
`python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...`
one rank per GPU.  This must work first try on the 8-GPU node, so the
rendezvous + sharding + MAX-over-ranks + single-JSON-line contract is
exercised here on CPU/gloo at world 2."""

import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_torchrun_world2_gloo():
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", "29539",
            "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
            "--layers", "2", "--seq", "32", "--batch", "2",
        ],
        cwd=REPO,
        env=env,
        capture_output=True,
        text=True,
        timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    # exactly one JSON line on stdout, from rank 0
    json_lines = [
        l for l in out.stdout.splitlines() if l.startswith("{")
    ]
    assert len(json_lines) == 1, out.stdout
    d = json.loads(json_lines[0])
    assert d["n_gpus"] == 2
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["metric"] == "samples_per_s" and d["value"] > 0
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 4  # per-GPU batch x world


def test_bench_single_process_defaults():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "0",
         "--layers", "1", "--seq", "32", "--batch", "2"],
        cwd=REPO,
        capture_output=True,
        text=True,
        timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(
        [l for l in out.stdout.splitlines() if l.startswith("{")][0]
    )
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy
    (well under 64 MB), identically from run to run; --full is accepted and
    the result line keeps its fields and honours --steps.  This is the CPU
    path (conftest hides devices from unmarked tests), whose arithmetic is
    order-stable, so equal inputs must give bit-equal dumps."""
    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--layers", "1", "--seq", "32", "--batch", "2",
             "--dump-outputs", str(d)] + extra,
            cwd=REPO,
            capture_output=True,
            text=True,
            timeout=600,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        json_lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(json_lines) == 1, out.stdout
        r = json.loads(json_lines[0])
        assert r["steps"] == 2 and r["ms_per_step"] > 0
        assert r["dtype"] == "fp32"
        # samples/s = per-GPU batch / seconds per timed step
        assert abs(r["value"] - 2 * 1000.0 / r["ms_per_step"]) < 1e-6 * r["value"]
        files = sorted(os.listdir(d))
        assert files == ["logits_sample.npy", "loss.npy", "params_sample.npy"]
        arrays = {f: np.load(d / f) for f in files}
        assert all(a.dtype == np.float32 for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 * 1000 * 1000
        assert all(np.isfinite(a).all() for a in arrays.values())
        assert arrays["loss.npy"].shape == (1,)
        # batch 2 x seq 32 x vocab exceeds the cap: a fixed-size sample
        assert arrays["logits_sample.npy"].shape == (1 << 20,)
        dumps.append(arrays)
    for f in dumps[0]:
        assert np.array_equal(dumps[0][f], dumps[1][f]), f
