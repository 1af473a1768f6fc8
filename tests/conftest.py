import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires an MI355X GPU (run with -m gpu)"
    )


def pytest_collection_modifyitems(config, items):
    """Skip gpu-marked tests automatically when no GPU is present."""
    try:
        import torch

        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        return
    skip = pytest.mark.skip(reason="no GPU in this container")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


@pytest.fixture(scope="session")
def machine_gpu_count():
    """GPUs this machine really has (session scope: read before any test
    hides them)."""
    try:
        import torch

        return torch.cuda.device_count() if torch.cuda.is_available() else 0
    except Exception:
        return 0


@pytest.fixture(autouse=True)
def cpu_path_unless_gpu_marked(request, monkeypatch, machine_gpu_count):
    """Tests without the gpu mark are the CPU suite: gloo gangs of 2-4 ranks,
    fp32 models.  The library picks nccl and one device per rank whenever a
    GPU is visible, so on a machine with fewer GPUs than ranks those tests
    would die at set_device.  Pin them to the CPU path wherever they run:
    child processes see no devices, and this process reports none.  (The
    engine's own launcher overrides HIP_VISIBLE_DEVICES per gang; a test
    that goes through it checks machine_gpu_count instead.)"""
    if "gpu" in request.keywords:
        return
    import torch

    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 0)


@pytest.fixture()
def library_path(tmp_path, monkeypatch):
    d = tmp_path / "udp_lib"
    d.mkdir()
    monkeypatch.setenv("SATURN_LIBRARY_PATH", str(d))
    return str(d)


@pytest.fixture()
def save_dir(tmp_path):
    d = tmp_path / "saved_models"
    d.mkdir()
    return str(d)
