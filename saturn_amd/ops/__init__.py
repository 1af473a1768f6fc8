"""saturn_amd.ops: hand-written CDNA4 HIP kernels + their Python wrappers.

The compiled extension (``saturn_amd/_C*.so``, built in-tree by
``setup.py build_ext --inplace`` / ``__graft_entry__.build()`` for gfx950)
provides the hot-path kernels (SURVEY §2.4 K1-K12 worklist): fused
multi-tensor SGD/Adam (K9), LayerNorm/RMSNorm fwd+bwd (K4), fused
shift-cross-entropy (K8), RoPE (K3), flash attention (K2).

Policy: on a GPU box these ops REQUIRE the extension — a silent eager
fallback would invalidate every measurement — while on CPU (the test
container has no GPU) pure-PyTorch reference paths keep the suite runnable.
"""

from __future__ import annotations

import importlib
from typing import Optional

_ext = None
_ext_err: Optional[str] = None


def _load():
    global _ext, _ext_err
    if _ext is not None or _ext_err is not None:
        return _ext
    try:
        _ext = importlib.import_module("saturn_amd._C")
    except Exception as e:  # noqa: BLE001
        _ext_err = f"{type(e).__name__}: {e}"
        _ext = None
    return _ext


def has_ext() -> bool:
    return _load() is not None


def require_ext():
    """Return the extension, or raise loudly — called from every GPU path."""
    ext = _load()
    if ext is None:
        raise RuntimeError(
            "saturn_amd._C (HIP/gfx950 extension) is not built but a GPU "
            "path needs it. Run `python setup.py build_ext --inplace` "
            f"(import error: {_ext_err})"
        )
    return ext


# MoE routing / dispatch ops (K13); imported last: ops.moe needs require_ext
from saturn_amd.ops.moe import (  # noqa: E402
    moe_combine,
    moe_permute,
    moe_route,
    moe_sort,
)

__all__ = [
    "has_ext",
    "require_ext",
    "moe_route",
    "moe_sort",
    "moe_permute",
    "moe_combine",
]
