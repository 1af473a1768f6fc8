"""Attention conformance suite (attention.hip through saturn_amd.ops.flash).

Every dispatch path, mask edge and layout of attn_fwd / attn_bwd against the
fp64 reference of tests/attn_ref.py under its `close` criterion (tolerance
measured on the bf16 reference composition, never on the kernel), the LSE
criterion, exact bitwise properties, analytic q = 0 results and one child
process per environment switch.  Shapes are the smallest that reach the code
in question: B*H <= 15, T <= 512.

Each comparison prints an ``ATTN_RATIO <group> <case> <json>`` line (kernel
error over the error floor, per tensor); docs/kernels.md tabulates the worst
of them.
"""

import json
import math
import os
import re
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402  (plain helper module beside this file)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DS = [64, 128, 256]


def _ext():
    from saturn_amd.ops import require_ext

    return require_ext()


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and \
        torch.equal(_bits(a), _bits(b))


def _default_paths(T, D):
    """What attn_dispatch must report for (padded T, D) with no switch set:
    the dispatch rule restated from the shape, so that a change to the rule
    in attention.hip fails here."""
    fwd = "attn_fwd_v2_kernel" if (T % 128 == 0 and D <= 128) else "attn_fwd_kernel"
    tr = 1 if D <= 128 else 0
    return (f"{fwd}<{D}> attn_delta_kernel<{D}> "
            f"attn_bwd_kernel<{D},{tr},0> attn_dq_kernel<{D},{tr},0>")


def _check(group, case, got, q, k, v, causal, do, skip=(), every_head=True):
    """every_head: the LSE tolerance must lie below the one-key shift on
    every (b, h), so a mask fault confined to one head is seen too; only the
    peaky inputs (edge key ~1e-6 of a row on some heads) settle for one."""
    rep, bad = ar.check_case(got, q, k, v, causal, do, every_head=every_head)
    print("ATTN_RATIO", group, case, json.dumps(ar.ratios(rep)),
          "lse", json.dumps(rep.get("lse")))
    bad = [b for b in bad if b.split(":")[0] not in skip]
    assert not bad, bad
    return rep


def _both(q, k, v, causal, do, gqa=False):
    """Public wrapper for out and the gradients (shape and leaf plumbing),
    direct calls for LSE; the two routes must agree bit for bit, except for
    dk/dv under GQA, which are summed with fp32 atomics in arrival order."""
    out, dq, dk, dv = ar.kernel_public(q, k, v, causal, do)
    assert out.shape == q.shape and dq.shape == q.shape
    assert dk.shape == k.shape and dv.shape == v.shape
    d = ar.kernel_direct(q, k, v, causal, do)
    assert _same(out, d[0]) and _same(dq, d[2])
    if not gqa:
        assert _same(dk, d[3]) and _same(dv, d[4])
    return out, d[1], dq, dk, dv


# ---------------------------------------------------------------------------
# A. path matrix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["randn", "peaky"])
@pytest.mark.parametrize("B,H", [(1, 3), (3, 5)])   # odd B*H: bh is the
#                                                     fastest grid dimension
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T,path", [
    (64, "v1"), (192, "v1"), (320, "v1"),            # T % 128 != 0
    (128, "v2"), (384, "v2"), (512, "v2"),           # T % 128 == 0, D <= 128
])
@pytest.mark.parametrize("D", DS)
def test_path_matrix(D, T, path, causal, B, H, kind):
    if D == 256:
        path = "v1"                                  # v2 stops at D = 128
    want = _default_paths(T, D)
    assert want.startswith("attn_fwd_v2_kernel" if path == "v2"
                           else "attn_fwd_kernel<")
    assert _ext().attn_dispatch(T, D) == want
    q, k, v, do = ar.make_inputs(kind, B, H, H, T, D, DEV, seed=1)
    got = ar.kernel_direct(q, k, v, causal, do)
    _check("A", f"D{D}T{T}{'c' if causal else 'n'}B{B}H{H}{kind}",
           got, q, k, v, causal, do, every_head=(kind != "peaky"))


# ---------------------------------------------------------------------------
# B. ragged T through the public wrapper
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [1, 63, 65, 130, 197, 257])
@pytest.mark.parametrize("D", DS)
def test_ragged_T(D, T, causal):
    """130 -> 192 and 257 -> 320 are the v1 forward with kv_len < T."""
    B, H = 2, 3
    assert _ext().attn_dispatch(ar.padded_t(T), D) == _default_paths(ar.padded_t(T), D)
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=2)
    got = _both(q, k, v, causal, do)
    if T > 1:
        _check("B", f"D{D}T{T}{'c' if causal else 'n'}", got, q, k, v, causal, do)
        return
    # T = 1, the one named exception to `close` (docs/kernels.md): softmax
    # over a single key is constant, so dq and dk are exactly 0 and the
    # floor's error can be 0 too.  What the kernel returns is the fp32
    # difference of two D-term sums of the same products do_i * v_i taken in
    # different orders (the dP MFMA and the delta kernel), each within
    # D * 2^-24 * sum|do_i v_i| of the true sum, times scale and one k (q)
    # element, rounded to bf16 twice (2 %).
    _check("B", f"D{D}T1", got, q, k, v, causal, do, skip=("dq", "dk"))
    ds = (2 * D * 2.0 ** -24 / math.sqrt(D)
          * (do.double() * v.double()).abs().sum(-1).max().item())
    assert got[2].abs().max().item() <= 1.02 * ds * k.abs().max().item()
    assert got[3].abs().max().item() <= 1.02 * ds * q.abs().max().item()
    assert _same(got[0], v) and _same(got[4], do)   # p = 1 exactly


# ---------------------------------------------------------------------------
# C. GQA and MQA
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [192, 197])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("H,Hkv", [(6, 2), (4, 1), (8, 2)])
@pytest.mark.parametrize("D", DS)
def test_gqa(D, H, Hkv, causal, T):
    """dk/dv are reduced over the q heads of a kv head with fp32 atomics:
    their summation order is not fixed, so this group makes no bitwise claim
    for them, only `close`."""
    q, k, v, do = ar.make_inputs("randn", 1, H, Hkv, T, D, DEV, seed=3)
    got = _both(q, k, v, causal, do, gqa=True)
    assert got[3].shape == (1, Hkv, T, D) and got[4].shape == (1, Hkv, T, D)
    _check("C", f"D{D}H{H}kv{Hkv}T{T}{'c' if causal else 'n'}",
           got, q, k, v, causal, do)


# ---------------------------------------------------------------------------
# D. exact properties (MHA): bit-identical, no tolerance
# ---------------------------------------------------------------------------
def _fresh(like, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(like.shape, generator=g).bfloat16().to(like.device)


@pytest.mark.parametrize("t0", [37, 97, 130])
@pytest.mark.parametrize("T", [192, 256])           # v1 / v2 forward
@pytest.mark.parametrize("D", DS)
def test_causality_bitwise(D, T, t0):
    q, k, v, do = ar.make_inputs("randn", 1, 3, 3, T, D, DEV, seed=4)
    o, lse, dq, dk, dv = ar.kernel_direct(q, k, v, True, do)
    # the future cannot reach the past
    k2, v2 = k.clone(), v.clone()
    k2[:, :, t0:] = _fresh(k[:, :, t0:], 41)
    v2[:, :, t0:] = _fresh(v[:, :, t0:], 42)
    o2, lse2, dq2, _, _ = ar.kernel_direct(q, k2, v2, True, do)
    assert _same(o[:, :, :t0], o2[:, :, :t0])
    assert _same(lse[:, :, :t0], lse2[:, :, :t0])
    assert _same(dq[:, :, :t0], dq2[:, :, :t0])
    assert not _same(o[:, :, t0:], o2[:, :, t0:])    # the change was seen
    # earlier queries cannot reach later keys
    q3, do3 = q.clone(), do.clone()
    q3[:, :, :t0] = _fresh(q[:, :, :t0], 43)
    do3[:, :, :t0] = _fresh(do[:, :, :t0], 44)
    _, _, _, dk3, dv3 = ar.kernel_direct(q3, k, v, True, do3)
    assert _same(dk[:, :, t0:], dk3[:, :, t0:])
    assert _same(dv[:, :, t0:], dv3[:, :, t0:])
    assert not _same(dk[:, :, :t0], dk3[:, :, :t0])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("kv_len", [70, 129, 197, 255])
@pytest.mark.parametrize("D", DS)
def test_kv_len_masking_bitwise(D, kv_len, causal):
    """ext.attn_fwd / attn_bwd directly at T = 256: what lies in the k/v
    padding rows must not matter.  q and dO padding rows are zero in both
    calls (the wrapper's contract).  kv_len = 70 leaves whole trailing kv
    tiles masked, which the wrapper (padding to 64) never produces."""
    T = 256
    q, k, v, do = ar.make_inputs("randn", 1, 3, 3, T, D, DEV, seed=5)
    q[:, :, kv_len:] = 0
    do[:, :, kv_len:] = 0
    res = []
    for zero_pad in (True, False):
        k2, v2 = k.clone(), v.clone()
        if zero_pad:
            k2[:, :, kv_len:] = 0
            v2[:, :, kv_len:] = 0
        o, lse, dq, dk, dv = ar.ext_fwd_bwd(q, k2, v2, causal, do, kv_len)
        assert (dk[:, :, kv_len:] == 0).all() and (dv[:, :, kv_len:] == 0).all()
        res.append(tuple(t[:, :, :kv_len] for t in (o, lse, dq, dk, dv)))
    for a, b in zip(*res):
        assert _same(a, b)
    n = kv_len
    _check("D", f"D{D}kv{kv_len}{'c' if causal else 'n'}", res[1],
           q[:, :, :n], k[:, :, :n], v[:, :, :n], causal, do[:, :, :n])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", DS)
def test_batch_head_isolation_bitwise(D, causal):
    B, H, T = 2, 3, 192
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=6)
    a = ar.kernel_direct(q, k, v, causal, do)
    q2, k2, v2, do2 = (t.clone() for t in (q, k, v, do))
    for i, t in enumerate((q2, k2, v2, do2)):
        t[1, 1] = _fresh(t[1, 1], 60 + i)
    b = ar.kernel_direct(q2, k2, v2, causal, do2)
    keep = torch.ones(B, H, dtype=torch.bool)
    keep[1, 1] = False
    keep = keep.to(DEV)
    for x, y in zip(a, b):
        assert _same(x[keep], y[keep])
        assert not _same(x[1, 1], y[1, 1])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", DS)
def test_gqa_kv_head_isolation(D, causal):
    """Changing kv head j may change only q heads [j*rep, (j+1)*rep)."""
    H, Hkv, T, j = 6, 2, 192, 1
    rep = H // Hkv
    q, k, v, do = ar.make_inputs("randn", 1, H, Hkv, T, D, DEV, seed=7)
    o, lse, dq, _, _ = ar.kernel_direct(q, k, v, causal, do)
    k2, v2 = k.clone(), v.clone()
    k2[:, j] = _fresh(k[:, j], 71)
    v2[:, j] = _fresh(v[:, j], 72)
    o2, lse2, dq2, _, _ = ar.kernel_direct(q, k2, v2, causal, do)
    other = [h for h in range(H) if not j * rep <= h < (j + 1) * rep]
    assert _same(o[:, other], o2[:, other])
    assert _same(lse[:, other], lse2[:, other])
    assert _same(dq[:, other], dq2[:, other])


@pytest.mark.parametrize("T", [192, 256])
@pytest.mark.parametrize("D", DS)
def test_run_to_run_bitwise(D, T):
    q, k, v, do = ar.make_inputs("randn", 3, 5, 5, T, D, DEV, seed=8)
    a = ar.kernel_direct(q, k, v, True, do)
    b = ar.kernel_direct(q, k, v, True, do)
    for x, y in zip(a, b):
        assert _same(x, y)


# ---------------------------------------------------------------------------
# E. analytic: q = 0 counts the unmasked keys exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [130, 192, 256])
@pytest.mark.parametrize("D", DS)
def test_q_zero_counts_keys(D, T, causal):
    q, k, v, do = ar.make_inputs("qzero", 1, 3, 3, T, D, DEV, seed=9)
    o, lse, _, _, _ = ar.kernel_direct(q, k, v, causal, do)
    n = torch.arange(1, T + 1, device=DEV, dtype=torch.float64)
    if not causal:
        n = torch.full_like(n, T)
    want_lse = torch.log(n).expand(1, 3, T)
    tol = ar.lse_tolerance(q, k, causal, want_lse)
    one_key = math.log(T) - math.log(T - 1)      # smallest miscount, last row
    assert tol < one_key
    assert ar.max_err(lse, want_lse) <= tol
    v64 = v.double()
    mean = v64.cumsum(2) / n[:, None] if causal else \
        v64.mean(2, keepdim=True).expand_as(v64)
    # P = 1 exactly: fp32 sum / count, one bf16 rounding (half an ulp is at
    # most 2^-8 relative) plus the fp32 summation error
    err = (o.double() - mean).abs()
    assert (err <= 2.0 ** -8 * mean.abs() + 1e-5).all()


# ---------------------------------------------------------------------------
# F. layouts: every result bit-identical to the contiguous call
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("T", [192, 197])
@pytest.mark.parametrize("D", DS)
def test_layout_fused_qkv_buffer(D, T, causal):
    """q, k, v as slices of one [B, T, 3, H, D] leaf: row stride 3*H*D."""
    B, H = 2, 3
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=10)
    ref = ar.kernel_public(q, k, v, causal, do)
    qkv = torch.stack([t.transpose(1, 2) for t in (q, k, v)], dim=2)
    qkv = qkv.contiguous().requires_grad_(True)
    assert qkv.shape == (B, T, 3, H, D)
    qv, kv, vv = (qkv[:, :, i].transpose(1, 2) for i in range(3))
    assert qv.stride(2) == 3 * H * D and not qv.is_contiguous()
    out = ar.flash_fwd_bwd(qv, kv, vv, causal, do)
    assert _same(out, ref[0])
    for i in range(3):
        assert _same(qkv.grad[:, :, i].transpose(1, 2), ref[1 + i])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("D", DS)
def test_layout_gqa_transposed_kv(D, causal):
    """k/v as transposed views of [B, T, Hkv, D] under GQA.  out and dq are
    bit-identical to the contiguous call; dk/dv go through fp32 atomics (no
    fixed order), so they are held to `close` instead."""
    H, Hkv, T = 6, 2, 197
    q, k, v, do = ar.make_inputs("randn", 1, H, Hkv, T, D, DEV, seed=11)
    ref = ar.kernel_public(q, k, v, causal, do)
    kl = k.transpose(1, 2).contiguous().requires_grad_(True)   # [B,T,Hkv,D]
    vl = v.transpose(1, 2).contiguous().requires_grad_(True)
    ql = q.clone().requires_grad_(True)
    out = ar.flash_fwd_bwd(ql, kl.transpose(1, 2), vl.transpose(1, 2),
                           causal, do)
    assert _same(out, ref[0]) and _same(ql.grad, ref[1])
    lse = ar.kernel_direct(q, k, v, causal, do)[1]
    got = (out, lse, ql.grad, kl.grad.transpose(1, 2),
           vl.grad.transpose(1, 2))
    _check("F", f"D{D}gqa{'c' if causal else 'n'}", got, q, k, v, causal, do)


@pytest.mark.parametrize("form", ["transposed", "odd_row_stride"])
@pytest.mark.parametrize("T", [192, 197])
@pytest.mark.parametrize("D", DS)
def test_layout_noncontiguous_dout(D, T, form):
    from saturn_amd.ops.flash import _dense_rows

    B, H = 2, 3
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=12)
    ref = ar.kernel_public(q, k, v, True, do)
    if form == "transposed":
        do2 = do.transpose(1, 2).contiguous().transpose(1, 2)
        assert _dense_rows(do2) is do2               # addressed in place
    else:
        wide = torch.zeros(B, H, T, D + 4, dtype=do.dtype, device=DEV)
        wide[..., :D] = do
        do2 = wide[..., :D]
        assert do2.stride(2) % 8 != 0 and _dense_rows(do2) is not do2
    assert not do2.is_contiguous() and torch.equal(do2, do)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = ar.flash_fwd_bwd(ql, kl, vl, True, do2)
    for a, b in zip((out, ql.grad, kl.grad, vl.grad), ref):
        assert _same(a, b)


def _off(t, form):
    """A copy of t whose every row starts 8 B off a 16-B boundary."""
    if form == "column_slice":
        wide = torch.zeros(*t.shape[:-1], t.shape[-1] + 8, dtype=t.dtype,
                           device=DEV)
        view = wide[..., 4:4 + t.shape[-1]]
    else:
        flat = torch.zeros(4 + t.numel(), dtype=t.dtype, device=DEV)
        view = flat[4:].view(t.shape)
        assert view.is_contiguous()
    view.copy_(t)
    assert view.data_ptr() % 16 == 8 and view.stride(2) % 8 == 0
    return view


@pytest.mark.parametrize("form", ["column_slice", "flat_offset"])
@pytest.mark.parametrize("D", DS)
def test_layout_misaligned_rows(D, form):
    """q, k, v and dO with every row starting 8 B off a 16-B boundary: as
    column slices [4, 4+D) of wider buffers (row stride still a multiple of
    8 elements), or contiguous at an odd offset into a flat buffer (where
    .contiguous() would copy nothing).  The kernels' 16-B vector loads need
    aligned rows (attn_fwd refuses a misaligned q and no other pointer is
    checked), so the wrapper has to copy all four.  T is a multiple of 64:
    with a ragged T the wrapper's padding would make fresh tensors anyway."""
    B, H, T = 2, 3, 192
    q, k, v, do = ar.make_inputs("randn", B, H, H, T, D, DEV, seed=13)
    ref = ar.kernel_public(q, k, v, True, do)

    leaves = [_off(t, form).detach().requires_grad_(True) for t in (q, k, v)]
    assert all(t.data_ptr() % 16 == 8 for t in leaves)
    out = ar.flash_fwd_bwd(*leaves, True, _off(do, form))
    for a, b in zip((out, *(t.grad for t in leaves)), ref):
        assert _same(a, b)


@pytest.mark.parametrize("T", [64, 128])            # v1 / v2 forward
@pytest.mark.parametrize("D", DS)
def test_layout_misaligned_kv_direct(D, T):
    """k and v as column slices whose rows start 8 B off a 16-B boundary,
    straight to ext.attn_fwd / ext.attn_bwd (no wrapper, so nothing is
    copied).  Only q's pointer is held to 16 B; such k and v are accepted and
    give the bits of the contiguous call."""
    q, k, v, do = ar.make_inputs("randn", 1, 2, 2, T, D, DEV, seed=14)
    ref = ar.ext_fwd_bwd(q, k, v, True, do, T)
    got = ar.ext_fwd_bwd(q, _off(k, "column_slice"), _off(v, "column_slice"),
                         True, do, T)
    for a, b in zip(got, ref):
        assert _same(a, b)


# ---------------------------------------------------------------------------
# G. environment switches: one fresh child process per setting (each switch
# is read once per process into a static)
# ---------------------------------------------------------------------------
SETTINGS = [
    ({"SAMD_ATTN_V2": "0"}, "T256_D64", "attn_fwd_kernel<64>"),
    ({"SAMD_ATTN_BWD_TR16": "0"}, "T256_D128",
     "attn_bwd_kernel<128,0,0> attn_dq_kernel<128,0,0>"),
    ({"SAMD_ATTN_BWD_VL2": "1"}, "T256_D128", "attn_bwd_kernel<128,1,1>"),
    ({"SAMD_ATTN_DQ_GKV": "1"}, "T256_D256", "attn_dq_kernel<256,0,1>"),
    # the scalar-gather kernel with V in L2 needs both
    ({"SAMD_ATTN_BWD_TR16": "0", "SAMD_ATTN_BWD_VL2": "1"}, "T256_D64",
     "attn_bwd_kernel<64,0,1>"),
]
SWITCH_NAMES = sorted({n for s, _, _ in SETTINGS for n in s})
# child time limit = START_UP_S + SWEEP_FACTOR x the default-settings sweep
# measured in this process: interpreter + torch import + device start-up and
# code-object load on a shared machine, then the sweep with 10x headroom
START_UP_S = 120.0
SWEEP_FACTOR = 10.0
_state = {"default_seconds": None, "child_died": False}


def _default_sweep_seconds():
    if _state["default_seconds"] is None:
        ar.sweep(DEV)                                # warm: code objects loaded
        res = ar.sweep(DEV)
        assert not res["failures"], res["failures"]
        _state["default_seconds"] = res["seconds"]
        _state["default"] = res
    return _state["default_seconds"]


def test_sweep_default_settings():
    for n in SWITCH_NAMES:
        assert n not in os.environ, f"{n} is set: this suite tests the defaults"
    _default_sweep_seconds()
    res = _state["default"]
    print("ATTN_SWEEP default", json.dumps(res))
    for key, path in res["paths"].items():
        T, D = (int(x[1:]) for x in key.split("_"))
        assert path == _default_paths(T, D)


@pytest.mark.parametrize("setting,key,expect", SETTINGS,
                         ids=["+".join(f"{k}={v}" for k, v in s.items())
                              for s, _, _ in SETTINGS])
def test_switch_in_child_process(setting, key, expect):
    if _state["child_died"]:
        pytest.skip("an earlier switch child ended by signal, abort or "
                    "timeout: no further child is started")
    if ar.device_error:
        pytest.fail("not started: device error earlier in this process: "
                    + ar.device_error[0])
    limit = START_UP_S + SWEEP_FACTOR * _default_sweep_seconds()
    env = {k: v for k, v in os.environ.items() if k not in SWITCH_NAMES}
    env.update(setting)
    cmd = [sys.executable, os.path.abspath(ar.__file__), "--sweep"]
    try:
        p = subprocess.run(cmd, env=env, timeout=limit, capture_output=True,
                           text=True)
    except subprocess.TimeoutExpired:
        _state["child_died"] = True
        pytest.fail(f"{setting}: child exceeded its {limit:.0f} s limit")
    if p.returncode < 0 or p.returncode == 134:
        _state["child_died"] = True
        pytest.fail(f"{setting}: child died with status {p.returncode}\n"
                    f"{p.stderr[-2000:]}")
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if not lines or "HIP error" in p.stderr or "hipError" in p.stderr:
        # the sweep did not finish (a device error surfaces as an exception,
        # status 1, no result line): treated like a signal, no further child
        _state["child_died"] = True
        pytest.fail(f"{setting}: child gave no result or hit a device error "
                    f"(status {p.returncode})\n{p.stderr[-2000:]}")
    res = json.loads(lines[-1])
    print("ATTN_SWEEP", json.dumps(setting), f"limit {limit:.0f}s",
          json.dumps(res))
    assert expect in res["paths"][key], (expect, res["paths"][key])
    assert not res["failures"], res["failures"]
    assert p.returncode == 0
    assert len(res["cases"]) == 2 * len(ar.SWEEP_CASES)


# ---------------------------------------------------------------------------
# H. attn_bwd checks its arguments on the host, before any launch
# ---------------------------------------------------------------------------
BAD_BWD_ARGS = [
    ("o", "T128", lambda a: a["o"].new_zeros(1, 2, 128, 64)),
    ("dout", "D128", lambda a: a["dout"].new_zeros(1, 2, 64, 128)),
    ("lse", "fp64", lambda a: a["lse"].double()),
    # a [B, T, H] tensor transposed: the right sizes, the wrong strides
    ("lse", "noncontiguous",
     lambda a: a["lse"].transpose(1, 2).contiguous().transpose(1, 2)),
    ("v", "T128", lambda a: a["v"].new_zeros(1, 2, 128, 64)),
    ("k", "fp32", lambda a: a["k"].float()),
]


@pytest.mark.parametrize("name,what,make", BAD_BWD_ARGS,
                         ids=[f"{n}-{w}" for n, w, _ in BAD_BWD_ARGS])
def test_bwd_refuses_bad_argument(name, what, make):
    q, k, v, do = ar.make_inputs("randn", 1, 2, 2, 64, 64, DEV, seed=15)
    o, lse = _ext().attn_fwd(q, k, v, True, 64)
    a = {"dout": do, "q": q, "k": k, "v": v, "o": o, "lse": lse}
    a[name] = make(a)
    if name == "lse":
        assert a["lse"].shape == lse.shape
    with pytest.raises(RuntimeError) as e:
        _ext().attn_bwd(a["dout"], a["q"], a["k"], a["v"], a["o"], a["lse"],
                        True, 64)
    msg = str(e.value).splitlines()[0]
    assert msg.startswith("attn_bwd:") and re.search(rf"\b{name}\b", msg), msg
    torch.cuda.synchronize()                         # and nothing was launched
