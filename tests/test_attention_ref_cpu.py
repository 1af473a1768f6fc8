"""CPU checks of the attention conformance tooling (tests/attn_ref.py):
the fp64 reference against torch's own attention, the mutation check (the
acceptance criterion must reject every planted bug at the shapes the GPU
tests use, and the old whole-tensor bound must be shown to miss one), and
the wrapper's padding / layout helpers."""

import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402  (plain helper module beside this file)
from saturn_amd.ops import flash


# ---------------------------------------------------------------------------
# ref64 against F.scaled_dot_product_attention in fp64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv,T,D", [
    (1, 3, 3, 64, 64),      # one tile
    (2, 3, 3, 197, 64),     # ragged
    (1, 6, 2, 130, 128),    # GQA rep 3, ragged
    (1, 4, 1, 65, 256),     # MQA
])
def test_ref64_matches_sdpa(B, H, Hkv, T, D, causal):
    q, k, v, do = ar.make_inputs("randn", B, H, Hkv, T, D)
    out, lse, dq, dk, dv = ar.ref64(q, k, v, causal, do)
    rep = H // Hkv
    q64 = q.double().requires_grad_()
    k64 = k.double().requires_grad_()
    v64 = v.double().requires_grad_()
    o2 = F.scaled_dot_product_attention(
        q64, k64.repeat_interleave(rep, 1), v64.repeat_interleave(rep, 1),
        is_causal=causal)
    g = torch.autograd.grad(o2, (q64, k64, v64), do.double())
    assert dk.shape == k.shape and dv.shape == v.shape
    for a, b in ((out, o2), (dq, g[0]), (dk, g[1]), (dv, g[2])):
        assert ar.max_err(a, b) < 1e-12
    # lse against its definition, row by row
    s = torch.matmul(q.double(), k.double().repeat_interleave(rep, 1)
                     .transpose(-1, -2)) / math.sqrt(D)
    for i in (0, T // 2, T - 1):
        n = i + 1 if causal else T
        want = torch.logsumexp(s[:, :, i, :n], dim=-1)
        assert ar.max_err(lse[:, :, i], want) < 1e-12


def test_ulp_bf16():
    assert ar.ulp_bf16(1.0) == 2.0 ** -7
    assert ar.ulp_bf16(1.99) == 2.0 ** -7
    assert ar.ulp_bf16(2.0) == 2.0 ** -6
    assert ar.ulp_bf16(0.3) == 2.0 ** -9
    assert ar.ulp_bf16(0.0) == 0.0
    x = torch.tensor([1.0, 3.0, 0.3])
    nxt = (x.bfloat16().view(torch.int16) + 1).view(torch.bfloat16).float()
    assert [ar.ulp_bf16(t) for t in x.tolist()] == (nxt - x.bfloat16().float()).tolist()


# ---------------------------------------------------------------------------
# the floor itself meets the criterion and the LSE check is not vacuous
# ---------------------------------------------------------------------------
SHAPES = [
    # (B, H, Hkv, T, D): shapes of the GPU tests' groups A, B and C
    (1, 3, 3, 192, 64),
    (3, 5, 5, 320, 128),
    (1, 3, 3, 512, 256),
    (1, 3, 3, 130, 64),
    (1, 3, 3, 257, 128),
    (1, 6, 2, 197, 128),
    (1, 4, 1, 192, 64),
]


@pytest.mark.parametrize("kind", ["randn", "peaky"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv,T,D", SHAPES)
def test_floor_passes_its_own_criterion(B, H, Hkv, T, D, causal, kind):
    """base_bf16 fed back as the 'kernel' must pass (ratio 1 by
    construction), including tolerance < one-key shift for the LSE: on
    every head for randn inputs, on at least one head for the peaky ones
    (their edge key weighs ~1e-6 on some heads)."""
    q, k, v, do = ar.make_inputs(kind, B, H, Hkv, T, D)
    got = ar.base_bf16(q, k, v, causal, do)
    rep, bad = ar.check_case(got, q, k, v, causal, do,
                             every_head=(kind != "peaky"))
    print(kind, causal, (B, H, Hkv, T, D), rep["lse"])
    assert not bad, bad


# ---------------------------------------------------------------------------
# mutation check
# ---------------------------------------------------------------------------
def _mutations(B, H, Hkv, T, D, causal):
    """(mutation, the checks that must reject it).  Faults that move whole
    elements (a zeroed block, swapped columns, a wrong kv head, a mask error
    at a short row) must be rejected by `close` on the named tensor.  A
    one-key mask error at a long row changes out and the gradients of that
    row by about one part in the row length, which is below what bf16
    tensors resolve (`close` is 2 x floor + ulp): the LSE check must reject
    those, and is sized for it (tolerance < one-key shift)."""
    muts = [
        (("dk_zero", B - 1, Hkv - 1, (T // 2) & ~15), ["dk: max err"]),
        (("o_swap", D - 32), ["out: max err"]),
        (("kv_len", -1), ["lse: max err"]),
    ]
    if causal:
        muts.append((("causal_row", 1), ["out: max err", "lse: max err"]))
        muts.append((("causal_row", T - 3), ["lse: max err"]))
    else:
        # under a causal mask no valid row can see key T: not a bug there
        muts.append((("kv_len", +1), ["lse: max err"]))
    if Hkv not in (1, H):
        muts.append((("gqa_mod",), ["out: max err", "dq: max err",
                                    "dk: max err", "dv: max err"]))
    return muts


def _mutated(q, k, v, causal, do, mut):
    """The mutated composition, run the way the kernels run: on inputs
    zero-padded to 64 rows with kv_len = T, sliced back."""
    T = q.shape[2]
    qp, kp, vp, dop = (flash._pad_t64(t) for t in (q, k, v, do))
    if T % 64 == 0 and mut == ("kv_len", +1):
        # no padding row to admit: give it one
        qp, kp, vp, dop = (F.pad(t, (0, 0, 0, 64)) for t in (q, k, v, do))
    res = ar.base_bf16(qp, kp, vp, causal, dop, kv_len=T, mut=mut)
    return tuple(t[:, :, :T] for t in res)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("B,H,Hkv,T,D", SHAPES)
def test_criterion_rejects_planted_bugs(B, H, Hkv, T, D, causal):
    q, k, v, do = ar.make_inputs("randn", B, H, Hkv, T, D)
    ref = ar.ref64(q, k, v, causal, do)
    # unmutated, through the same padded route: passes
    rep, bad = ar.check_case(_mutated(q, k, v, causal, do, None),
                             q, k, v, causal, do, ref=ref)
    assert not bad, bad
    for mut, must in _mutations(B, H, Hkv, T, D, causal):
        got = _mutated(q, k, v, causal, do, mut)
        rep, bad = ar.check_case(got, q, k, v, causal, do, ref=ref)
        print(mut, bad)
        for check in must:
            assert any(b.startswith(check) for b in bad), \
                f"planted bug {mut} not rejected by '{check}': {bad}"


def test_old_norm_check_accepts_single_row_bug():
    """The documented reason for the new metric: a causal off-by-one at one
    row passes the whole-tensor 4e-2 / 5e-2 bounds on every tensor, and is
    rejected by the LSE check."""
    B, H, Hkv, T, D = 1, 3, 3, 192, 64
    q, k, v, do = ar.make_inputs("randn", B, H, Hkv, T, D)
    ref = ar.ref64(q, k, v, True, do)
    got = ar.base_bf16(q, k, v, True, do, mut=("causal_row", T - 3))
    for name, x, r in zip(ar.NAMES, got, ref):
        if name == "lse":
            continue
        tol = ar.NORM_TOL_FWD if name == "out" else ar.NORM_TOL_BWD
        assert ar.rel_err(x, r) < tol, name
    rep, bad = ar.check_case(got, q, k, v, True, do, ref=ref)
    assert any(b.startswith("lse: max err") for b in bad), bad


# ---------------------------------------------------------------------------
# flash._pad_t64 / flash._dense_rows
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 63, 64, 65, 128, 192])
def test_pad_t64(T):
    x = torch.randn(2, 3, T, 8).bfloat16()
    p = flash._pad_t64(x)
    Tp = T + (-T) % 64
    assert p.shape == (2, 3, Tp, 8) and p.dtype == x.dtype
    assert torch.equal(p[:, :, :T], x)
    assert (p[:, :, T:] == 0).all()
    if T % 64 == 0:
        assert p is x                       # no copy for full tiles
    # a transposed [B,T,H,D] view pads to the same values
    xv = x.transpose(1, 2).contiguous().transpose(1, 2)
    assert torch.equal(flash._pad_t64(xv), p)


@pytest.mark.parametrize("T", [1, 63, 64, 65, 128])
def test_dense_rows(T):
    B, H, D = 2, 3, 16
    c = torch.randn(B, H, T, D).bfloat16()
    assert flash._dense_rows(c) is c
    # the model's layout: [B,T,H,D] physical, viewed as [B,H,T,D]
    tv = torch.randn(B, T, H, D).bfloat16().transpose(1, 2)
    assert flash._dense_rows(tv) is tv
    # a slice of a fused [B,T,3,H,D] buffer: row stride 3*H*D
    fused = torch.randn(B, T, 3, H, D).bfloat16()
    kv = fused[:, :, 1].transpose(1, 2)
    assert kv.stride(2) == 3 * H * D and flash._dense_rows(kv) is kv
    # row stride not a multiple of 8 elements (16 B): must copy
    wide = torch.randn(B, H, T, D + 4).bfloat16()
    odd = wide[..., :D]
    assert odd.stride(2) % 8 != 0
    d = flash._dense_rows(odd)
    assert d is not odd and d.is_contiguous() and torch.equal(d, odd)
    # a column slice that starts off a 16-B boundary: every row misaligned
    wide8 = torch.randn(B, H, T, D + 8).bfloat16()
    off = wide8[..., 4:4 + D]
    assert off.stride(2) % 8 == 0 and off.storage_offset() % 8 != 0
    d = flash._dense_rows(off)
    assert d is not off and d.is_contiguous() and torch.equal(d, off)
    # contiguous already, but starting off a boundary: needs a real copy
    flat = torch.randn(4 + B * H * T * D).bfloat16()
    co = flat[4:].view(B, H, T, D)
    assert co.is_contiguous() and co.data_ptr() % 16 != 0
    d = flash._dense_rows(co)
    assert d.data_ptr() % 16 == 0 and d.is_contiguous() and torch.equal(d, co)
    # ... while one that starts on a boundary stays a view
    al = wide8[..., 8:8 + D]
    assert flash._dense_rows(al) is al
    # innermost dim not dense: must copy
    sw = torch.randn(B, H, D, T).bfloat16().transpose(2, 3)
    d = flash._dense_rows(sw)
    assert d.stride(-1) == 1 and torch.equal(d, sw)
