"""Sliding-window / packed-document attention on the CPU: the reference and
its mutants (does the criterion of the GPU tests reject planted bugs at the
GPU tests' own shapes?), the bound helpers, and the model plumbing."""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import attn_window_ref as wr  # noqa: E402


# ---------------------------------------------------------------------------
# 1. reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("hkv", [3, 1])
def test_zero_bound_is_the_causal_reference(hkv):
    q, k, v, do = ar.make_inputs("randn", 2, 3, hkv, 192, 64)
    for lo in (torch.zeros(192, dtype=torch.int32),
               torch.zeros(2, 192, dtype=torch.int32)):
        for a, b in zip(wr.ref64_lo(q, k, v, lo, do),
                        ar.ref64(q, k, v, True, do)):
            assert torch.equal(a, b)
        for a, b in zip(wr.base_bf16_lo(q, k, v, lo, do),
                        ar.base_bf16(q, k, v, True, do)):
            assert torch.equal(a, b)
        assert wr.lse_tolerance_lo(q, k, lo, ar.ref64(q, k, v, True)[1]) == \
            ar.lse_tolerance(q, k, True, ar.ref64(q, k, v, True)[1])


# ---------------------------------------------------------------------------
# 2. mutation check, at the shapes of the GPU matrix
# ---------------------------------------------------------------------------
ALL5 = set(ar.NAMES)
# mutant -> (tensors it must be rejected on, bounds it does nothing to)
MUTANTS = {
    "lo_plus": (ALL5, ()),
    "lo_minus": (ALL5, ()),
    # W=65 at T=256: every block's first bound (0, 0, 64, 128) is a multiple
    # of 32, so rounding up changes nothing
    "round_up": ({"out", "lse"}, ("W65_T256",)),
    "early_stop": ({"dk", "dv"}, ()),
}


@pytest.mark.parametrize("D,bound,kind", wr.MATRIX,
                         ids=[f"D{d}-{b}-{k}" for d, b, k in wr.MATRIX])
def test_criterion_rejects_planted_bugs(D, bound, kind):
    T = wr.BOUNDS[bound][0]
    c = wr.case(kind, *wr.BH, wr.BH[1], T, D, bound)
    q, k, v, do, lo = (c[n] for n in ("q", "k", "v", "do", "lo"))
    # the clean floor passes its own criterion
    _, bad = wr.check_case_lo(c["base"], c["ref"], c["base"], c["lse_tol"])
    assert not bad, bad
    for name, (must, noop) in MUTANTS.items():
        got = wr.base_bf16_lo(q, k, v, lo, do, mut=(name,))
        if bound in noop:
            assert all(torch.equal(a, b) for a, b in zip(got, c["base"]))
            continue
        _, bad = wr.check_case_lo(got, c["ref"], c["base"], c["lse_tol"])
        missed = must - wr.rejected(bad)
        assert not missed, (name, sorted(missed), bad)


# ---------------------------------------------------------------------------
# 3. helpers
# ---------------------------------------------------------------------------
def _monotone_le_t(lo):
    T = lo.shape[-1]
    t = torch.arange(T)
    return bool((lo >= 0).all() and (lo <= t).all()
                and (lo[..., 1:] >= lo[..., :-1]).all())


@pytest.mark.parametrize("T,W", [(1, 1), (7, 1), (64, 17), (100, 100),
                                 (100, 101), (130, 64)])
def test_window_lo_matches_loop(T, W):
    from saturn_amd.ops.flash import window_lo

    lo = window_lo(T, W, "cpu")
    assert lo.dtype == torch.int32 and lo.shape == (T,)
    assert torch.equal(lo, wr.window_bound(T, W))
    assert _monotone_le_t(lo)
    assert window_lo(T, W, "cpu") is lo          # cached
    with pytest.raises(ValueError):
        window_lo(T, 0, "cpu")


def _document_loop(ids, sep):
    rows = []
    for row in ids.tolist():
        start, out = 0, []
        for t, tok in enumerate(row):
            out.append(start)
            if tok == sep:
                start = t + 1
        rows.append(out)
    return torch.tensor(rows, dtype=torch.int32)


def test_document_lo_matches_loop():
    from saturn_amd.ops.flash import document_lo

    SEP = 7
    T = 24
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(8, 50, (5, T), generator=g)
    ids[0, 0] = SEP                       # separator at position 0
    ids[1, T - 1] = SEP                   # separator at position T-1
    ids[2, 9] = ids[2, 10] = ids[2, 11] = SEP   # adjacent separators
    ids[3, [0, 1, 5, T - 2, T - 1]] = SEP
    # row 4: one document
    lo = document_lo(ids, SEP)
    assert lo.dtype == torch.int32 and lo.shape == (5, T)
    assert torch.equal(lo, _document_loop(ids, SEP))
    assert _monotone_le_t(lo)
    assert lo[0, 0] == 0 and lo[0, 1] == 1
    assert lo[1, T - 1] == lo[1, T - 2]   # the separator ends ITS document
    assert lo[2, 10] == 10 and lo[2, 11] == 11 and lo[2, 12] == 12
    assert int(lo[4].max()) == 0
    with pytest.raises(ValueError):
        document_lo(ids[0], SEP)


def test_window_and_documents_combine_to_the_maximum():
    from saturn_amd.ops.flash import document_lo, resolve_lo, window_lo

    T, W, SEP = 40, 6, 0
    ids = torch.randint(1, 9, (3, T), generator=torch.Generator().manual_seed(1))
    ids[0, [4, 5, 20]] = SEP
    ids[1, [0, 39]] = SEP
    dl = document_lo(ids, SEP)
    dev = torch.device("cpu")
    both = resolve_lo(T, dev, True, W, dl)
    assert both.dtype == torch.int32
    assert torch.equal(both, torch.maximum(dl, window_lo(T, W, dev)))
    assert _monotone_le_t(both)
    assert torch.equal(resolve_lo(T, dev, True, None, dl), dl)
    assert torch.equal(resolve_lo(T, dev, True, T + 3, dl), dl)
    assert resolve_lo(T, dev, True, None, None) is None
    assert resolve_lo(T, dev, True, T, None) is None
    assert resolve_lo(T, dev, True, T + 5, None) is None
    assert torch.equal(resolve_lo(T, dev, True, T - 1, None),
                       window_lo(T, T - 1, dev))
    # an explicit bound is brought into the kernels' contract
    wild = torch.tensor([[5, -3, 9, 1] + [2] * (T - 4)], dtype=torch.int32)
    assert _monotone_le_t(resolve_lo(T, dev, True, None, wild))
    with pytest.raises(ValueError):
        resolve_lo(T, dev, False, W, None)
    with pytest.raises(ValueError):
        resolve_lo(T, dev, False, None, dl)
    with pytest.raises(ValueError):
        resolve_lo(T, dev, True, 0, None)
    with pytest.raises(ValueError):
        resolve_lo(T, dev, True, None, dl.long())
    with pytest.raises(ValueError):
        resolve_lo(T, dev, True, None, dl[:, :-1])


@pytest.mark.parametrize("bound", ["W17_T192", "docs_T192"])
def test_attention_math_with_bound_matches_fp64(bound):
    from saturn_amd.ops.functional import attention_math, causal_attention

    T = wr.BOUNDS[bound][0]
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(2, 3, T, 64, generator=g) for _ in range(3))
    lo = wr.make_bound(bound)
    ref, _ = wr.ref64_lo(q, k, v, lo)           # fp32 inputs, upcast exactly
    out = attention_math(q, k, v, kv_lo=lo)
    assert out.dtype == torch.float32
    assert (out.double() - ref).abs().max().item() < 1e-6
    assert torch.equal(out, causal_attention(q, k, v, kv_lo=lo))
    with pytest.raises(ValueError):
        attention_math(q, k, v, causal=False, kv_lo=lo)


def test_flash_attention_rejects_bounds_without_causal():
    from saturn_amd.ops.flash import flash_attention

    q = torch.randn(1, 2, 64, 64)
    lo = torch.zeros(64, dtype=torch.int32)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False, window=8)
    with pytest.raises(ValueError):
        flash_attention(q, q, q, causal=False, kv_lo=lo)


# ---------------------------------------------------------------------------
# 4. models
# ---------------------------------------------------------------------------
def _explicit_window_attention(W):
    """A stand-in for causal_attention: masked softmax written out."""
    def attn(q, k, v, window=None, kv_lo=None):
        B, H, T, D = q.shape
        rep = H // k.shape[1]
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
        s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(D)
        t = torch.arange(T)
        ok = (t[None, :] <= t[:, None]) & (t[:, None] - t[None, :] < W)
        p = torch.softmax(s.masked_fill(~ok, float("-inf")), dim=-1)
        return torch.matmul(p, v.float()).to(q.dtype)
    return attn


def _tiny_llama(sliding_window):
    from saturn_amd.models.llama import LlamaConfig, LlamaForCausalLM

    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(
        vocab_size=128, n_ctx=96, n_embd=64, n_head=4, n_kv_head=2,
        n_layer=2, ffn_dim=128, sliding_window=sliding_window))


def _tiny_mixtral(sliding_window):
    from saturn_amd.models.mixtral import get_mixtral_model

    return get_mixtral_model({
        "vocab_size": 128, "n_ctx": 96, "n_embd": 64, "n_head": 4,
        "n_kv_head": 2, "n_layer": 2, "ffn_dim": 64, "n_expert": 4,
        "top_k": 2, "sliding_window": sliding_window})


@pytest.mark.parametrize("make", [_tiny_llama, _tiny_mixtral],
                         ids=["llama", "mixtral"])
def test_model_sliding_window(make, monkeypatch):
    T = 96
    x = torch.randint(0, 128, (2, T), generator=torch.Generator().manual_seed(2))
    with torch.no_grad():
        plain = make(None)(x)
        # a window that covers the sequence is the plain model
        assert torch.equal(make(T)(x), plain)
        assert torch.equal(make(T + 7)(x), plain)
        m = make(20)
        assert m.cfg.sliding_window == 20
        got = m(x)
        assert not torch.equal(got, plain)
        import saturn_amd.models.llama as llama_mod

        monkeypatch.setattr(llama_mod, "causal_attention",
                            _explicit_window_attention(20))
        want = m(x)
    # the same fp32 operations up to the order of a few hundred roundings
    assert (got - want).abs().max().item() < 1e-5


def test_get_llama_model_takes_sliding_window():
    from saturn_amd.models.llama import PRESETS, get_llama_model

    with torch.device("meta"):
        m = get_llama_model({"preset": "mistral-7b"})
    cfg = m.cfg
    assert (cfg.vocab_size, cfg.n_layer, cfg.n_head, cfg.n_kv_head,
            cfg.ffn_dim, cfg.n_embd) == (32000, 32, 32, 8, 14336, 4096)
    assert cfg.rope_theta == 10000.0 and cfg.sliding_window == 4096
    assert cfg.n_ctx == 8192
    assert m.h[0].self_attn.sliding_window == 4096
    assert PRESETS["8b"].sliding_window is None
    with torch.device("meta"):
        m = get_llama_model({"preset": "mistral-7b", "n_layer": 1,
                             "n_ctx": 256, "sliding_window": 128})
    assert m.cfg.sliding_window == 128 and m.cfg.n_ctx == 256


def _sp2_window_worker(rank, world, _):
    from saturn_amd.executors.launch import destroy_process_group, init_process_group
    from saturn_amd.ops.functional import fused_cross_entropy
    from saturn_amd.parallel.sequence import sp_region
    from saturn_amd.models.llama import llama_loss

    init_process_group(rank, world)
    try:
        m = _tiny_llama(20)
        x = torch.randint(0, 128, (2, 96),
                          generator=torch.Generator().manual_seed(5))
        B, T = x.shape
        Tl = T // world
        lo = rank * Tl
        labels = torch.full((B, Tl), -100, dtype=torch.long)
        hi = min(lo + Tl + 1, T)
        labels[:, : hi - lo - 1] = x[:, lo + 1 : hi]
        with sp_region(world, rank):
            logits = m(x[:, lo : lo + Tl].contiguous())
            local_mean = fused_cross_entropy(logits, labels, shift=False)
        n_local = int((labels != -100).sum())
        loss = local_mean * (n_local * world / (B * (T - 1)))
        loss.backward()
        import torch.distributed as dist

        g = m.wte.weight.grad.clone()
        dist.all_reduce(g)
        g /= world

        ref = _tiny_llama(20)
        ref_logits = ref(x)
        llama_loss(ref_logits, x).backward()
        plain = _tiny_llama(None)(x)
        if rank == 0:
            return (
                float((logits - ref_logits[:, :Tl]).abs().max()),
                float((g - ref.wte.weight.grad).abs().max()),
                float(ref.wte.weight.grad.abs().max()),
                float((plain - ref_logits).abs().max()),
            )
        return None
    finally:
        destroy_process_group()


def test_sp2_sliding_window_matches_full_sequence():
    from saturn_amd.executors.launch import gang_spawn

    ldiff, gdiff, gmax, window_effect = gang_spawn(
        _sp2_window_worker, 2, 963, None, timeout=300)
    # the bound of tests/test_sp_cpu.py
    assert gdiff < 5e-5 * max(1.0, gmax), (gdiff, gmax)
    assert ldiff < 5e-5, ldiff
    assert window_effect > 1e-3      # the window really changes this model
