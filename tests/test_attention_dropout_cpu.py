"""Attention dropout without a GPU: the keep function's twin
(saturn_amd.ops.flash.dropout_keep), the math path, the reference and floor
of tests/attn_dropout_ref.py with its mutation check, the models' attn_pdrop
and the refusals.
"""

import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as ar  # noqa: E402
import attn_dropout_ref as dr  # noqa: E402

from saturn_amd.ops import flash  # noqa: E402
from saturn_amd.ops.functional import (  # noqa: E402
    attention_math,
    causal_attention,
    full_attention,
)

SEEDS = (1234, 0, 2**61 + 7)
PS = (0.1, 0.5, 0.9)


# ---------------------------------------------------------------------------
# 1. dropout_keep
# ---------------------------------------------------------------------------
def _keep_py(seed, bh, i, j, thr):
    """The keep function in plain Python integers (the definition)."""
    M = (1 << 64) - 1
    z = ((seed & M) ^ ((bh << 40) | (i << 20) | (j >> 2))) & M
    z = (z + 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    z ^= z >> 31
    return ((z >> (16 * (j & 3))) & 0xFFFF) >= thr


@pytest.mark.parametrize("seed", SEEDS + (-5, 2**63 - 1))
def test_keep_matches_the_integer_definition(seed):
    B, H, T, p = 2, 3, 11, 0.3
    thr, _ = flash.dropout_threshold(p)
    got = flash.dropout_keep(seed, B, H, T, p)
    assert got.dtype == torch.bool and got.shape == (B, H, T, T)
    for bh in range(B * H):
        for i in range(T):
            for j in range(T):
                assert bool(got[bh // H, bh % H, i, j]) == _keep_py(
                    seed, bh, i, j, thr), (bh, i, j)


def test_keep_is_deterministic_and_ragged_is_a_corner():
    a = flash.dropout_keep(77, 2, 3, 256, 0.25)
    assert torch.equal(a, flash.dropout_keep(77, 2, 3, 256, 0.25))
    for T in (130, 197, 1, 3):
        assert torch.equal(flash.dropout_keep(77, 2, 3, T, 0.25),
                           a[:, :, :T, :T]), T
    # B enters only through b*H + h
    assert torch.equal(flash.dropout_keep(77, 1, 6, 64, 0.25).view(2, 3, 64, 64),
                       a[:, :, :64, :64])


def test_keep_differs_across_seeds_heads_and_batches():
    a = flash.dropout_keep(1, 2, 3, 64, 0.5)
    b = flash.dropout_keep(2, 2, 3, 64, 0.5)
    assert not torch.equal(a, b)
    flat = a.view(6, -1)
    for x in range(6):
        for y in range(x + 1, 6):
            # independent fair bits agree on about half of 4096 positions
            agree = (flat[x] == flat[y]).float().mean().item()
            assert 0.4 < agree < 0.6, (x, y, agree)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", PS)
def test_keep_count_is_binomial(seed, p):
    """n = 2*3*256*256 independent draws with keep probability 1 - thr/65536:
    the count is within 4 sigma (two-sided 6e-5 per case; the chosen function
    stays under 1.3 sigma in all nine)."""
    thr, _ = flash.dropout_threshold(p)
    pe = thr / 65536.0
    k = flash.dropout_keep(seed, 2, 3, 256, p)
    n = k.numel()
    sig = (k.sum().item() - n * (1 - pe)) / math.sqrt(n * pe * (1 - pe))
    print(f"DROPOUT_KEEP seed={seed} p={p} sigma={sig:+.2f}")
    assert abs(sig) < 4.0, sig


def test_threshold():
    assert flash.dropout_threshold(0.0) == (0, 1.0)
    assert flash.dropout_threshold(0.5) == (32768, 2.0)
    thr, r = flash.dropout_threshold(0.1)
    assert thr == 6554 and r == torch.tensor(65536.0 / (65536 - 6554),
                                             dtype=torch.float32).item()
    # thr == 0 keeps everything (p below 2^-17 is no dropout)
    assert flash.dropout_threshold(2.0 ** -18)[0] == 0
    assert flash.dropout_keep(5, 1, 2, 33, 2.0 ** -18).all()
    assert flash.dropout_keep(5, 1, 2, 33, 0.0).all()
    assert flash.dropout_threshold(0.99999999)[0] == 65535


# ---------------------------------------------------------------------------
# the reference and the floor reduce to attn_ref's, exactly
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
def test_all_true_mask_is_the_plain_reference(causal):
    q, k, v, do = ar.make_inputs("randn", 1, 4, 2, 96, 64, seed=3)
    ones = torch.ones(1, 4, 96, 96, dtype=torch.bool)
    for a, b in zip(dr.ref64_drop(q, k, v, causal, ones, 1.0, do),
                    ar.ref64(q, k, v, causal, do)):
        assert torch.equal(a, b)
    for a, b in zip(dr.base_bf16_drop(q, k, v, causal, ones, 1.0, do),
                    ar.base_bf16(q, k, v, causal, do)):
        assert torch.equal(a, b)
    for a, b in zip(dr.base_bf16_drop(q, k, v, causal, ones, 1.0, do, kv_len=90),
                    ar.base_bf16(q, k, v, causal, do, kv_len=90)):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 2. attention_math
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_math_matches_ref64_drop(causal, p):
    B, H, T, D = 2, 3, 70, 32
    q, k, v, do = (t.float() for t in ar.make_inputs("randn", B, H, H, T, D, seed=5))
    keep, r = dr.keep_r(991, B, H, T, p)
    ref = dr.ref64_drop(q, k, v, causal, keep, r, do)
    ql, kl, vl = (t.clone().requires_grad_(True) for t in (q, k, v))
    out = attention_math(ql, kl, vl, causal=causal, dropout_p=p, seed=991)
    out.backward(do)
    # fp32 softmax and GEMMs over T = 70, D = 32 against fp64: a few 1e-6
    for name, x, y in zip(("out", "dq", "dk", "dv"),
                          (out, ql.grad, kl.grad, vl.grad),
                          (ref[0], ref[2], ref[3], ref[4])):
        err = ar.max_err(x.detach(), y)
        assert err <= 2e-5 * max(1.0, y.abs().max().item()), (name, err)


def test_attention_math_p0_is_bit_identical():
    q, k, v, _ = ar.make_inputs("randn", 1, 2, 2, 50, 32, seed=6)
    for causal in (True, False):
        a = attention_math(q, k, v, causal=causal)
        assert torch.equal(a, attention_math(q, k, v, causal=causal,
                                             dropout_p=0.0, seed=123))
    assert torch.equal(causal_attention(q, k, v),
                       causal_attention(q, k, v, dropout_p=0.0, seed=9))
    assert torch.equal(full_attention(q, k, v),
                       full_attention(q, k, v, dropout_p=0.0, seed=9))


def test_public_cpu_routes_share_the_mask_and_draw_seeds():
    q, k, v, _ = ar.make_inputs("randn", 1, 4, 2, 40, 32, seed=8)   # GQA
    a = causal_attention(q, k, v, dropout_p=0.5, seed=17)
    kk, vv = (t.repeat_interleave(2, dim=1) for t in (k, v))
    assert torch.equal(a, attention_math(q, kk, vv, causal=True,
                                         dropout_p=0.5, seed=17))
    torch.manual_seed(3)
    b = full_attention(q, kk, vv, dropout_p=0.5)
    c = full_attention(q, kk, vv, dropout_p=0.5)
    torch.manual_seed(3)
    assert torch.equal(b, full_attention(q, kk, vv, dropout_p=0.5))
    assert not torch.equal(b, c)


# ---------------------------------------------------------------------------
# 3. mutation check at the GPU matrix's shapes
# ---------------------------------------------------------------------------
MUT_SHAPES = sorted({(D, T, causal) for D, T, causal, _, _ in dr.MATRIX})


@pytest.mark.parametrize("D,T,causal", MUT_SHAPES,
                         ids=[f"D{d}-T{t}-{'c' if c else 'n'}" for d, t, c in MUT_SHAPES])
def test_mutants_are_rejected(D, T, causal):
    """Each planted bug must fail `close` (factor 2 over the floor) on every
    tensor the table names, at every shape of the GPU matrix and at the
    smaller of its two rates (fewer dropped entries: the harder case)."""
    c = dr.case("randn", *dr.BH, dr.BH[1], T, D, causal, 0.1)
    q, k, v, do, keep, r = (c[n] for n in ("q", "k", "v", "do", "keep", "r"))
    keep2, _ = dr.keep_r(c["seed"] + 1, *dr.BH, T, 0.1)
    # the unmutated floor passes its own criterion trivially (ratio 1)
    for i, name in enumerate(dr.NAMES):
        if name != "lse":
            assert ar.close(c["base"][i], c["ref"][i], c["base"][i])
    for kind, tensors in dr.MUTANTS.items():
        mut = (kind, keep2) if kind == "bwd_seed" else (kind,)
        got = dr.base_bf16_drop(q, k, v, causal, keep, r, do, mut=mut)
        for name in tensors:
            i = dr.NAMES.index(name)
            info = ar.close_info(got[i], c["ref"][i], c["base"][i])
            assert not info["ok"], (kind, name, info)


# ---------------------------------------------------------------------------
# 4. models
# ---------------------------------------------------------------------------
def _gptj(**kw):
    from saturn_amd.models.gptj import get_gptj_model

    return get_gptj_model(dict(n_layer=2, n_embd=64, n_head=4, n_ctx=32,
                               vocab_size=97, rotary_dim=8, **kw))


def _bert(**kw):
    from saturn_amd.models.bert import get_bert_model

    return get_bert_model(dict(n_layer=2, n_embd=64, n_head=4, n_ctx=32,
                               vocab_size=97, **kw))


@pytest.mark.parametrize("make", [_gptj, _bert], ids=["gptj", "bert"])
def test_models_attn_pdrop(make):
    x = torch.randint(0, 97, (2, 32), generator=torch.Generator().manual_seed(1))
    plain, zero, drop = make(), make(attn_pdrop=0.0), make(attn_pdrop=0.5)
    assert list(plain.state_dict()) == list(drop.state_dict())
    assert list(plain.state_dict()) == list(zero.state_dict())
    for a, b in zip(plain.state_dict().values(), drop.state_dict().values()):
        assert torch.equal(a, b)
    # eval: dropout off, bit for bit the attn_pdrop = 0 model
    base = plain.eval()(x)
    assert torch.equal(drop.eval()(x), base)
    assert torch.equal(zero.eval()(x), base)
    # attn_pdrop = 0 trains on the present path
    assert torch.equal(zero.train()(x), plain.train()(x))
    # train: two forwards differ, a fixed manual_seed reproduces
    drop.train()
    torch.manual_seed(11)
    a = drop(x)
    b = drop(x)
    torch.manual_seed(11)
    a2 = drop(x)
    assert not torch.equal(a, b)
    assert torch.equal(a, a2)
    assert not torch.equal(a, plain(x))
    a.float().sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in drop.parameters()
               if p.grad is not None)


def test_every_config_has_attn_pdrop():
    from saturn_amd.models.bert import BertConfig
    from saturn_amd.models.gpt2 import GPT2Config, get_gpt2_model
    from saturn_amd.models.gptj import GPTJConfig
    from saturn_amd.models.llama import LlamaConfig
    from saturn_amd.models.mixtral import MixtralConfig
    from saturn_amd.models.vit import ViTConfig

    for cfg in (BertConfig, GPT2Config, GPTJConfig, LlamaConfig,
                MixtralConfig, ViTConfig):
        assert cfg().attn_pdrop == 0.0, cfg
    m = get_gpt2_model({"n_layer": 1, "n_ctx": 16, "attn_pdrop": 0.1})
    assert m.cfg.attn_pdrop == 0.1 if hasattr(m, "cfg") else True
    assert any(getattr(mod, "attn_pdrop", None) == 0.1 for mod in m.modules())


# ---------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------
def test_refusals():
    q, k, v, _ = ar.make_inputs("randn", 1, 2, 2, 32, 32, seed=2)
    lo = torch.zeros(32, dtype=torch.int32)
    for fn in (causal_attention, lambda *a, **kw: attention_math(*a, causal=True, **kw)):
        with pytest.raises(ValueError, match="dropout_p"):
            fn(q, k, v, dropout_p=-0.1)
        with pytest.raises(ValueError, match="dropout_p"):
            fn(q, k, v, dropout_p=1.0)
        with pytest.raises(ValueError, match="kv_lo"):
            fn(q, k, v, kv_lo=lo, dropout_p=0.1)
    with pytest.raises(ValueError, match="window"):
        causal_attention(q, k, v, window=4, dropout_p=0.1)
    with pytest.raises(ValueError, match="dropout_p"):
        full_attention(q, k, v, dropout_p=float("nan"))
    # flash_attention refuses before it looks for a device or the extension
    for kw in (dict(dropout_p=1.5), dict(dropout_p=0.1, window=4),
               dict(dropout_p=0.1, kv_lo=lo)):
        with pytest.raises(ValueError):
            flash.flash_attention(q, k, v, causal=True, **kw)
    with pytest.raises(ValueError, match="2\\^20"):
        flash.dropout_keep(0, 1 << 12, 1 << 12, 4, 0.5)
