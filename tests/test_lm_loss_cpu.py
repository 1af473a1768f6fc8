"""fused_linear_cross_entropy, LazyLogits and the models' fused_lm_loss flag
off the GPU: the fallback is F.linear + cross-entropy."""

import pytest
import torch
import torch.nn.functional as F

from saturn_amd.ops import LazyLogits, fused_linear_cross_entropy
from saturn_amd.ops.functional import fused_cross_entropy


def _inputs(bias):
    g = torch.Generator().manual_seed(5)
    h = torch.randn(2, 9, 32, generator=g)
    w = torch.randn(37, 32, generator=g) * 0.3
    b = torch.randn(37, generator=g) if bias else None
    t = torch.randint(0, 37, (2, 9), generator=g)
    t.view(-1)[::4] = -1
    return h, w, b, t


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("shift", [True, False])
def test_fallback_is_linear_then_cross_entropy(bias, shift):
    h, w, b, t = _inputs(bias)
    got = fused_linear_cross_entropy(h, w, b, t, shift=shift, ignore_index=-1)
    lg = F.linear(h, w, b).float()
    lg, tg = (lg[:, :-1], t[:, 1:]) if shift else (lg, t)
    want = F.cross_entropy(lg.reshape(-1, 37), tg.reshape(-1), ignore_index=-1)
    assert torch.equal(got, want)
    # [N, K] hidden with [N] targets is one sequence
    one = fused_linear_cross_entropy(h[0], w, b, t[0], shift=shift,
                                     ignore_index=-1)
    assert torch.equal(one, F.cross_entropy(lg[0], tg[0], ignore_index=-1))


def test_lazy_logits_through_fused_cross_entropy():
    h, w, b, t = _inputs(True)
    lazy = LazyLogits(h, w, b)
    assert torch.equal(lazy.materialize(), F.linear(h, w, b))
    for shift in (True, False):
        assert torch.equal(
            fused_cross_entropy(lazy, t, shift=shift, ignore_index=-1),
            fused_cross_entropy(lazy.materialize(), t, shift=shift,
                                ignore_index=-1))


def test_llama_flag_same_cpu_loss():
    from saturn_amd.models.llama import (LlamaConfig, LlamaForCausalLM,
                                         llama_loss)

    tiny = dict(vocab_size=203, n_ctx=16, n_embd=64, n_head=2, n_kv_head=1,
                n_layer=2, ffn_dim=96)
    x = torch.randint(0, 203, (2, 16), generator=torch.Generator().manual_seed(2))
    torch.manual_seed(0)
    off = LlamaForCausalLM(LlamaConfig(**tiny))
    torch.manual_seed(0)
    on = LlamaForCausalLM(LlamaConfig(**tiny, fused_lm_loss=True))
    assert isinstance(on(x), LazyLogits) and isinstance(off(x), torch.Tensor)
    assert torch.equal(llama_loss(on(x), x), llama_loss(off(x), x))
    assert isinstance(on.eval()(x), torch.Tensor)
