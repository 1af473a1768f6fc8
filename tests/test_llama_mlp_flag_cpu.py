"""LlamaConfig.fused_mlp_bwd on the CPU: the fused backward is a GPU path, so
the flag must leave the CPU model exactly as it is."""

import torch

from saturn_amd.models.llama import LlamaConfig, LlamaForCausalLM, llama_loss
from saturn_amd.ops.functional import llama_mlp_supported


def _step(fused):
    torch.manual_seed(0)
    model = LlamaForCausalLM(LlamaConfig(
        vocab_size=128, n_ctx=16, n_embd=32, n_head=4, n_kv_head=2, n_layer=2,
        ffn_dim=40, fused_mlp_bwd=fused))
    ids = torch.randint(0, 128, (2, 16), generator=torch.Generator().manual_seed(1))
    loss = llama_loss(model(ids), ids)
    loss.backward()
    return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


def test_flag_changes_nothing_on_cpu():
    loss_off, g_off = _step(False)
    loss_on, g_on = _step(True)
    assert torch.equal(loss_on, loss_off)
    assert set(g_on) == set(g_off)
    assert all(torch.equal(g_on[n], g_off[n]) for n in g_off)


def test_supported_refuses_bias_fp32_and_ragged_m():
    def args(M=16, dtype=torch.bfloat16):
        return (torch.zeros(M, 32, dtype=dtype), torch.zeros(40, 32, dtype=dtype),
                torch.zeros(40, 32, dtype=dtype), torch.zeros(32, 40, dtype=dtype))

    bias = torch.zeros(32, dtype=torch.bfloat16)
    assert not llama_mlp_supported(*args(), b_down=bias)
    assert not llama_mlp_supported(*args(dtype=torch.float32))
    assert not llama_mlp_supported(*args(M=12))
