// saturn_amd._C: pybind entry for the hand-written CDNA4 kernels.

#include "ops.h"

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "saturn_amd hand-written CDNA4 (gfx950) kernels";
  m.def("fused_sgd", &samd::fused_sgd, "fused multi-tensor SGD",
        py::arg("params"), py::arg("grads"), py::arg("moms"),
        py::arg("masters"), py::arg("lr"), py::arg("momentum"),
        py::arg("weight_decay"), py::arg("grad_scale") = py::none());
  m.def("fused_adam", &samd::fused_adam, "fused multi-tensor AdamW",
        py::arg("params"), py::arg("grads"), py::arg("ms"), py::arg("vs"),
        py::arg("masters"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("weight_decay"),
        py::arg("bc1"), py::arg("bc2"), py::arg("grad_scale") = py::none());
  m.def("grad_sqsum", &samd::grad_sqsum,
        "fp32 sum of squares over a tensor list (no atomics, reproducible)",
        py::arg("tensors"), py::arg("partials"));
  m.def("grad_sqsum_plan", &samd::grad_sqsum_plan,
        "(blocks, threads) of each launch grad_sqsum makes for these sizes",
        py::arg("numels"));
  m.def("grad_sqsum_slots", &samd::grad_sqsum_slots,
        "partials slots a list of n tensors can need (launches x grid cap)",
        py::arg("n_tensors"));
  m.def("clip_coef", &samd::clip_coef,
        "out = {norm, coef, skipped_total} from a squared gradient sum",
        py::arg("sq"), py::arg("max_norm"), py::arg("out"));
  m.def("norm_fwd", &samd::norm_fwd, "LayerNorm/RMSNorm forward");
  m.def("norm_bwd", &samd::norm_bwd, "LayerNorm/RMSNorm backward");
  m.def("ce_fwd", &samd::ce_fwd, "fused cross-entropy forward");
  m.def("ce_bwd", &samd::ce_bwd, "fused cross-entropy backward");
  m.def("rope_apply", &samd::rope_apply,
        "fused rotary embedding (out-of-place, offset table rows)");
  m.def("gelu_fwd", &samd::gelu_fwd, "fused tanh-approx GELU forward");
  m.def("gelu_bwd", &samd::gelu_bwd, "fused tanh-approx GELU backward");
  m.def("attn_fwd", &samd::attn_fwd, "fused flash attention forward",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("causal"),
        py::arg("kv_len") = -1, py::arg("kv_lo") = py::none(),
        py::arg("dropout_p") = 0.0, py::arg("seed") = 0);
  m.def("attn_dispatch", &samd::attn_dispatch,
        "kernel instantiations attn_fwd/attn_bwd launch for (padded T, D)",
        py::arg("T"), py::arg("D"), py::arg("has_lo") = false,
        py::arg("has_drop") = false);
  m.def("attn_bwd", &samd::attn_bwd, "fused flash attention backward",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("causal"),
        py::arg("kv_len") = -1, py::arg("kv_lo") = py::none(),
        py::arg("dropout_p") = 0.0, py::arg("seed") = 0);
  m.def("add3", &samd::add3, "fused 3-way residual add");
  m.def("swiglu_fwd", &samd::swiglu_fwd, "fused silu(gate)*up");
  m.def("swiglu_bwd", &samd::swiglu_bwd, "fused SwiGLU backward");
  m.def("embed_fwd", &samd::embed_fwd, "token embedding gather");
  m.def("embed_bwd", &samd::embed_bwd, "embedding scatter-add backward");
  m.def("dropout_fwd", &samd::dropout_fwd, "counter-based fused dropout");
  m.def("dropout_bwd", &samd::dropout_bwd, "dropout backward (mask recompute)");
  m.def("moe_route_fwd", &samd::moe_route_fwd,
        "MoE softmax + top-k + renormalise (ties to the lower expert)");
  m.def("moe_route_bwd", &samd::moe_route_bwd, "MoE routing backward");
  m.def("moe_sort", &samd::moe_sort,
        "stable counting sort of (token, slot) pairs by expert");
  m.def("moe_permute_fwd", &samd::moe_permute_fwd,
        "gather token rows into expert order");
  m.def("moe_permute_bwd", &samd::moe_permute_bwd,
        "sum each token's k permuted rows");
  m.def("moe_combine_fwd", &samd::moe_combine_fwd,
        "weighted sum of each token's k expert rows");
  m.def("moe_combine_bwd", &samd::moe_combine_bwd,
        "combine backward: dy and fp32 dweights");
  m.def("mlp_act_bwd", &samd::mlp_act_bwd,
        "GELU backward + transposed d_pre / gelu(pre) + fp32 bias grad",
        py::arg("d_act"), py::arg("pre"), py::arg("want_dT") = true,
        py::arg("want_aT") = true);
  m.def("transpose_colsum", &samd::transpose_colsum,
        "bf16 transpose with optional fp32 column sums");
  m.def("mlp_bwd", &samd::mlp_bwd,
        "GPT-J MLP backward with TN-layout weight gradients");
  m.def("transpose_into", &samd::transpose_into,
        "bf16 transpose stored into a caller-given [N, M] view",
        py::arg("x"), py::arg("dst"));
  m.def("rope_bwd_t", &samd::rope_bwd_t,
        "interleaved RoPE backward that also stores dx^T into a [E, M] view",
        py::arg("dy"), py::arg("cos"), py::arg("sin"), py::arg("t_len"),
        py::arg("t_off"), py::arg("dim"), py::arg("dxT"));
  m.def("gptj_branches_bwd", &samd::gptj_branches_bwd,
        "GPT-J attention + MLP branch backward with shared transposes");
}
