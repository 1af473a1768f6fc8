// saturn_amd._C: pybind entry for the hand-written CDNA4 kernels.

#include <torch/extension.h>
#include <vector>

namespace samd {
void fused_sgd(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> moms, std::vector<at::Tensor> masters,
               double lr, double momentum, double weight_decay,
               c10::optional<at::Tensor> grad_scale);
void fused_adam(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                std::vector<at::Tensor> masters, double lr, double beta1,
                double beta2, double eps, double weight_decay, double bc1,
                double bc2, c10::optional<at::Tensor> grad_scale);
at::Tensor grad_sqsum(std::vector<at::Tensor> tensors, at::Tensor partials);
std::vector<std::pair<int64_t, int64_t>> grad_sqsum_plan(
    std::vector<int64_t> numels);
int64_t grad_sqsum_slots(int64_t n_tensors);
void clip_coef(at::Tensor sq, double max_norm, at::Tensor out);
std::vector<at::Tensor> norm_fwd(at::Tensor x, at::Tensor w,
                                 c10::optional<at::Tensor> b, double eps,
                                 bool rms);
std::vector<at::Tensor> norm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                 at::Tensor mean, at::Tensor rstd, bool rms,
                                 bool needs_db);
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor targets,
                               int64_t Tr, int64_t ignore_index);
at::Tensor ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                  at::Tensor dloss, int64_t Tr, int64_t ignore_index);
void rope_apply(at::Tensor y, at::Tensor x, at::Tensor cos_t, at::Tensor sin_t,
                int64_t t_len, int64_t t_off, bool half_style, bool backward);
at::Tensor gelu_fwd(at::Tensor x);
at::Tensor gelu_bwd(at::Tensor dy, at::Tensor x);
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 bool causal, int64_t kv_len,
                                 c10::optional<at::Tensor> kv_lo);
std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor q, at::Tensor k,
                                 at::Tensor v, at::Tensor o, at::Tensor lse,
                                 bool causal, int64_t kv_len,
                                 c10::optional<at::Tensor> kv_lo);
std::string attn_dispatch(int64_t T, int64_t D, bool has_lo);
at::Tensor add3(at::Tensor a, at::Tensor b, at::Tensor c);
at::Tensor swiglu_fwd(at::Tensor gate, at::Tensor up);
std::vector<at::Tensor> swiglu_bwd(at::Tensor dout, at::Tensor gate,
                                   at::Tensor up);
at::Tensor embed_fwd(at::Tensor weight, at::Tensor idx);
at::Tensor embed_bwd(at::Tensor dout, at::Tensor idx, long vocab);
at::Tensor dropout_fwd(at::Tensor x, double p, long seed);
at::Tensor dropout_bwd(at::Tensor dout, double p, long seed);
std::vector<at::Tensor> moe_route_fwd(at::Tensor logits, int64_t top_k,
                                      at::ScalarType out_dtype);
at::Tensor moe_route_bwd(at::Tensor logits, at::Tensor ids,
                         at::Tensor dweights);
std::vector<at::Tensor> moe_sort(at::Tensor ids, int64_t n_expert);
at::Tensor moe_permute_fwd(at::Tensor x, at::Tensor order, int64_t top_k);
at::Tensor moe_permute_bwd(at::Tensor dxs, at::Tensor pos);
at::Tensor moe_combine_fwd(at::Tensor y, at::Tensor weights, at::Tensor pos);
std::vector<at::Tensor> moe_combine_bwd(at::Tensor dout, at::Tensor y,
                                        at::Tensor weights, at::Tensor pos);
std::vector<at::Tensor> mlp_act_bwd(at::Tensor d_act, at::Tensor pre,
                                    bool want_dT, bool want_aT);
std::vector<at::Tensor> transpose_colsum(at::Tensor x, bool want_sum);
std::vector<at::Tensor> mlp_bwd(at::Tensor g, at::Tensor h, at::Tensor pre,
                                at::Tensor W_in, at::Tensor W_out,
                                bool use_tn_in, bool use_tn_out);
void transpose_into(at::Tensor x, at::Tensor dst);
at::Tensor rope_bwd_t(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t,
                      int64_t t_len, int64_t t_off, int64_t dim,
                      at::Tensor dxT);
std::vector<at::Tensor> gptj_branches_bwd(
    at::Tensor g_a, at::Tensor g_m, at::Tensor h, at::Tensor pre, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse, at::Tensor Wq,
    at::Tensor Wk, at::Tensor Wv, at::Tensor Wo, at::Tensor W_in,
    at::Tensor W_out, at::Tensor cos_t, at::Tensor sin_t, int64_t t_off,
    bool tn_in, bool tn_out, bool tn_qkv, bool tn_o, bool dh_accum);
}  // namespace samd

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
        py::arg("kv_len") = -1, py::arg("kv_lo") = py::none());
  m.def("attn_dispatch", &samd::attn_dispatch,
        "kernel instantiations attn_fwd/attn_bwd launch for (padded T, D)",
        py::arg("T"), py::arg("D"), py::arg("has_lo") = false);
  m.def("attn_bwd", &samd::attn_bwd, "fused flash attention backward",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("causal"),
        py::arg("kv_len") = -1, py::arg("kv_lo") = py::none());
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
