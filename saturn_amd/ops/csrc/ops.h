// Entry points of saturn_amd._C: declared once, for bindings.cpp and for
// every .hip that defines or calls one of them.
#pragma once

#include <torch/extension.h>

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace samd {

// fused_optim.hip
void fused_sgd(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> moms, std::vector<at::Tensor> masters,
               double lr, double momentum, double weight_decay,
               c10::optional<at::Tensor> grad_scale);
void fused_adam(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                std::vector<at::Tensor> masters, double lr, double beta1,
                double beta2, double eps, double weight_decay, double bc1,
                double bc2, c10::optional<at::Tensor> grad_scale);

// grad_norm.hip
at::Tensor grad_sqsum(std::vector<at::Tensor> tensors, at::Tensor partials);
std::vector<std::pair<int64_t, int64_t>> grad_sqsum_plan(
    std::vector<int64_t> numels);
int64_t grad_sqsum_slots(int64_t n_tensors);
void clip_coef(at::Tensor sq, double max_norm, at::Tensor out);

// layernorm.hip
std::vector<at::Tensor> norm_fwd(at::Tensor x, at::Tensor w,
                                 c10::optional<at::Tensor> b, double eps,
                                 bool rms);
std::vector<at::Tensor> norm_bwd(at::Tensor dy, at::Tensor x, at::Tensor w,
                                 at::Tensor mean, at::Tensor rstd, bool rms,
                                 bool needs_db);

// cross_entropy.hip
std::vector<at::Tensor> ce_fwd(at::Tensor logits, at::Tensor targets,
                               int64_t Tr, int64_t ignore_index);
at::Tensor ce_bwd(at::Tensor logits, at::Tensor targets, at::Tensor lse,
                  at::Tensor dloss, int64_t Tr, int64_t ignore_index);

// rope.hip
void rope_apply(at::Tensor y, at::Tensor x, at::Tensor cos_t, at::Tensor sin_t,
                int64_t t_len, int64_t t_off, bool half_style, bool backward);

// gelu.hip
at::Tensor gelu_fwd(at::Tensor x);
at::Tensor gelu_bwd(at::Tensor dy, at::Tensor x);

// attention.hip
std::vector<at::Tensor> attn_fwd(at::Tensor q, at::Tensor k, at::Tensor v,
                                 bool causal, int64_t kv_len,
                                 c10::optional<at::Tensor> kv_lo,
                                 double dropout_p = 0.0, int64_t seed = 0);
std::vector<at::Tensor> attn_bwd(at::Tensor dout, at::Tensor q, at::Tensor k,
                                 at::Tensor v, at::Tensor o, at::Tensor lse,
                                 bool causal, int64_t kv_len,
                                 c10::optional<at::Tensor> kv_lo,
                                 double dropout_p = 0.0, int64_t seed = 0);
std::string attn_dispatch(int64_t T, int64_t D, bool has_lo = false,
                          bool has_drop = false);

// add3.hip, swiglu.hip, embedding.hip, dropout.hip
at::Tensor add3(at::Tensor a, at::Tensor b, at::Tensor c);
at::Tensor swiglu_fwd(at::Tensor gate, at::Tensor up);
std::vector<at::Tensor> swiglu_bwd(at::Tensor dout, at::Tensor gate,
                                   at::Tensor up);
at::Tensor embed_fwd(at::Tensor weight, at::Tensor idx);
at::Tensor embed_bwd(at::Tensor dout, at::Tensor idx, long vocab);
at::Tensor dropout_fwd(at::Tensor x, double p, long seed);
at::Tensor dropout_bwd(at::Tensor dout, double p, long seed);

// moe.hip
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

// mlp_bwd.hip
std::vector<at::Tensor> mlp_act_bwd(at::Tensor d_act, at::Tensor pre,
                                    bool want_dT, bool want_aT);
std::vector<at::Tensor> transpose_colsum(at::Tensor x, bool want_sum);
std::vector<at::Tensor> mlp_bwd(at::Tensor g, at::Tensor h, at::Tensor pre,
                                at::Tensor W_in, at::Tensor W_out,
                                bool use_tn_in, bool use_tn_out);
void transpose_into(at::Tensor x, at::Tensor dst);

// gptj_block_bwd.hip
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
