// GPT-J parallel block backward: attention and MLP branches as one unit.
//
// The block computes x + attn(h) + mlp(h), so both branches receive the same
// incoming gradient g and read the same input h.  Treated together,
//
//   g^T  (out_proj and fc_out share dY = g) and
//   h^T  (q/k/v_proj and fc_in share X = h)
//
// are produced once, and the four attention weight gradients can run as TN
// GEMMs F.linear(dY^T, X^T) like the MLP's (mlp_bwd.hip).  The Q, K and V
// gradients share h^T, so their transposed dY are written into the row
// slices of one [3E, M] buffer and one GEMM gives [dWq; dWk; dWv]:
//
//   rope_bwd_t   the RoPE backward (the inverse rotation of rope.hip's
//                interleaved vector kernel), which besides dx row-major also
//                stores dx^T into a caller-given [E, M] slice.  It rides on
//                the elementwise pass the backward makes anyway and uses the
//                tile image of tile_image.h.
//   dV           goes into its slice through transpose_colsum_impl.
//
// The gradient of h is the sum of four GEMMs, added in autograd's order so
// that it keeps the unfused path's bits; dh_accum lets the last three
// accumulate into the first with addmm (beta = 1) instead of three
// elementwise adds, at one rounding fewer per term.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "ops.h"
#include "tile_image.h"

namespace samd {

namespace {

// dy viewed as [M, E], E = heads * dim; column c is element c % dim of head
// c / dim, and dim % 8 == 0 keeps each 16-B vector inside one head.  The
// rotation is rope_oop_vec_kernel<bf16, false> with the same operand order,
// so every element rounds as it does there.
__global__ void __launch_bounds__(MB_BLOCK)
rope_bwd_t_kernel(const bf16_t* __restrict__ dy, bf16_t* __restrict__ dx,
                  bf16_t* __restrict__ dxT, const float* __restrict__ cos_t,
                  const float* __restrict__ sin_t, long M, long E, int t_len,
                  long t_off, int dim, int half, float sign) {
  __shared__ uint4 img[MB_TILE * 8];

  const int tid = threadIdx.x;
  const int cv = tid & 7;   // load phase: 16-B column vector of the tile
  const int rp = tid >> 3;  // load phase: row pair of the tile
  const int mv = tid & 7;   // store phase: 16-B vector along M
  const int cr = tid >> 3;  // store phase: image row (and cr + 32)
  const long col0 = (long)blockIdx.x * MB_TILE;
  const long col = col0 + cv * 8;
  const bool col_ok = col < E;
  const int j0 = (int)(col % dim);
  const bool rotary = j0 < 2 * half;  // else the copied tail of the head

  for (int it = 0; it < MB_ROW_ITERS; ++it) {
    const long row0 = ((long)blockIdx.y * MB_ROW_ITERS + it) * MB_TILE;
    if (row0 >= M) break;  // block-uniform
    const long row = row0 + 2 * rp;
    const bool ok = col_ok && row < M;  // M is even: row + 1 < M as well

    const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    short8v ov[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      ov[i] = zero8;
      if (!ok) continue;
      const short8v xv =
          *reinterpret_cast<const short8v*>(dy + (row + i) * E + col);
      if (rotary) {
        const long trow = (t_off + ((row + i) % t_len)) * (long)half;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int p = j0 / 2 + e;
          const float c = cos_t[trow + p];
          const float s = sin_t[trow + p] * sign;
          bf16_t e0, e1;
          e0.x = (unsigned short)xv[2 * e];
          e1.x = (unsigned short)xv[2 * e + 1];
          const float x0 = toF<bf16_t>(e0);
          const float x1 = toF<bf16_t>(e1);
          ov[i][2 * e] = (short)fromF<bf16_t>(x0 * c - x1 * s).x;
          ov[i][2 * e + 1] = (short)fromF<bf16_t>(x1 * c + x0 * s).x;
        }
      } else {
        ov[i] = xv;
      }
      *reinterpret_cast<short8v*>(dx + (row + i) * E + col) = ov[i];
    }
    unsigned* i32 = reinterpret_cast<unsigned*>(img);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      i32[img_dword(cv * 8 + e, rp)] =
          (unsigned)(unsigned short)ov[0][e] |
          ((unsigned)(unsigned short)ov[1][e] << 16);
    }
    __syncthreads();

    const long mrow = row0 + mv * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = cr + 32 * j;
      if ((col0 + c < E) && (mrow < M))
        *reinterpret_cast<uint4*>(dxT + (col0 + c) * M + mrow) =
            img[img_slot(c, mv)];
    }
    __syncthreads();
  }
}

void check_f32_table(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.dim() == 2 &&
                  t.is_contiguous(),
              name, ": expected a contiguous fp32 [T, half] GPU tensor");
}

}  // namespace

// RoPE backward (interleaved pairs) of dy [..., heads, dim], flattened to
// [M, E]: returns dx shaped like dy and stores dx^T into dxT, a contiguous
// [E, M] view (a row slice of a [*, M] buffer).  Table row of token m is
// t_off + m % t_len.
at::Tensor rope_bwd_t(at::Tensor dy, at::Tensor cos_t, at::Tensor sin_t,
                      int64_t t_len, int64_t t_off, int64_t dim,
                      at::Tensor dxT) {
  TORCH_CHECK(dy.is_cuda() && dy.scalar_type() == at::kBFloat16 &&
                  dy.is_contiguous() && dy.numel() > 0,
              "rope_bwd_t dy: expected a contiguous bf16 GPU tensor");
  check_f32_table(cos_t, "rope_bwd_t cos");
  check_f32_table(sin_t, "rope_bwd_t sin");
  const long half = cos_t.size(1);
  TORCH_CHECK(sin_t.sizes() == cos_t.sizes(), "rope_bwd_t: table mismatch");
  TORCH_CHECK(dim > 0 && dim % 8 == 0, "rope_bwd_t: head dim ", dim,
              " must be a positive multiple of 8");
  TORCH_CHECK((2 * half) % 8 == 0 && 2 * half <= dim,
              "rope_bwd_t: rotary dim ", 2 * half,
              " must be a multiple of 8 within the head dim");
  TORCH_CHECK(dy.numel() % dim == 0 && dy.size(-1) == dim,
              "rope_bwd_t: last dim of dy must be the head dim");
  TORCH_CHECK(dy.dim() >= 2, "rope_bwd_t dy: expected [..., heads, dim]");
  const long E = dy.size(-2) * dim;
  const long M = dy.numel() / E;
  TORCH_CHECK(M % 8 == 0, "rope_bwd_t: token count ", M,
              " must be a multiple of 8");
  TORCH_CHECK(t_len > 0 && M % t_len == 0,
              "rope_bwd_t: token count not a multiple of T");
  TORCH_CHECK(t_off >= 0 && cos_t.size(0) >= t_off + t_len,
              "rope_bwd_t: table too short for offset+T");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(dy.data_ptr()) % 16 == 0,
              "rope_bwd_t dy: data must be 16-byte aligned");
  check_operand(dxT, "rope_bwd_t dxT");
  TORCH_CHECK(dxT.size(0) == E && dxT.size(1) == M &&
                  dxT.device() == dy.device(),
              "rope_bwd_t: dxT must be [", E, ", ", M, "], got ", dxT.sizes());

  auto dx = at::empty_like(dy);
  const dim3 grid = tile_grid(M, E);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(rope_bwd_t_kernel, grid, dim3(MB_BLOCK), 0,
                     stream.stream(), bptr(dy), bptr(dx), bptr(dxT),
                     cos_t.data_ptr<float>(), sin_t.data_ptr<float>(), M, E,
                     (int)t_len, (long)t_off, (int)dim, (int)half, -1.f);
  SAMD_CHECK_HIP(hipGetLastError());
  return dx;
}

// Backward of  attn_out = out_proj(attn(rope(q_proj h), rope(k_proj h),
// v_proj h)),  mlp_out = fc_out(gelu(fc_in h)).
//   g_a, g_m [M,E]   gradients of the two outputs; when they are one tensor
//                    (the block's add3 hands the same g to both) g^T is
//                    shared between out_proj and fc_out
//   h [M,E], pre [M,F]; q, k (rotated), v, o [B,H,T,D] as attn_fwd took and
//   gave them; lse [B,H,T]; cos/sin fp32 [T_total, half]
// Returns (dh, dWq, dWk, dWv, dWo, dW_in, db_in, dW_out, db_out).  Per-site
// flags: tn_in/tn_out as in mlp_bwd; tn_qkv one TN GEMM for the three
// projections, tn_o TN for out_proj, dh_accum addmm accumulation into dh.  A
// site whose flag is off keeps the NT call dY.t() @ X and its transposed
// operands are not produced.
std::vector<at::Tensor> gptj_branches_bwd(
    at::Tensor g_a, at::Tensor g_m, at::Tensor h, at::Tensor pre, at::Tensor q,
    at::Tensor k, at::Tensor v, at::Tensor o, at::Tensor lse, at::Tensor Wq,
    at::Tensor Wk, at::Tensor Wv, at::Tensor Wo, at::Tensor W_in,
    at::Tensor W_out, at::Tensor cos_t, at::Tensor sin_t, int64_t t_off,
    bool tn_in, bool tn_out, bool tn_qkv, bool tn_o, bool dh_accum) {
  check_operand(g_a, "gptj_branches_bwd g_a");
  check_operand(g_m, "gptj_branches_bwd g_m");
  check_operand(h, "gptj_branches_bwd h");
  check_operand(pre, "gptj_branches_bwd pre");
  check_operand(W_in, "gptj_branches_bwd W_in");
  check_operand(W_out, "gptj_branches_bwd W_out");
  const long M = h.size(0), E = h.size(1), F = pre.size(1);
  TORCH_CHECK(q.dim() == 4 && o.dim() == 4, "gptj_branches_bwd: q, o 4-D");
  const long B = q.size(0), H = q.size(1), T = q.size(2), D = q.size(3);
  TORCH_CHECK(B * T == M && H * D == E && k.sizes() == q.sizes() &&
                  v.sizes() == q.sizes() && o.sizes() == q.sizes(),
              "gptj_branches_bwd: attention shapes do not match h");
  TORCH_CHECK(g_a.sizes() == h.sizes() && g_m.sizes() == h.sizes() &&
                  pre.size(0) == M && W_in.size(0) == F && W_in.size(1) == E &&
                  W_out.size(0) == E && W_out.size(1) == F,
              "gptj_branches_bwd: inconsistent shapes");
  for (const at::Tensor* w : {&Wq, &Wk, &Wv, &Wo}) {
    check_operand(*w, "gptj_branches_bwd projection weight");
    TORCH_CHECK(w->size(0) == E && w->size(1) == E,
                "gptj_branches_bwd: projection weights must be [E, E]");
  }
  // o as [M, E]: attn_fwd lays it out [B,T,H,D]
  auto o_phys = o.permute({0, 2, 1, 3});
  TORCH_CHECK(o_phys.is_contiguous(),
              "gptj_branches_bwd: o must be physically [B,T,H,D]");
  auto o2 = o_phys.view({M, E});
  const bool shared = g_a.data_ptr() == g_m.data_ptr();

  // ---- shared transposes
  auto gt = transpose_colsum_impl(g_m, true, tn_out || (shared && tn_o));
  at::Tensor gaT;
  if (tn_o) gaT = shared ? gt[0] : transpose_colsum_impl(g_a, false, true)[0];
  at::Tensor hT;
  if (tn_in || tn_qkv) hT = transpose_colsum_impl(h, false, true)[0];

  // ---- MLP branch, as mlp_bwd
  at::Tensor dh, dW_in, db_in, dW_out;
  {
    at::Tensor d_pre, d_preT, act;
    {
      auto d_act = at::mm(g_m, W_out);
      auto r = mlp_act_bwd(d_act, pre, tn_in, tn_out);
      d_pre = r[0];
      d_preT = r[1];
      act = r[2];  // [F,M] when tn_out, else [M,F]
      db_in = r[3];
    }
    dW_out = tn_out ? at::linear(gt[0], act) : at::mm(g_m.t(), act);
    act.reset();
    if (!tn_o) gt[0].reset();
    dW_in = tn_in ? at::linear(d_preT, hT) : at::mm(d_pre.t(), h);
    d_preT.reset();
    if (!tn_qkv) hT.reset();
    dh = at::mm(d_pre, W_in);
  }

  // ---- out_proj
  auto d_o = at::mm(g_a, Wo);
  at::Tensor dWo;
  if (tn_o) {
    auto oT = transpose_colsum_impl(o2, false, true)[0];
    dWo = at::linear(gaT, oT);
    gaT.reset();
    gt[0].reset();
  } else {
    dWo = at::mm(g_a.t(), o2);
  }

  // ---- attention core; gradients come back physically [B,T,H,D]
  at::Tensor dq_r, dk_r, dv;
  {
    auto r = attn_bwd(d_o.view({B, T, H, D}).permute({0, 2, 1, 3}), q, k, v, o,
                      lse, true, T, c10::nullopt);
    dq_r = r[0].permute({0, 2, 1, 3});
    dk_r = r[1].permute({0, 2, 1, 3});
    dv = r[2].permute({0, 2, 1, 3});
    TORCH_CHECK(dq_r.is_contiguous() && dk_r.is_contiguous() &&
                    dv.is_contiguous(),
                "gptj_branches_bwd: attn_bwd layout changed");
  }
  d_o.reset();
  auto dv2 = dv.view({M, E});

  // ---- RoPE backward and the q/k/v weight gradients
  at::Tensor dq, dk, dWq, dWk, dWv;
  if (tn_qkv) {
    auto dqkvT = at::empty({3 * E, M}, h.options());
    dq = rope_bwd_t(dq_r, cos_t, sin_t, T, t_off, D, dqkvT.narrow(0, 0, E));
    dq_r.reset();
    dk = rope_bwd_t(dk_r, cos_t, sin_t, T, t_off, D, dqkvT.narrow(0, E, E));
    dk_r.reset();
    transpose_colsum_impl(dv2, false, true, dqkvT.narrow(0, 2 * E, E));
    auto dW = at::linear(dqkvT, hT);  // [3E, E]
    dqkvT.reset();
    hT.reset();
    dWq = dW.narrow(0, 0, E);
    dWk = dW.narrow(0, E, E);
    dWv = dW.narrow(0, 2 * E, E);
  } else {
    dq = at::empty_like(dq_r);
    rope_apply(dq, dq_r, cos_t, sin_t, T, t_off, false, true);
    dq_r.reset();
    dk = at::empty_like(dk_r);
    rope_apply(dk, dk_r, cos_t, sin_t, T, t_off, false, true);
    dk_r.reset();
    dWq = at::mm(dq.view({M, E}).t(), h);
    dWk = at::mm(dk.view({M, E}).t(), h);
    dWv = at::mm(dv2.t(), h);
  }

  // ---- dh = ((d_pre W_in + dv Wv) + dk Wk) + dq Wq: the order in which
  // autograd sums the four gradients of h on the unfused path (fc_in's node
  // runs first, then the projections' in reverse order of their forward
  // calls), so that without dh_accum dh keeps its bits
  auto dq2 = dq.view({M, E}), dk2 = dk.view({M, E});
  if (dh_accum) {
    dh.addmm_(dv2, Wv);
    dh.addmm_(dk2, Wk);
    dh.addmm_(dq2, Wq);
  } else {
    dh.add_(at::mm(dv2, Wv));
    dh.add_(at::mm(dk2, Wk));
    dh.add_(at::mm(dq2, Wq));
  }
  return {dh, dWq, dWk, dWv, dWo, dW_in, db_in.to(W_in.scalar_type()),
          dW_out, gt[1].to(W_out.scalar_type())};
}

}  // namespace samd
