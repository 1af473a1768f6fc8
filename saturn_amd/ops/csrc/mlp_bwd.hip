// GPT-J MLP backward: activation backward fused with the transposed stores
// and the bias gradient, so both MLP weight gradients can run as TN GEMMs.
//
// For dW[N,K] = dY^T X, storing both operands with the token dimension
// contiguous (dY^T [N,M], X^T [K,M]) turns the NT problem into
// F.linear(dY^T, X^T), the layout of the forward GEMM.  Producing the
// transposes rides on the pass the backward makes anyway:
//
//   mlp_act_bwd      reads d_act and pre once; writes d_pre = d_act*dgelu(pre)
//                    row-major, d_pre^T and gelu(pre)^T, and fp32 per-block
//                    column sums of the rounded d_pre (the fc_in bias grad).
//   transpose_colsum bf16 transpose, optionally with the same column sums
//                    (g^T + the fc_out bias grad; h^T without a sum).
//
// Tiling: one block walks ROW_ITERS 64x64 tiles down the rows.  Lane
// (rp, cv) loads rows 2rp, 2rp+1 x columns 8cv..8cv+7 as 16-B vectors and
// writes each column's row pair as one dword into a transposed LDS image:
// 64 image rows (one per source column) of 128 B (the 64 source rows).  The
// 16-B slot s of image row c is stored at slot s ^ (c >> 3), which makes the
// dword writes (a half-wave covers 8 cv x 4 rp) and the ds_read_b128 of the
// store phase (a wave covers 8 image rows of one c >> 3) hit every bank once.
// The store phase writes full 128-B runs along M.  Column sums come from the
// same LDS reads, are kept in registers over the block's tiles and leave as
// one partial row per block; at::sum reduces the partial rows (the
// layernorm.hip scheme: no atomics, deterministic).
//
// Rows and columns past the edge are staged as zeros, so ragged tiles need
// no masking in the sums; M % 8 == 0 and N % 8 == 0 keep every 16-B vector
// whole.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "ops.h"
#include "gelu_math.h"
#include "tile_image.h"

namespace samd {

namespace {

// TN_IN: store d_pre^T.  TN_OUT: store gelu(pre)^T into `act`, else store
// gelu(pre) row-major there (the NT weight gradient reads it that way).
template <bool TN_IN, bool TN_OUT>
__global__ void __launch_bounds__(MB_BLOCK)
mlp_act_bwd_kernel(const bf16_t* __restrict__ d_act,
                   const bf16_t* __restrict__ pre, bf16_t* __restrict__ d_pre,
                   bf16_t* __restrict__ d_preT, bf16_t* __restrict__ act,
                   float* __restrict__ partial, long M, long F) {
  __shared__ uint4 img_d[MB_TILE * 8];
  __shared__ uint4 img_a[TN_OUT ? MB_TILE * 8 : 1];
  __shared__ float4 lds_sum[MB_TILE / 4];

  const int tid = threadIdx.x;
  const int cv = tid & 7;   // load phase: 16-B column vector of the tile
  const int rp = tid >> 3;  // load phase: row pair of the tile
  const int mv = tid & 7;   // store phase: 16-B vector along M
  const int cr = tid >> 3;  // store phase: image row (and cr + 32)
  const long col0 = (long)blockIdx.x * MB_TILE;
  const long col = col0 + cv * 8;
  const bool col_ok = col < F;

  float acc0 = 0.f, acc1 = 0.f;

  for (int it = 0; it < MB_ROW_ITERS; ++it) {
    const long row0 = ((long)blockIdx.y * MB_ROW_ITERS + it) * MB_TILE;
    if (row0 >= M) break;  // block-uniform
    const long row = row0 + 2 * rp;
    const bool ok = col_ok && row < M;  // M is even: row + 1 < M as well

    const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    short8v xv[2], gv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (ok) {
        const long o = (row + i) * F + col;
        xv[i] = *reinterpret_cast<const short8v*>(pre + o);
        gv[i] = *reinterpret_cast<const short8v*>(d_act + o);
      } else {
        xv[i] = zero8;
        gv[i] = zero8;
      }
    }
    short8v dv[2], av[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t xe, de;
        xe.x = (unsigned short)xv[i][e];
        de.x = (unsigned short)gv[i][e];
        const float xf = toF<bf16_t>(xe);
        dv[i][e] = (short)fromF<bf16_t>(toF<bf16_t>(de) * dgelu_f(xf)).x;
        av[i][e] = (short)fromF<bf16_t>(gelu_f(xf)).x;
      }
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long o = (row + i) * F + col;
        *reinterpret_cast<short8v*>(d_pre + o) = dv[i];
        if (!TN_OUT) *reinterpret_cast<short8v*>(act + o) = av[i];
      }
    }
    unsigned* d32 = reinterpret_cast<unsigned*>(img_d);
    unsigned* a32 = reinterpret_cast<unsigned*>(img_a);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int w = img_dword(cv * 8 + e, rp);
      d32[w] = ok ? ((unsigned)(unsigned short)dv[0][e] |
                     ((unsigned)(unsigned short)dv[1][e] << 16))
                  : 0u;
      if (TN_OUT)
        a32[w] = ok ? ((unsigned)(unsigned short)av[0][e] |
                       ((unsigned)(unsigned short)av[1][e] << 16))
                    : 0u;
    }
    __syncthreads();

    const long mrow = row0 + mv * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = cr + 32 * j;
      const uint4 d = img_d[img_slot(c, mv)];
      const float s = sum8_bf16(d);
      if (j == 0) acc0 += s; else acc1 += s;
      const bool st = (col0 + c < F) && (mrow < M);
      if (TN_IN && st)
        *reinterpret_cast<uint4*>(d_preT + (col0 + c) * M + mrow) = d;
      if (TN_OUT && st)
        *reinterpret_cast<uint4*>(act + (col0 + c) * M + mrow) =
            img_a[img_slot(c, mv)];
    }
    __syncthreads();
  }
  store_colsums(acc0, acc1, lds_sum, partial, col0, F);
}

// STORE=false keeps only the column sums (a bias grad whose weight grad
// stays NT needs no transposed operand).
template <bool SUM, bool STORE>
__global__ void __launch_bounds__(MB_BLOCK)
transpose_colsum_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ xT,
                        float* __restrict__ partial, long M, long N) {
  __shared__ uint4 img[MB_TILE * 8];
  __shared__ float4 lds_sum[MB_TILE / 4];

  const int tid = threadIdx.x;
  const int cv = tid & 7;
  const int rp = tid >> 3;
  const int mv = tid & 7;
  const int cr = tid >> 3;
  const long col0 = (long)blockIdx.x * MB_TILE;
  const long col = col0 + cv * 8;
  const bool col_ok = col < N;

  float acc0 = 0.f, acc1 = 0.f;

  for (int it = 0; it < MB_ROW_ITERS; ++it) {
    const long row0 = ((long)blockIdx.y * MB_ROW_ITERS + it) * MB_TILE;
    if (row0 >= M) break;  // block-uniform
    const long row = row0 + 2 * rp;
    const bool ok = col_ok && row < M;

    const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    short8v xv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      xv[i] = zero8;
      if (ok) xv[i] = *reinterpret_cast<const short8v*>(x + (row + i) * N + col);
    }
    unsigned* i32 = reinterpret_cast<unsigned*>(img);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      i32[img_dword(cv * 8 + e, rp)] =
          (unsigned)(unsigned short)xv[0][e] |
          ((unsigned)(unsigned short)xv[1][e] << 16);
    }
    __syncthreads();

    const long mrow = row0 + mv * 8;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c = cr + 32 * j;
      const uint4 v = img[img_slot(c, mv)];
      if (SUM) {
        const float s = sum8_bf16(v);
        if (j == 0) acc0 += s; else acc1 += s;
      }
      if (STORE && (col0 + c < N) && (mrow < M))
        *reinterpret_cast<uint4*>(xT + (col0 + c) * M + mrow) = v;
    }
    __syncthreads();
  }
  if (SUM) store_colsums(acc0, acc1, lds_sum, partial, col0, N);
}

}  // namespace

// Returns (d_pre[M,F], d_preT[F,M], actT[F,M], db[F] fp32).  With
// want_dT=false d_preT is an empty tensor; with want_aT=false the third
// result is gelu(pre) row-major [M,F] instead of its transpose.
std::vector<at::Tensor> mlp_act_bwd(at::Tensor d_act, at::Tensor pre,
                                    bool want_dT, bool want_aT) {
  check_operand(d_act, "mlp_act_bwd d_act");
  check_operand(pre, "mlp_act_bwd pre");
  TORCH_CHECK(d_act.sizes() == pre.sizes(), "mlp_act_bwd: shape mismatch");
  const long M = pre.size(0), F = pre.size(1);
  auto d_pre = at::empty_like(pre);
  auto d_preT = want_dT ? at::empty({F, M}, pre.options())
                        : at::empty({0}, pre.options());
  auto act = want_aT ? at::empty({F, M}, pre.options()) : at::empty_like(pre);
  const dim3 grid = tile_grid(M, F);
  auto partial =
      at::empty({(long)grid.y, F}, pre.options().dtype(at::kFloat));
  auto stream = at::hip::getCurrentHIPStream();
#define SAMD_LAUNCH_ACT_BWD(TI, TO)                                        \
  hipLaunchKernelGGL((mlp_act_bwd_kernel<TI, TO>), grid, dim3(MB_BLOCK), 0, \
                     stream.stream(), bptr(d_act), bptr(pre), bptr(d_pre),  \
                     want_dT ? bptr(d_preT) : nullptr, bptr(act),           \
                     partial.data_ptr<float>(), M, F)
  if (want_dT && want_aT) SAMD_LAUNCH_ACT_BWD(true, true);
  else if (want_dT) SAMD_LAUNCH_ACT_BWD(true, false);
  else if (want_aT) SAMD_LAUNCH_ACT_BWD(false, true);
  else SAMD_LAUNCH_ACT_BWD(false, false);
#undef SAMD_LAUNCH_ACT_BWD
  SAMD_CHECK_HIP(hipGetLastError());
  return {d_pre, d_preT, act, at::sum(partial, {0})};
}

// Declared in tile_image.h.  want_store=false returns an empty xT;
// want_sum=false an empty colsum; `dst` takes the transpose instead of a
// fresh tensor.
std::vector<at::Tensor> transpose_colsum_impl(
    const at::Tensor& x, bool want_sum, bool want_store,
    const c10::optional<at::Tensor>& dst) {
  check_operand(x, "transpose_colsum x");
  TORCH_CHECK(want_sum || want_store, "transpose_colsum: nothing to do");
  const long M = x.size(0), N = x.size(1);
  at::Tensor xT;
  if (want_store && dst.has_value()) {
    xT = *dst;
    check_operand(xT, "transpose_colsum dst");
    TORCH_CHECK(xT.size(0) == N && xT.size(1) == M &&
                    xT.device() == x.device(),
                "transpose_colsum: dst must be [", N, ", ", M, "], got ",
                xT.sizes());
  } else {
    xT = want_store ? at::empty({N, M}, x.options())
                    : at::empty({0}, x.options());
  }
  const dim3 grid = tile_grid(M, N);
  const auto fopt = x.options().dtype(at::kFloat);
  auto partial = want_sum ? at::empty({(long)grid.y, N}, fopt)
                          : at::empty({0}, fopt);
  auto stream = at::hip::getCurrentHIPStream();
#define SAMD_LAUNCH_TRANSPOSE(SUM, STORE)                                    \
  hipLaunchKernelGGL((transpose_colsum_kernel<SUM, STORE>), grid,            \
                     dim3(MB_BLOCK), 0, stream.stream(), bptr(x),            \
                     want_store ? bptr(xT) : nullptr,                        \
                     want_sum ? partial.data_ptr<float>() : nullptr, M, N)
  if (want_sum && want_store) SAMD_LAUNCH_TRANSPOSE(true, true);
  else if (want_sum) SAMD_LAUNCH_TRANSPOSE(true, false);
  else SAMD_LAUNCH_TRANSPOSE(false, true);
#undef SAMD_LAUNCH_TRANSPOSE
  SAMD_CHECK_HIP(hipGetLastError());
  return {xT, want_sum ? at::sum(partial, {0}) : partial};
}

// Returns (xT[N,M], colsum[N] fp32); colsum is empty without want_sum.
std::vector<at::Tensor> transpose_colsum(at::Tensor x, bool want_sum) {
  return transpose_colsum_impl(x, want_sum, true);
}

// x^T into `dst`, a contiguous [N, M] view such as a row slice of a larger
// [*, M] buffer.
void transpose_into(at::Tensor x, at::Tensor dst) {
  transpose_colsum_impl(x, false, true, dst);
}

// Whole MLP backward for out = fc_out(gelu(fc_in(h))):
//   g[M,E] = d out, h[M,E], pre[M,F] = fc_in(h), W_in[F,E], W_out[E,F].
// Returns (dh, dW_in, db_in, dW_out, db_out); the bias grads are summed in
// fp32 and rounded once to the weights' dtype.  use_tn_in / use_tn_out pick
// the TN route per weight gradient; a site whose flag is off keeps the NT
// call dY.t() @ X.
std::vector<at::Tensor> mlp_bwd(at::Tensor g, at::Tensor h, at::Tensor pre,
                                at::Tensor W_in, at::Tensor W_out,
                                bool use_tn_in, bool use_tn_out) {
  check_operand(g, "mlp_bwd g");
  check_operand(h, "mlp_bwd h");
  check_operand(pre, "mlp_bwd pre");
  check_operand(W_in, "mlp_bwd W_in");
  check_operand(W_out, "mlp_bwd W_out");
  const long M = g.size(0), E = g.size(1), F = pre.size(1);
  TORCH_CHECK(h.size(0) == M && h.size(1) == E && pre.size(0) == M &&
                  W_in.size(0) == F && W_in.size(1) == E &&
                  W_out.size(0) == E && W_out.size(1) == F,
              "mlp_bwd: inconsistent shapes");

  at::Tensor d_pre, d_preT, act, db_in;
  {
    auto d_act = at::mm(g, W_out);
    auto r = mlp_act_bwd(d_act, pre, use_tn_in, use_tn_out);
    d_pre = r[0];
    d_preT = r[1];
    act = r[2];  // [F,M] when use_tn_out, else [M,F]
    db_in = r[3];
  }
  // g^T rides with the fc_out bias grad; without the TN route only the sum
  auto gt = transpose_colsum_impl(g, true, use_tn_out);
  at::Tensor hT;
  if (use_tn_in) hT = transpose_colsum_impl(h, false, true)[0];
  auto dW_out = use_tn_out ? at::linear(gt[0], act) : at::mm(g.t(), act);
  act.reset();
  auto dW_in = use_tn_in ? at::linear(d_preT, hT) : at::mm(d_pre.t(), h);
  d_preT.reset();
  hT.reset();
  auto dh = at::mm(d_pre, W_in);
  return {dh, dW_in, db_in.to(W_in.scalar_type()), dW_out,
          gt[1].to(W_out.scalar_type())};
}

}  // namespace samd
