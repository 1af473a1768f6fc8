// Llama SwiGLU MLP backward (K19): the SwiGLU backward fused with the
// transposed stores, so all three MLP weight gradients can run as TN GEMMs
// (see mlp_bwd.hip for why dW = F.linear(dY^T, X^T) is the faster layout).
//
//   swiglu_bwd_t   reads d_act, gate and up once; writes d_gate and d_up
//                  row-major (the dx GEMMs read them), [d_gate^T; d_up^T] as
//                  one [2F, M] buffer (gate_proj's and up_proj's weight
//                  gradients become one TN GEMM) and (silu(gate) up)^T, which
//                  the forward never saved.
//
// Tiling: the 64x64 tile and the transposed LDS image of tile_image.h, one
// image per transposed output.  A block walks MB_ROW_ITERS tiles down the
// rows.  Lane (rp, cv) holds rows 2rp, 2rp+1 x columns 8cv..8cv+7 of the three
// inputs (six 16-B loads), computes the three results in registers, stores
// the row-major ones as 16-B vectors and writes each column's row pair as one
// dword into the images.  After one barrier lane (cr, mv) reads image rows
// cr and cr + 32 as ds_read_b128 and stores them as full 128-B runs along M.
//
// Loads in flight: the six loads of the next tile are issued between the LDS
// writes and the barrier, into the registers the arithmetic has just
// consumed, so they are in flight across both barriers and the store phase
// and the next iteration starts on data that has arrived.
//
// LDS: the three images are live at once (24 KB with both flags on; an
// image whose flag is off is not allocated).  Reusing one image in three
// rounds would cost four more barriers per tile and serialise the three
// transposed stores; at 24 KB six blocks fit a CU's 160 KB, more than the
// four (4 waves per SIMD at 128 VGPRs) the registers allow.
//
// Rows and columns past the edge are neither read nor written (their lanes
// compute on zeros); M % 8 == 0 and F % 8 == 0 keep every 16-B vector whole.
// No atomics, no column sums (Llama has no biases), block-uniform barriers.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "ops.h"
#include "swiglu_math.h"
#include "tile_image.h"

namespace samd {

namespace {

__device__ __forceinline__ void load_row_pair(const bf16_t* __restrict__ p,
                                              long o, long ld, bool ok,
                                              short8v (&v)[2]) {
  const short8v zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    v[i] = zero8;
    if (ok) v[i] = *reinterpret_cast<const short8v*>(p + o + i * ld);
  }
}

__device__ __forceinline__ unsigned pack_pair(short lo, short hi) {
  return (unsigned)(unsigned short)lo | ((unsigned)(unsigned short)hi << 16);
}

// TN_GU: store [d_gate^T; d_up^T] into dguT.  TN_DOWN: store
// (silu(gate) up)^T into `act`, else store it row-major there (the NT weight
// gradient reads it that way).
// 4 waves per SIMD asked for: left alone the allocator takes 130 VGPRs with
// TN_GU on, two over the 128 that a fourth wave needs.
template <bool TN_GU, bool TN_DOWN>
__global__ void __launch_bounds__(MB_BLOCK, 4)
swiglu_bwd_t_kernel(const bf16_t* __restrict__ d_act,
                    const bf16_t* __restrict__ gate,
                    const bf16_t* __restrict__ up, bf16_t* __restrict__ d_gate,
                    bf16_t* __restrict__ d_up, bf16_t* __restrict__ dguT,
                    bf16_t* __restrict__ act, long M, long F) {
  __shared__ uint4 img_g[TN_GU ? MB_TILE * 8 : 1];
  __shared__ uint4 img_u[TN_GU ? MB_TILE * 8 : 1];
  __shared__ uint4 img_a[TN_DOWN ? MB_TILE * 8 : 1];

  const int tid = threadIdx.x;
  const int cv = tid & 7;   // load phase: 16-B column vector of the tile
  const int rp = tid >> 3;  // load phase: row pair of the tile
  const int mv = tid & 7;   // store phase: 16-B vector along M
  const int cr = tid >> 3;  // store phase: image row (and cr + 32)
  const long col0 = (long)blockIdx.x * MB_TILE;
  const long col = col0 + cv * 8;
  const bool col_ok = col < F;

  long row0 = (long)blockIdx.y * MB_ROW_ITERS * MB_TILE;
  // M is even: row + 1 < M whenever row < M
  bool ok = col_ok && row0 + 2 * rp < M;
  short8v gv[2], uv[2], ov[2];
  {
    const long o = (row0 + 2 * rp) * F + col;
    load_row_pair(gate, o, F, ok, gv);
    load_row_pair(up, o, F, ok, uv);
    load_row_pair(d_act, o, F, ok, ov);
  }

  for (int it = 0; it < MB_ROW_ITERS; ++it) {
    if (row0 >= M) break;  // block-uniform

    short8v dg[2], du[2], av[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float g = us2f((unsigned short)gv[i][e]);
        const float u = us2f((unsigned short)uv[i][e]);
        const float go = us2f((unsigned short)ov[i][e]);
        const float sig = sigmoid_f(g);
        dg[i][e] = (short)f2us(swiglu_dgate_f(go, g, u, sig));
        du[i][e] = (short)f2us(swiglu_dup_f(go, g, sig));
        av[i][e] = (short)f2us(silu_f(g) * u);
      }
      // one row at a time: interleaving both rows' 48 results unpacked
      // costs the registers of a fourth wave per SIMD
      __builtin_amdgcn_sched_barrier(0);
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const long o = (row0 + 2 * rp + i) * F + col;
        *reinterpret_cast<short8v*>(d_gate + o) = dg[i];
        *reinterpret_cast<short8v*>(d_up + o) = du[i];
        if (!TN_DOWN) *reinterpret_cast<short8v*>(act + o) = av[i];
      }
    }
    if (TN_GU || TN_DOWN) {
      unsigned* g32 = reinterpret_cast<unsigned*>(img_g);
      unsigned* u32 = reinterpret_cast<unsigned*>(img_u);
      unsigned* a32 = reinterpret_cast<unsigned*>(img_a);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int w = img_dword(cv * 8 + e, rp);
        if (TN_GU) {
          g32[w] = pack_pair(dg[0][e], dg[1][e]);
          u32[w] = pack_pair(du[0][e], du[1][e]);
        }
        if (TN_DOWN) a32[w] = pack_pair(av[0][e], av[1][e]);
      }
    }

    // the next tile's loads, in flight over the store phase; the scheduler
    // may not lift them above the arithmetic, where they would need 24
    // registers of their own
    __builtin_amdgcn_sched_barrier(0);
    const long nrow0 = row0 + MB_TILE;
    const bool nok =
        it + 1 < MB_ROW_ITERS && col_ok && nrow0 + 2 * rp < M;
    {
      const long o = (nrow0 + 2 * rp) * F + col;
      load_row_pair(gate, o, F, nok, gv);
      load_row_pair(up, o, F, nok, uv);
      load_row_pair(d_act, o, F, nok, ov);
    }

    if (TN_GU || TN_DOWN) {
      __syncthreads();
      const long mrow = row0 + mv * 8;  // M % 8 == 0: mrow + 7 < M too
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int c = cr + 32 * j;
        if ((col0 + c < F) && (mrow < M)) {
          const int s = img_slot(c, mv);
          if (TN_GU) {
            *reinterpret_cast<uint4*>(dguT + (col0 + c) * M + mrow) = img_g[s];
            *reinterpret_cast<uint4*>(dguT + (F + col0 + c) * M + mrow) =
                img_u[s];
          }
          if (TN_DOWN)
            *reinterpret_cast<uint4*>(act + (col0 + c) * M + mrow) = img_a[s];
        }
      }
      __syncthreads();
    }
    row0 = nrow0;
    ok = nok;
  }
}

void check_shape(const at::Tensor& t, long rows, long cols, const char* name) {
  TORCH_CHECK(t.size(0) == rows && t.size(1) == cols, name, ": expected [",
              rows, ", ", cols, "], got ", t.sizes());
}

}  // namespace

// Returns (d_gate[M,F], d_up[M,F], dguT[2F,M], act).  With want_guT=false
// dguT is an empty tensor; act is (silu(gate) up)^T [F,M] with want_aT, else
// silu(gate) up row-major [M,F].  d_act is left as it was: d_gate gets a
// buffer of its own.
std::vector<at::Tensor> swiglu_bwd_t(at::Tensor d_act, at::Tensor gate,
                                     at::Tensor up, bool want_guT,
                                     bool want_aT) {
  check_operand(d_act, "swiglu_bwd_t d_act");
  check_operand(gate, "swiglu_bwd_t gate");
  check_operand(up, "swiglu_bwd_t up");
  const long M = gate.size(0), F = gate.size(1);
  check_shape(d_act, M, F, "swiglu_bwd_t d_act");
  check_shape(up, M, F, "swiglu_bwd_t up");
  TORCH_CHECK(d_act.device() == gate.device() && up.device() == gate.device(),
              "swiglu_bwd_t: operands on different devices");
  auto d_gate = at::empty_like(gate);
  auto d_up = at::empty_like(gate);
  auto dguT = want_guT ? at::empty({2 * F, M}, gate.options())
                       : at::empty({0}, gate.options());
  auto act = want_aT ? at::empty({F, M}, gate.options()) : at::empty_like(gate);
  const dim3 grid = tile_grid(M, F);
  auto stream = at::hip::getCurrentHIPStream();
#define SAMD_LAUNCH_SWIGLU_BWD_T(GU, DN)                                     \
  hipLaunchKernelGGL((swiglu_bwd_t_kernel<GU, DN>), grid, dim3(MB_BLOCK), 0, \
                     stream.stream(), bptr(d_act), bptr(gate), bptr(up),     \
                     bptr(d_gate), bptr(d_up),                               \
                     want_guT ? bptr(dguT) : nullptr, bptr(act), M, F)
  if (want_guT && want_aT) SAMD_LAUNCH_SWIGLU_BWD_T(true, true);
  else if (want_guT) SAMD_LAUNCH_SWIGLU_BWD_T(true, false);
  else if (want_aT) SAMD_LAUNCH_SWIGLU_BWD_T(false, true);
  else SAMD_LAUNCH_SWIGLU_BWD_T(false, false);
#undef SAMD_LAUNCH_SWIGLU_BWD_T
  SAMD_CHECK_HIP(hipGetLastError());
  return {d_gate, d_up, dguT, act};
}

// Whole MLP backward for out = down(silu(gate_proj x) * up_proj x):
//   g[M,E] = d out, x[M,E], gate[M,F], up[M,F], W_gate[F,E], W_up[F,E],
//   W_down[E,F].
// Returns (dx, dW_gate, dW_up, dW_down).  tn_gu / tn_down pick the TN route
// per site; a site whose flag is off keeps the NT call dY.t() @ X.  With
// tn_gu the two gradients are the row halves of one [2F, E] product.
std::vector<at::Tensor> llama_mlp_bwd(at::Tensor g, at::Tensor x,
                                      at::Tensor gate, at::Tensor up,
                                      at::Tensor W_gate, at::Tensor W_up,
                                      at::Tensor W_down, bool tn_gu,
                                      bool tn_down) {
  check_operand(g, "llama_mlp_bwd g");
  check_operand(x, "llama_mlp_bwd x");
  check_operand(gate, "llama_mlp_bwd gate");
  check_operand(up, "llama_mlp_bwd up");
  check_operand(W_gate, "llama_mlp_bwd W_gate");
  check_operand(W_up, "llama_mlp_bwd W_up");
  check_operand(W_down, "llama_mlp_bwd W_down");
  const long M = g.size(0), E = g.size(1), F = gate.size(1);
  check_shape(x, M, E, "llama_mlp_bwd x");
  check_shape(gate, M, F, "llama_mlp_bwd gate");
  check_shape(up, M, F, "llama_mlp_bwd up");
  check_shape(W_gate, F, E, "llama_mlp_bwd W_gate");
  check_shape(W_up, F, E, "llama_mlp_bwd W_up");
  check_shape(W_down, E, F, "llama_mlp_bwd W_down");
  const at::Tensor* rest[] = {&x, &gate, &up, &W_gate, &W_up, &W_down};
  const char* names[] = {"x", "gate", "up", "W_gate", "W_up", "W_down"};
  for (int i = 0; i < 6; ++i)
    TORCH_CHECK(rest[i]->device() == g.device(), "llama_mlp_bwd ", names[i],
                ": expected the device of g");

  at::Tensor d_gate, d_up, dguT, act;
  {
    auto d_act = at::mm(g, W_down);
    auto r = swiglu_bwd_t(d_act, gate, up, tn_gu, tn_down);
    d_gate = r[0];
    d_up = r[1];
    dguT = r[2];
    act = r[3];  // [F,M] when tn_down, else [M,F]
  }
  at::Tensor dW_down;
  if (tn_down) {
    auto gT = transpose_colsum_impl(g, false, true)[0];
    dW_down = at::linear(gT, act);
  } else {
    dW_down = at::mm(g.t(), act);
  }
  act.reset();
  at::Tensor dW_gate, dW_up;
  if (tn_gu) {
    auto xT = transpose_colsum_impl(x, false, true)[0];
    auto dW_gu = at::linear(dguT, xT);
    dguT.reset();
    dW_gate = dW_gu.narrow(0, 0, F);
    dW_up = dW_gu.narrow(0, F, F);
  } else {
    dW_gate = at::mm(d_gate.t(), x);
    dW_up = at::mm(d_up.t(), x);
  }
  // the unfused path's two GEMMs and one add: dx keeps its bits
  auto dx = at::mm(d_gate, W_gate) + at::mm(d_up, W_up);
  return {dx, dW_gate, dW_up, dW_down};
}

}  // namespace samd
