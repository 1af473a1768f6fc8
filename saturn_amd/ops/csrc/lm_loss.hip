// Fused lm_head + cross-entropy (K18): the loss of logits = h W^T + bias and
// its gradients without a [N, V] logits or dlogits tensor.
//
//   N = B*T rows, K = n_embd, V = vocabulary; h [N,K], W [V,K], bias [V] or
//   absent, t_r the target of row r (ignore_index: the row does not count).
//
//   forward   STAT   per (row, 128-column tile): m = max x, s = sum exp(x - m)
//                    of the fp32 logits x, and the target's logit
//             merge  lse[r] from the row's partials; loss[r] = lse - x[r,t_r]
//   backward, per vocabulary chunk [c0, c0 + vcw):
//             DL     dl[r,v] = g_r (exp(x - lse[r]) - [v == t_r])   bf16 [N,vcw]
//             DH     dh[r,k]    += sum_v dl[r,v] W[c0+v,k]
//             DW     dW[c0+v,k]  = sum_r dl[r,v] h[r,k]
//
// The logits live only as MFMA accumulators: STAT reduces them, DL recomputes
// them (one extra GEMM) and keeps one chunk of dl.  Chunking over the
// vocabulary, not over rows, leaves every dW element to one block and one
// summation order; only dh crosses chunks.
//
// Tile map (the design of moe_gemm.hip, K17; the small load / stage /
// fragment helpers are copied here so that K17's code object is unchanged).
// 256 threads = 2x2 waves, block tile 128x128, 64x64 per wave as 4x4
// v_mfma_f32_16x16x32_bf16 accumulators, reduction step 64, global ->
// registers -> LDS in 16-B vectors with the next step's loads in flight, two
// LDS buffers, one barrier per step.  A tile is [128][64+8] where the
// reduction index is contiguous (plain 16-B LDS reads) and [64][128+8] where
// it is the row index (ds_read_tr16_b64).  Edges are staged as zeros and
// never stored.
//
//   mode | grid (x, y)            | A tile            | B tile
//   STAT | (V/128,  N/128) ceil   | h  [128 r][64 k]  | W  [128 v][64 k]
//   DL   | (vcw/128, N/128)       | h  [128 r][64 k]  | W  [128 v][64 k]
//   DH   | (K/128,  N/128)        | dl [128 r][64 v]  | W  [64 v][128 k]  tr
//   DW   | (K/128,  vcw/128)      | dl [64 r][128 v]  | h  [64 r][128 k]  both tr
//
// Operands are swapped in the MFMA so that acc[i][j][c] is
// C[m0 + i*16 + r][n0 + j*16 + qg*4 + c] (r = lane & 15, qg = lane >> 4): a
// lane holds 16 columns of each of its 4 rows, four consecutive per register
// quad.
//
// Epilogues.
//   STAT  x += bias (fp32), columns >= V become -inf; (m, s) per row: over
//         the lane's 16 values, shfl_xor 16 and 32 across qg, the two wn
//         waves through the staging LDS (free after the loop's last barrier);
//         one float2 per row into part[N][V/128].  The one lane of the grid
//         that owns column t_r stores x to tlogit[r] (zero-filled by the
//         launcher; a target outside [0, V) matches no column).
//   DL    one rounding to bf16, 8-B stores, zeros for columns >= V and for
//         ignored rows.  BIAS: column sums of the ROUNDED values over the
//         block's 128 rows (over i, shfl_xor 1,2,4,8 over r, wm through LDS)
//         into dbpart[row tile][v]; the launcher sums the row tiles.
//   DH    accumulators start from the fp32 tile of dh32 on every chunk but
//         the first and go back to it on every chunk but the last, which
//         rounds once into dh: with vcw % 64 == 0 each accumulator sees the
//         unchunked sequence of MFMAs, so dh does not depend on the chunking.
//   DW    all N rows in ascending 64-row steps, one bf16 store.
//
// No atomics, no scratch, nothing read on the host; every [N, V]-sized index
// is a long.  Envelope (TORCH_CHECKed): bf16, contiguous, 16-B aligned, one
// device, K % 32 == 0, V >= 1, targets int64 [N], chunk % 128 == 0.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <algorithm>
#include <atomic>

#include "common.h"
#include "ops.h"

namespace samd {

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;  // 16 B in flight
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int LC_BM = 128;          // block tile rows (and columns)
constexpr int LC_BK = 64;           // reduction step
constexpr int LC_PK = LC_BK + 8;    // pitch of a [128][64] tile
constexpr int LC_PT = LC_BM + 8;    // pitch of a [64][128] tile
constexpr int LC_TILE = LC_BM * LC_PK;  // elements per tile slot
constexpr int LC_LDS = 2 * 2 * LC_TILE * (int)sizeof(unsigned short);
static_assert(LC_TILE >= LC_BK * LC_PT, "tile slot holds either shape");
constexpr long LC_CHUNK_BYTES = 64l << 20;  // default dl chunk: N*vc*2 B

enum LCMode { LC_STAT = 0, LC_DL = 1, LC_DH = 2, LC_DW = 3 };

// a window into a row-major matrix: rows [row0, row_end), columns
// [col0, col_end) are real, everything else of the tile is staged as zero
struct LCSrc {
  const unsigned short* p;
  long ld;
  long row0, row_end;
  int col0, col_end;
};

struct LCArgs {
  const unsigned short* h;     // [N, K]
  const unsigned short* w;     // [V, K]
  const unsigned short* bias;  // [V] or null
  const long* targets;         // [N]
  const float* lse;            // [N]            DL
  const float* gscale;         // [1]            DL
  unsigned short* dl;          // [N, vcw]       DL out; DH, DW in
  float2* part;                // [N, nvt]       STAT
  float* tlogit;               // [N]            STAT
  float* dbpart;               // [N/128, vpad]  DL with bias
  float* dh32;                 // [N, K]         DH, more than one chunk
  unsigned short* dh;          // [N, K]         DH, last chunk
  unsigned short* dw;          // [V, K]         DW
  long N, ignore_index;
  int K, V, c0, vcw, nvt, vpad;
  int first, last;             // DH: this chunk's place in the sequence
};

// CV = 16-B vectors per tile row: 8 for [128][64], 16 for [64][128]; either
// way a tile is 1024 vectors, four per thread
template <int CV>
__device__ __forceinline__ void lc_load(const LCSrc& s, u32x4 (&reg)[4],
                                        int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = tid + i * 256;
    const long row = s.row0 + v / CV;
    const int col = s.col0 + (v % CV) * 8;
    reg[i] = (row < s.row_end && col < s.col_end)
                 ? *reinterpret_cast<const u32x4*>(s.p + row * s.ld + col)
                 : u32x4{0u, 0u, 0u, 0u};
  }
}

template <int CV>
__device__ __forceinline__ void lc_stage(unsigned short* tile,
                                         const u32x4 (&reg)[4], int tid) {
  constexpr int PITCH = CV * 8 + 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = tid + i * 256;
    *reinterpret_cast<u32x4*>(tile + (v / CV) * PITCH + (v % CV) * 8) = reg[i];
  }
}

// fragment of a [128][64] tile: 8 reduction elements of row `row`, one b128
__device__ __forceinline__ bf16x8 lc_frag(const unsigned short* tile, int row,
                                          int k) {
  return *reinterpret_cast<const bf16x8*>(tile + row * LC_PK + k);
}

// fragment of a [64][128] tile by hardware transpose: lane l slot j gets
// tile[k + (l>>4)*8 + j][col0 + (l&15)]
__device__ __forceinline__ bf16x8 lc_frag_tr(const unsigned short* tile, int k,
                                             int col0, int lane) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const unsigned short* p = tile + (k + (lane >> 4) * 8 + ((lane >> 2) & 3)) *
                                       LC_PT + col0 + 4 * (lane & 3);
  bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
  bf16x4 v1 =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 4 * LC_PT));
  return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// softmax partials (m, s = sum exp(x - m)); (-inf, 0) is the empty one
__device__ __forceinline__ void lc_merge(float& m, float& s, float m2,
                                         float s2) {
  const float mm = fmaxf(m, m2);
  s = mm == -INFINITY ? 0.f : s * __expf(m - mm) + s2 * __expf(m2 - mm);
  m = mm;
}

__device__ __forceinline__ u32x2 lc_pack(const unsigned short (&u)[4]) {
  u32x2 pk;
  pk.x = (unsigned)u[0] | ((unsigned)u[1] << 16);
  pk.y = (unsigned)u[2] | ((unsigned)u[3] << 16);
  return pk;
}

template <int MODE, bool BIAS>
__launch_bounds__(256, 2)
__global__ void lce_gemm_kernel(LCArgs p) {
  constexpr bool A_TR = MODE == LC_DW;                   // A tile is [64][128]
  constexpr bool B_TR = MODE == LC_DH || MODE == LC_DW;  // B tile is [64][128]
  constexpr int ACV = A_TR ? 16 : 8;
  constexpr int BCV = B_TR ? 16 : 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* lds = reinterpret_cast<unsigned short*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wm = tid >> 7, wn = (tid >> 6) & 1;
  const int r = lane & 15, qg = lane >> 4;
  const long N = p.N;
  const int K = p.K, V = p.V;

  // ---- operand windows; tile origin (m0 rows, n0 columns of C) ----
  LCSrc a, b;
  long m0;
  int n0, nsteps;
  if (MODE == LC_STAT || MODE == LC_DL) {
    m0 = (long)blockIdx.y * LC_BM;
    n0 = (MODE == LC_DL ? p.c0 : 0) + (int)blockIdx.x * LC_BM;  // vocabulary
    a = LCSrc{p.h, (long)K, m0, N, 0, K};
    b = LCSrc{p.w, (long)K, (long)n0, (long)V, 0, K};
    nsteps = (K + LC_BK - 1) / LC_BK;
  } else if (MODE == LC_DH) {
    m0 = (long)blockIdx.y * LC_BM;
    n0 = (int)blockIdx.x * LC_BM;  // k
    a = LCSrc{p.dl, (long)p.vcw, m0, N, 0, p.vcw};
    b = LCSrc{p.w, (long)K, (long)p.c0, (long)V, n0, K};
    nsteps = p.vcw / LC_BK;
  } else {
    m0 = (long)blockIdx.y * LC_BM;  // vocabulary, relative to c0
    n0 = (int)blockIdx.x * LC_BM;   // k
    a = LCSrc{p.dl, (long)p.vcw, 0, N, (int)m0, p.vcw};
    b = LCSrc{p.h, (long)K, 0, N, n0, K};
    nsteps = (int)((N + LC_BK - 1) / LC_BK);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (MODE == LC_DH && !p.first) {
    // a later chunk continues the fp32 sums of the earlier ones
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = m0 + wm * 64 + i * 16 + r;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + wn * 64 + j * 16 + qg * 4;
        if (row < N && col < K)
          acc[i][j] = *reinterpret_cast<const f32x4*>(p.dh32 + row * K + col);
      }
    }
  }

  u32x4 ra[4], rb[4];
  lc_load<ACV>(a, ra, tid);
  lc_load<BCV>(b, rb, tid);
  lc_stage<ACV>(lds, ra, tid);
  lc_stage<BCV>(lds + LC_TILE, rb, tid);
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const unsigned short* At = lds + (s & 1) * 2 * LC_TILE;
    const unsigned short* Bt = At + LC_TILE;
    const bool more = s + 1 < nsteps;
    if (more) {
      // advance both windows along the reduction and start the next loads
      if (A_TR) a.row0 += LC_BK; else a.col0 += LC_BK;
      if (B_TR) b.row0 += LC_BK; else b.col0 += LC_BK;
      lc_load<ACV>(a, ra, tid);
      lc_load<BCV>(b, rb, tid);
    }
#pragma unroll
    for (int ks = 0; ks < LC_BK; ks += 32) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int am = wm * 64 + i * 16, bn = wn * 64 + i * 16;
        fa[i] = A_TR ? lc_frag_tr(At, ks, am, lane)
                     : lc_frag(At, am + r, ks + qg * 8);
        fb[i] = B_TR ? lc_frag_tr(Bt, ks, bn, lane)
                     : lc_frag(Bt, bn + r, ks + qg * 8);
      }
      // swapped operands: acc[i][j][c] = C[am + r][bn + qg*4 + c]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              fb[j], fa[i], acc[i][j], 0, 0, 0);
    }
    if (more) {
      // the other buffer was last read in step s-1, before the barrier
      // that ended it
      unsigned short* nxt = lds + ((s + 1) & 1) * 2 * LC_TILE;
      lc_stage<ACV>(nxt, ra, tid);
      lc_stage<BCV>(nxt + LC_TILE, rb, tid);
    }
    __syncthreads();
  }
  // every wave is past its last LDS read: the staging buffers are free

  const int cl0 = wn * 64 + qg * 4;  // + j*16 + c: column inside the tile

  if (MODE == LC_STAT || MODE == LC_DL) {
    // the lane's 16 bias values, shared by its 4 rows
    float bv[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int col = n0 + cl0 + j * 16 + c;
        bv[j][c] = (BIAS && col < V) ? us2f(p.bias[col]) : 0.f;
      }

    if (MODE == LC_STAT) {
      float2* red = reinterpret_cast<float2*>(smem);  // [128 rows]
      float mi[4], si[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rl = wm * 64 + i * 16 + r;
        const long row = m0 + rl;
        const long t = row < N ? p.targets[row] : -1;
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int col = n0 + cl0 + j * 16 + c;
            const float x = col < V ? acc[i][j][c] + bv[j][c] : -INFINITY;
            acc[i][j][c] = x;
            m = fmaxf(m, x);
            if (col < V && (long)col == t) p.tlogit[row] = x;
          }
        float s = 0.f;
        if (m > -INFINITY) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) s += __expf(acc[i][j][c] - m);
        }
        lc_merge(m, s, __shfl_xor(m, 16, 64), __shfl_xor(s, 16, 64));
        lc_merge(m, s, __shfl_xor(m, 32, 64), __shfl_xor(s, 32, 64));
        mi[i] = m, si[i] = s;
        if (wn == 1 && qg == 0) red[rl] = make_float2(m, s);
      }
      __syncthreads();
      if (wn == 0 && qg == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int rl = wm * 64 + i * 16 + r;
          const long row = m0 + rl;
          const float2 o = red[rl];
          lc_merge(mi[i], si[i], o.x, o.y);
          if (row < N)
            p.part[row * p.nvt + blockIdx.x] = make_float2(mi[i], si[i]);
        }
      }
    } else {
      const float g = p.gscale[0];
      const int tc0 = (int)blockIdx.x * LC_BM;  // tile's column in the chunk
      float csum[4][4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 4; ++c) csum[j][c] = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const long row = m0 + wm * 64 + i * 16 + r;
        const bool live = row < N;
        const long t = live ? p.targets[row] : p.ignore_index;
        const float l = live ? p.lse[row] : 0.f;
        const bool counts = live && t != p.ignore_index;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned short u[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const int col = n0 + cl0 + j * 16 + c;
            const float pr = __expf(acc[i][j][c] + bv[j][c] - l);
            const float d = g * (pr - ((long)col == t ? 1.f : 0.f));
            u[c] = f2us((counts && col < V) ? d : 0.f);
            if (BIAS) csum[j][c] += us2f(u[c]);
          }
          if (live)
            *reinterpret_cast<u32x2*>(p.dl + row * p.vcw + tc0 + cl0 + j * 16) =
                lc_pack(u);
        }
      }
      if (BIAS) {
        float* red = reinterpret_cast<float*>(smem);  // [128 columns]
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float v = csum[j][c];
            v += __shfl_xor(v, 1, 64);
            v += __shfl_xor(v, 2, 64);
            v += __shfl_xor(v, 4, 64);
            v += __shfl_xor(v, 8, 64);
            csum[j][c] = v;
            if (wm == 1 && r == 0) red[cl0 + j * 16 + c] = v;
          }
        __syncthreads();
        if (wm == 0 && r == 0) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const int cl = cl0 + j * 16 + c;
              if (n0 + cl < p.vpad)
                p.dbpart[(long)blockIdx.y * p.vpad + n0 + cl] =
                    csum[j][c] + red[cl];
            }
        }
      }
    }
  } else {
    // ---- DH, DW: plain tile store, 4 consecutive columns per quad ----
    const long orow0 = MODE == LC_DW ? (long)p.c0 + m0 : m0;
    const long orow_end = MODE == LC_DW ? (long)V : N;
    const bool as_f32 = MODE == LC_DH && !p.last;
    unsigned short* out = MODE == LC_DW ? p.dw : p.dh;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long row = orow0 + wm * 64 + i * 16 + r;
      if (row >= orow_end) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int col = n0 + cl0 + j * 16;
        if (col >= K) continue;
        const f32x4 v = acc[i][j];
        if (as_f32) {
          *reinterpret_cast<f32x4*>(p.dh32 + row * K + col) = v;
        } else {
          const unsigned short u[4] = {f2us(v[0]), f2us(v[1]), f2us(v[2]),
                                       f2us(v[3])};
          *reinterpret_cast<u32x2*>(out + row * K + col) = lc_pack(u);
        }
      }
    }
  }
}

// one wave per row: the row's nvt partials in a fixed order (lane-strided,
// then a butterfly), lse and the row's loss
__launch_bounds__(256)
__global__ void lce_merge_kernel(const float2* __restrict__ part,
                                 const float* __restrict__ tlogit,
                                 const long* __restrict__ targets,
                                 float* __restrict__ lse,
                                 float* __restrict__ loss, long N, int nvt,
                                 long ignore_index) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= N) return;
  float m = -INFINITY, s = 0.f;
  for (int i = lane; i < nvt; i += 64) {
    const float2 o = part[row * nvt + i];
    lc_merge(m, s, o.x, o.y);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    lc_merge(m, s, __shfl_xor(m, off, 64), __shfl_xor(s, off, 64));
  if (lane == 0) {
    const float l = m + logf(s);
    lse[row] = l;
    loss[row] = targets[row] == ignore_index ? 0.f : l - tlogit[row];
  }
}

const unsigned short* lc_in(const at::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}
unsigned short* lc_out(at::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

void lc_check_bf16(const at::Tensor& t, const char* name, int dim) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == dim && t.is_contiguous(), name,
              " must be a contiguous ", dim, "-D tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

void lc_check_vec(const at::Tensor& t, const char* name, at::ScalarType ty,
                  long n, const at::Tensor& like) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name,
              " must be on the device of hidden");
  TORCH_CHECK(t.scalar_type() == ty, name, " must be ", ty, ", got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 1 && t.is_contiguous() && t.size(0) == n, name,
              " must be a contiguous 1-D tensor of ", n, " elements, got ",
              t.sizes());
}

// the checks both launchers share; fills the argument block's inputs
LCArgs lc_check(const at::Tensor& h, const at::Tensor& w,
                const c10::optional<at::Tensor>& bias,
                const at::Tensor& targets, int64_t ignore_index) {
  lc_check_bf16(h, "hidden", 2);
  lc_check_bf16(w, "weight", 2);
  TORCH_CHECK(w.device() == h.device(), "weight must be on the device of "
              "hidden");
  const long N = h.size(0), K = h.size(1), V = w.size(0);
  TORCH_CHECK(K > 0 && K % 32 == 0, "hidden: K (", K,
              ") must be a positive multiple of 32");
  TORCH_CHECK(w.size(1) == K, "weight must have K = ", K, " columns, got ",
              w.size(1));
  TORCH_CHECK(N >= 1, "hidden must have at least one row");
  TORCH_CHECK(V >= 1 && V <= (1l << 30), "weight: V (", V, ") out of range");
  TORCH_CHECK((N + LC_BM - 1) / LC_BM <= 65535, "hidden has too many rows");
  TORCH_CHECK(K / LC_BM + 1 <= 65535, "hidden has too many columns");
  lc_check_vec(targets, "targets", at::kLong, N, h);
  LCArgs a{};
  if (bias.has_value()) {
    lc_check_bf16(*bias, "bias", 1);
    TORCH_CHECK(bias->device() == h.device() && bias->size(0) == V,
                "bias must hold V = ", V, " elements on the device of hidden");
    a.bias = lc_in(*bias);
  }
  a.h = lc_in(h);
  a.w = lc_in(w);
  a.targets = reinterpret_cast<const long*>(targets.data_ptr<int64_t>());
  a.N = N;
  a.K = (int)K;
  a.V = (int)V;
  a.ignore_index = ignore_index;
  a.nvt = (int)((V + LC_BM - 1) / LC_BM);
  a.vpad = a.nvt * LC_BM;
  return a;
}

template <int MODE, bool BIAS>
void lc_launch(dim3 grid, const LCArgs& a) {
  static std::atomic<bool> lds_raised{false};
  if (!lds_raised.load(std::memory_order_relaxed)) {
    SAMD_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(lce_gemm_kernel<MODE, BIAS>),
        hipFuncAttributeMaxDynamicSharedMemorySize, LC_LDS));
    lds_raised.store(true, std::memory_order_relaxed);
  }
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL((lce_gemm_kernel<MODE, BIAS>), grid, dim3(256), LC_LDS,
                     stream.stream(), a);
  SAMD_CHECK_HIP(hipGetLastError());
}

inline unsigned lc_tiles(long n) { return (unsigned)((n + LC_BM - 1) / LC_BM); }

}  // namespace

std::vector<at::Tensor> lce_fwd(at::Tensor hidden, at::Tensor weight,
                                c10::optional<at::Tensor> bias,
                                at::Tensor targets, int64_t ignore_index) {
  LCArgs a = lc_check(hidden, weight, bias, targets, ignore_index);
  const auto f32 = hidden.options().dtype(at::kFloat);
  auto part = at::empty({a.N, (long)a.nvt, 2}, f32);
  auto tlogit = at::zeros({a.N}, f32);
  auto lse = at::empty({a.N}, f32);
  auto loss = at::empty({a.N}, f32);
  a.part = reinterpret_cast<float2*>(part.data_ptr<float>());
  a.tlogit = tlogit.data_ptr<float>();
  const dim3 grid((unsigned)a.nvt, lc_tiles(a.N));
  if (a.bias) lc_launch<LC_STAT, true>(grid, a);
  else lc_launch<LC_STAT, false>(grid, a);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(lce_merge_kernel, dim3((unsigned)((a.N + 3) / 4)),
                     dim3(256), 0, stream.stream(), a.part, a.tlogit,
                     a.targets, lse.data_ptr<float>(), loss.data_ptr<float>(),
                     a.N, a.nvt, (long)ignore_index);
  SAMD_CHECK_HIP(hipGetLastError());
  return {loss, lse};
}

std::vector<at::Tensor> lce_bwd(at::Tensor hidden, at::Tensor weight,
                                c10::optional<at::Tensor> bias,
                                at::Tensor targets, at::Tensor lse,
                                at::Tensor gscale, int64_t ignore_index,
                                int64_t chunk) {
  LCArgs a = lc_check(hidden, weight, bias, targets, ignore_index);
  lc_check_vec(lse, "lse", at::kFloat, a.N, hidden);
  lc_check_vec(gscale, "gscale", at::kFloat, 1, hidden);
  TORCH_CHECK(chunk >= 0 && chunk % LC_BM == 0, "chunk (", chunk,
              ") must be a positive multiple of ", LC_BM,
              ", or 0 for the default");
  // chunk width from shapes alone: the largest multiple of 128 whose dl
  // buffer stays within LC_CHUNK_BYTES, at least one tile, at most all of V
  long vc = chunk > 0 ? chunk : LC_CHUNK_BYTES / (a.N * 2) / LC_BM * LC_BM;
  vc = std::min(std::max(vc, (long)LC_BM), (long)a.vpad);
  vc = std::min(vc, 65535l * LC_BM);  // DW's grid.y
  const int nchunks = (int)((a.vpad + vc - 1) / vc);

  const auto f32 = hidden.options().dtype(at::kFloat);
  auto dh = at::empty_like(hidden);
  auto dw = at::empty_like(weight);
  auto dl = at::empty({a.N * vc}, hidden.options());
  at::Tensor dh32, dbpart;
  if (nchunks > 1) dh32 = at::empty({a.N, (long)a.K}, f32);
  if (a.bias) dbpart = at::empty({(long)lc_tiles(a.N), (long)a.vpad}, f32);
  a.lse = lse.data_ptr<float>();
  a.gscale = gscale.data_ptr<float>();
  a.dl = lc_out(dl);
  a.dh32 = nchunks > 1 ? dh32.data_ptr<float>() : nullptr;
  a.dbpart = a.bias ? dbpart.data_ptr<float>() : nullptr;
  a.dh = lc_out(dh);
  a.dw = lc_out(dw);

  for (int ci = 0; ci < nchunks; ++ci) {
    a.c0 = (int)(ci * vc);
    a.vcw = (int)std::min(vc, (long)a.vpad - a.c0);  // whole tiles up to V
    a.first = ci == 0;
    a.last = ci == nchunks - 1;
    const dim3 gdl(a.vcw / LC_BM, lc_tiles(a.N));
    if (a.bias) lc_launch<LC_DL, true>(gdl, a);
    else lc_launch<LC_DL, false>(gdl, a);
    lc_launch<LC_DH, false>(dim3(lc_tiles(a.K), lc_tiles(a.N)), a);
    lc_launch<LC_DW, false>(dim3(lc_tiles(a.K), a.vcw / LC_BM), a);
  }
  std::vector<at::Tensor> out{dh, dw};
  if (a.bias)
    out.push_back(dbpart.sum(0).slice(0, 0, a.V).to(at::kBFloat16));
  return out;
}

}  // namespace samd
