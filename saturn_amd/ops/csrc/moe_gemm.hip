// Grouped expert GEMMs of the Mixtral path (K17): the three matrix products
// of E unstacked nn.Linear experts over rows that moe_permute left in expert
// order, one launch each, with the segment sizes read on the device.
//
//   fwd  Y[r,n]    = sum_k xs[r,k] * W_e[n,k]       r in segment e
//   dx   dX[r,k]   = sum_n dY[r,n] * W_e[n,k]       r in segment e
//   dw   dW_e[n,k] = sum_{r in segment e} dY[r,n] * xs[r,k]
//
// Segment e is rows [off_e, off_e + counts[e]) with off the exclusive prefix
// sum of counts; every block derives it from `counts` itself (<= 64 ints at
// block-uniform addresses), so no count ever reaches the host and the calls
// can be captured into a hipGraph.  No atomics, no split-K, no scratch: each
// output tile belongs to exactly one block.
//
// Tile map.  256 threads = 2x2 waves, block tile 128x128, 64x64 per wave
// (4x4 v_mfma_f32_16x16x32_bf16 accumulators), reduction step 64.
//   fwd/dx: grid (column tiles, P/128 + E row-tile slots).  Row tiles start
//     at off_e + i*128, never at multiples of 128 of the global row space; a
//     block walks counts to find its (expert, tile) and returns before its
//     first barrier when its slot lies past the last real tile (P/128 + E
//     bounds sum_e ceil(counts[e]/128) from above).
//   dw: grid (K tiles, Nout tiles, E); the block loops over its segment's
//     rows in 64-row steps from off_e and stores its dW tile once (zeros for
//     an empty expert, so the buffer needs no memset).
// Rows at or past the segment's end and columns past the matrix edge are
// staged into LDS as zeros and never stored, so a block neither reads nor
// writes another expert's rows.
//
// Staging: global -> registers -> LDS in 16-B vectors, the next step's loads
// in flight while the current step multiplies; two LDS buffers of two tiles
// (one barrier per step).  A tile is [128][64+8] when the reduction index is
// contiguous in memory (fragments are plain 16-B LDS reads) and [64][128+8]
// when it is the row index (fragments come through ds_read_tr16_b64, the
// hardware transpose attention.hip uses for V).  The +8 pad keeps both read
// patterns conflict-free.
//
//   kernel | A tile            | B tile
//   fwd    | xs  [128 r][64 k] | W  [128 n][64 k]   both plain reads
//   dx     | dY  [128 r][64 n] | W  [64 n][128 k]   B by transpose read
//   dw     | dY  [64 r][128 n] | xs [64 r][128 k]   both by transpose read
//
// The MFMA operands are swapped (B fragment as A, A fragment as B) so that
// a lane's four accumulator registers are four consecutive columns of one
// output row: the tile is stored with 8-B vectors straight from registers.
//
// Determinism: reduction steps ascend from 0 (fwd, dx) or from off_e (dw),
// and the MFMA order inside a step is fixed, so the order in which an output
// element is accumulated depends only on its own segment and the problem
// sizes, never on where the segment lies in xs or on other experts' counts.
//
// Envelope (TORCH_CHECKed below): bf16, contiguous, one device, 1 <= E <= 64,
// K % 32 == 0, Nout % 32 == 0, equal weight shapes, counts int32 [E], P > 0.
// sum(counts) == P is the caller's (moe_sort guarantees it); rows past
// sum(counts) are left unwritten and a count is clamped to [0, P - off_e],
// never followed past P.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

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

constexpr int GG_MAX_E = 64;
constexpr int GG_BM = 128;          // block tile rows (and columns)
constexpr int GG_BK = 64;           // reduction step
constexpr int GG_PK = GG_BK + 8;    // pitch of a [128][64] tile
constexpr int GG_PT = GG_BM + 8;    // pitch of a [64][128] tile
constexpr int GG_TILE = GG_BM * GG_PK;  // elements per tile slot (>= 64*GG_PT)
constexpr int GG_LDS = 2 * 2 * GG_TILE * (int)sizeof(unsigned short);
static_assert(GG_TILE >= GG_BK * GG_PT, "tile slot holds either shape");

enum GGMode { GG_FWD = 0, GG_DX = 1, GG_DW = 2 };

// the experts' weight matrices, passed by value in the kernel arguments
struct GGWeights {
  const unsigned short* w[GG_MAX_E];
};

// a window into a row-major matrix: rows [row0, row_end), columns
// [col0, col_end) are real, everything else of the tile is staged as zero
struct GGSrc {
  const unsigned short* p;
  long ld;
  long row0, row_end;
  int col0, col_end;
};

// CV = 16-B vectors per tile row: 8 for [128][64], 16 for [64][128]; either
// way a tile is 1024 vectors, four per thread
template <int CV>
__device__ __forceinline__ void gg_load(const GGSrc& s, u32x4 (&reg)[4],
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
__device__ __forceinline__ void gg_stage(unsigned short* tile,
                                         const u32x4 (&reg)[4], int tid) {
  constexpr int PITCH = CV * 8 + 8;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int v = tid + i * 256;
    *reinterpret_cast<u32x4*>(tile + (v / CV) * PITCH + (v % CV) * 8) = reg[i];
  }
}

// fragment of a [128][64] tile: 8 reduction elements of row `row`, one b128
__device__ __forceinline__ bf16x8 gg_frag(const unsigned short* tile, int row,
                                          int k) {
  return *reinterpret_cast<const bf16x8*>(tile + row * GG_PK + k);
}

// fragment of a [64][128] tile by hardware transpose: lane l slot j gets
// tile[k + (l>>4)*8 + j][col0 + (l&15)] (lane -> address map: attention.hip,
// tr16_bfrag)
__device__ __forceinline__ bf16x8 gg_frag_tr(const unsigned short* tile, int k,
                                             int col0, int lane) {
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const unsigned short* p = tile + (k + (lane >> 4) * 8 + ((lane >> 2) & 3)) *
                                       GG_PT + col0 + 4 * (lane & 3);
  bf16x4 v0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)p);
  bf16x4 v1 =
      __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)(p + 4 * GG_PT));
  return __builtin_shufflevector(v0, v1, 0, 1, 2, 3, 4, 5, 6, 7);
}

// a count as the walk uses it: clamped to [0, rows left before P]
__device__ __forceinline__ long gg_count(int c, long left) {
  const long n = c < 0 ? 0 : c;
  return n < left ? n : left;
}

template <int MODE>
__launch_bounds__(256, 2)
__global__ void moe_gemm_kernel(const unsigned short* __restrict__ L,
                                const unsigned short* __restrict__ R,
                                GGWeights wt, const int* __restrict__ counts,
                                unsigned short* __restrict__ out, int E, long P,
                                int Nout, int K) {
  constexpr bool A_TR = MODE == GG_DW;   // A tile is [64][128]
  constexpr bool B_TR = MODE != GG_FWD;  // B tile is [64][128]
  constexpr int ACV = A_TR ? 16 : 8;
  constexpr int BCV = B_TR ? 16 : 8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned short* lds = reinterpret_cast<unsigned short*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wm = tid >> 7, wn = (tid >> 6) & 1;
  const int r = lane & 15, qg = lane >> 4;

  // ---- which segment, which tile (block-uniform) ----
  long seg0 = 0, seg1 = 0;  // this block's segment [seg0, seg1)
  int e = -1;
  if (MODE == GG_DW) {
    e = blockIdx.z;
    for (int i = 0; i <= e; ++i) {
      const long c = gg_count(counts[i], P - seg1);
      seg0 = seg1;
      seg1 += c;
    }
  } else {
    long slot = blockIdx.y;
    for (int i = 0; i < E; ++i) {
      const long c = gg_count(counts[i], P - seg1);
      const long tiles = (c + GG_BM - 1) / GG_BM;
      if (slot < tiles) {
        e = i;
        seg0 = seg1 + slot * GG_BM;  // first row of this tile
        seg1 += c;
        break;
      }
      slot -= tiles;
      seg1 += c;
    }
    if (e < 0) return;  // slot past the last real tile: before any barrier
  }

  // ---- operand windows; out tile origin and edges ----
  GGSrc a, b;
  long orow0, orow_end;
  int ocol0, ocol_end, nsteps;
  long old;
  unsigned short* obase = out;
  if (MODE == GG_FWD) {
    a = GGSrc{L, (long)K, seg0, seg1, 0, K};
    b = GGSrc{wt.w[e], (long)K, (long)blockIdx.x * GG_BM, (long)Nout, 0, K};
    orow0 = seg0, orow_end = seg1, ocol0 = blockIdx.x * GG_BM, ocol_end = Nout;
    old = Nout;
    nsteps = (K + GG_BK - 1) / GG_BK;
  } else if (MODE == GG_DX) {
    a = GGSrc{L, (long)Nout, seg0, seg1, 0, Nout};
    b = GGSrc{wt.w[e], (long)K, 0, (long)Nout, (int)blockIdx.x * GG_BM, K};
    orow0 = seg0, orow_end = seg1, ocol0 = blockIdx.x * GG_BM, ocol_end = K;
    old = K;
    nsteps = (Nout + GG_BK - 1) / GG_BK;
  } else {
    a = GGSrc{L, (long)Nout, seg0, seg1, (int)blockIdx.y * GG_BM, Nout};
    b = GGSrc{R, (long)K, seg0, seg1, (int)blockIdx.x * GG_BM, K};
    orow0 = (long)blockIdx.y * GG_BM, orow_end = Nout;
    ocol0 = blockIdx.x * GG_BM, ocol_end = K;
    old = K;
    obase = out + (long)e * Nout * K;
    nsteps = (int)((seg1 - seg0 + GG_BK - 1) / GG_BK);
  }

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 ra[4], rb[4];
  if (nsteps > 0) {
    gg_load<ACV>(a, ra, tid);
    gg_load<BCV>(b, rb, tid);
    gg_stage<ACV>(lds, ra, tid);
    gg_stage<BCV>(lds + GG_TILE, rb, tid);
  }
  __syncthreads();

  for (int s = 0; s < nsteps; ++s) {
    const unsigned short* At = lds + (s & 1) * 2 * GG_TILE;
    const unsigned short* Bt = At + GG_TILE;
    const bool more = s + 1 < nsteps;
    if (more) {
      // advance both windows along the reduction and start the next loads
      if (MODE == GG_FWD) a.col0 += GG_BK, b.col0 += GG_BK;
      if (MODE == GG_DX) a.col0 += GG_BK, b.row0 += GG_BK;
      if (MODE == GG_DW) a.row0 += GG_BK, b.row0 += GG_BK;
      gg_load<ACV>(a, ra, tid);
      gg_load<BCV>(b, rb, tid);
    }
#pragma unroll
    for (int ks = 0; ks < GG_BK; ks += 32) {
      bf16x8 fa[4], fb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m0 = wm * 64 + i * 16, n0 = wn * 64 + i * 16;
        fa[i] = A_TR ? gg_frag_tr(At, ks, m0, lane)
                     : gg_frag(At, m0 + r, ks + qg * 8);
        fb[i] = B_TR ? gg_frag_tr(Bt, ks, n0, lane)
                     : gg_frag(Bt, n0 + r, ks + qg * 8);
      }
      // swapped operands: acc[i][j][c] = C[m0 + r][n0 + qg*4 + c]
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
      unsigned short* nxt = lds + ((s + 1) & 1) * 2 * GG_TILE;
      gg_stage<ACV>(nxt, ra, tid);
      gg_stage<BCV>(nxt + GG_TILE, rb, tid);
    }
    __syncthreads();
  }

  // ---- store: one rounding, 4 consecutive columns (8 B) per accumulator ----
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long row = orow0 + wm * 64 + i * 16 + r;
    if (row >= orow_end) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = ocol0 + wn * 64 + j * 16 + qg * 4;
      if (col >= ocol_end) continue;
      const f32x4 v = acc[i][j];
      u32x2 pk;
      pk.x = (unsigned)f2us(v[0]) | ((unsigned)f2us(v[1]) << 16);
      pk.y = (unsigned)f2us(v[2]) | ((unsigned)f2us(v[3]) << 16);
      *reinterpret_cast<u32x2*>(obase + row * old + col) = pk;
    }
  }
}

const unsigned short* gg_in(const at::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}

void gg_check_rows(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16, got ",
              t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), name,
              " must be a contiguous 2-D tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

// checks counts and the weight list, fills the pointer table; returns
// {E, Nout, K}
struct GGShape {
  int E, Nout, K;
};
GGShape gg_check(const at::Tensor& rows, const char* rows_name,
                 const at::Tensor& counts,
                 const std::vector<at::Tensor>* weights, GGWeights* table) {
  gg_check_rows(rows, rows_name);
  TORCH_CHECK(rows.size(0) > 0, rows_name, " must have at least one row");
  TORCH_CHECK(counts.is_cuda() && counts.device() == rows.device(),
              "counts must be on the device of ", rows_name);
  TORCH_CHECK(counts.scalar_type() == at::kInt, "counts must be int32, got ",
              counts.scalar_type());
  TORCH_CHECK(counts.dim() == 1 && counts.is_contiguous(),
              "counts must be a contiguous 1-D tensor");
  const long E = counts.size(0);
  TORCH_CHECK(E >= 1 && E <= GG_MAX_E, "counts must have 1..", GG_MAX_E,
              " entries, got ", E);
  GGShape s{(int)E, 0, 0};
  if (!weights) return s;
  TORCH_CHECK((long)weights->size() == E, "weights must hold one matrix per "
              "entry of counts (", E, "), got ", weights->size());
  for (long i = 0; i < E; ++i) {
    const at::Tensor& w = (*weights)[i];
    gg_check_rows(w, "weights");
    TORCH_CHECK(w.device() == rows.device(), "weights must be on the device "
                "of ", rows_name);
    TORCH_CHECK(w.sizes() == (*weights)[0].sizes(), "weights must all have "
                "the same shape: weights[", i, "] is ", w.sizes(),
                ", weights[0] is ", (*weights)[0].sizes());
    table->w[i] = gg_in(w);
  }
  for (long i = E; i < GG_MAX_E; ++i) table->w[i] = nullptr;
  s.Nout = (int)(*weights)[0].size(0);
  s.K = (int)(*weights)[0].size(1);
  TORCH_CHECK(s.K > 0 && s.K % 32 == 0, "weights: K (", s.K,
              ") must be a positive multiple of 32");
  TORCH_CHECK(s.Nout > 0 && s.Nout % 32 == 0, "weights: Nout (", s.Nout,
              ") must be a positive multiple of 32");
  return s;
}

template <int MODE>
void gg_launch(dim3 grid, const at::Tensor& L, const unsigned short* R,
               const GGWeights& table, const at::Tensor& counts,
               at::Tensor& out, int E, long P, int Nout, int K) {
  static std::atomic<bool> lds_raised{false};
  if (!lds_raised.load(std::memory_order_relaxed)) {
    SAMD_CHECK_HIP(hipFuncSetAttribute(
        reinterpret_cast<const void*>(moe_gemm_kernel<MODE>),
        hipFuncAttributeMaxDynamicSharedMemorySize, GG_LDS));
    lds_raised.store(true, std::memory_order_relaxed);
  }
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_gemm_kernel<MODE>, grid, dim3(256), GG_LDS,
                     stream.stream(), gg_in(L), R, table,
                     counts.data_ptr<int>(),
                     reinterpret_cast<unsigned short*>(out.data_ptr()), E, P,
                     Nout, K);
  SAMD_CHECK_HIP(hipGetLastError());
}

inline unsigned gg_tiles(long n) { return (unsigned)((n + GG_BM - 1) / GG_BM); }

}  // namespace

at::Tensor moe_gemm_fwd(at::Tensor xs, at::Tensor counts,
                        std::vector<at::Tensor> weights) {
  GGWeights table;
  const GGShape s = gg_check(xs, "xs", counts, &weights, &table);
  const long P = xs.size(0);
  TORCH_CHECK(xs.size(1) == s.K, "xs must have K = ", s.K, " columns, got ",
              xs.size(1));
  TORCH_CHECK(P / GG_BM + s.E <= 65535, "xs has too many rows");
  auto y = at::empty({P, (long)s.Nout}, xs.options());
  gg_launch<GG_FWD>(dim3(gg_tiles(s.Nout), (unsigned)(P / GG_BM + s.E)), xs,
                    nullptr, table, counts, y, s.E, P, s.Nout, s.K);
  return y;
}

at::Tensor moe_gemm_dx(at::Tensor dy, at::Tensor counts,
                       std::vector<at::Tensor> weights) {
  GGWeights table;
  const GGShape s = gg_check(dy, "dy", counts, &weights, &table);
  const long P = dy.size(0);
  TORCH_CHECK(dy.size(1) == s.Nout, "dy must have Nout = ", s.Nout,
              " columns, got ", dy.size(1));
  TORCH_CHECK(P / GG_BM + s.E <= 65535, "dy has too many rows");
  auto dx = at::empty({P, (long)s.K}, dy.options());
  gg_launch<GG_DX>(dim3(gg_tiles(s.K), (unsigned)(P / GG_BM + s.E)), dy,
                   nullptr, table, counts, dx, s.E, P, s.Nout, s.K);
  return dx;
}

at::Tensor moe_gemm_dw(at::Tensor dy, at::Tensor xs, at::Tensor counts) {
  const GGShape s = gg_check(dy, "dy", counts, nullptr, nullptr);
  gg_check_rows(xs, "xs");
  TORCH_CHECK(xs.device() == dy.device(), "xs must be on the device of dy");
  const long P = dy.size(0);
  TORCH_CHECK(xs.size(0) == P, "xs and dy must have the same number of rows");
  const long Nout = dy.size(1), K = xs.size(1);
  TORCH_CHECK(K > 0 && K % 32 == 0, "xs: K (", K,
              ") must be a positive multiple of 32");
  TORCH_CHECK(Nout > 0 && Nout % 32 == 0, "dy: Nout (", Nout,
              ") must be a positive multiple of 32");
  TORCH_CHECK(gg_tiles(Nout) <= 65535, "dy has too many columns");
  auto dw = at::empty({(long)s.E, Nout, K}, dy.options());
  GGWeights table{};
  gg_launch<GG_DW>(dim3(gg_tiles(K), gg_tiles(Nout), (unsigned)s.E), dy,
                   gg_in(xs), table, counts, dw, s.E, P, (int)Nout, (int)K);
  return dw;
}

}  // namespace samd
