// The 64x64 transposed LDS tile image shared by the kernels that store a
// bf16 operand both row-major and transposed (mlp_bwd.hip,
// gptj_block_bwd.hip), with the host helpers their wrappers use.
//
// Lane (rp, cv) of a 256-thread block holds rows 2rp, 2rp+1 x columns
// 8cv..8cv+7 of a tile and writes each column's row pair as one dword into
// the image: 64 image rows (one per source column) of 128 B (the 64 source
// rows).  The 16-B slot s of image row c is stored at slot s ^ (c >> 3),
// which makes the dword writes (a half-wave covers 8 cv x 4 rp) and the
// ds_read_b128 of the store phase (a wave covers 8 image rows of one c >> 3)
// hit every bank once.
#pragma once

#include <torch/extension.h>

#include <vector>

#include "common.h"

namespace samd {

constexpr int MB_TILE = 64;
constexpr int MB_ROW_ITERS = 4;
constexpr int MB_BLOCK = 256;

// the same 16-bit type the elementwise kernels are instantiated with, so
// toF/fromF round identically
typedef c10::BFloat16 bf16_t;

// dword index of (image row c, source-row pair rp) in the swizzled image
__device__ __forceinline__ int img_dword(int c, int rp) {
  return c * 32 + (((rp >> 2) ^ (c >> 3)) << 2) + (rp & 3);
}
// 16-B slot index of (image row c, source rows 8mv..8mv+7)
__device__ __forceinline__ int img_slot(int c, int mv) {
  return c * 8 + (mv ^ (c >> 3));
}

__device__ __forceinline__ float sum8_bf16(const uint4 v) {
  float s = us2f((unsigned short)(v.x & 0xffffu));
  s += us2f((unsigned short)(v.x >> 16));
  s += us2f((unsigned short)(v.y & 0xffffu));
  s += us2f((unsigned short)(v.y >> 16));
  s += us2f((unsigned short)(v.z & 0xffffu));
  s += us2f((unsigned short)(v.z >> 16));
  s += us2f((unsigned short)(v.w & 0xffffu));
  s += us2f((unsigned short)(v.w >> 16));
  return s;
}

// Sum the 8 lanes that share an image row, gather the block's 64 column
// sums in LDS and store them as 16 float4.
__device__ __forceinline__ void store_colsums(float acc0, float acc1,
                                              float4* lds_sum,
                                              float* __restrict__ partial,
                                              long col0, long ncols) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int off = 1; off < 8; off <<= 1) {
    acc0 += __shfl_xor(acc0, off, 64);
    acc1 += __shfl_xor(acc1, off, 64);
  }
  float* s = reinterpret_cast<float*>(lds_sum);
  if ((tid & 7) == 0) {
    s[tid >> 3] = acc0;
    s[(tid >> 3) + 32] = acc1;
  }
  __syncthreads();
  if (tid < MB_TILE / 4 && col0 + tid * 4 < ncols) {
    *reinterpret_cast<float4*>(partial + (long)blockIdx.y * ncols + col0 +
                               tid * 4) = lds_sum[tid];
  }
}

inline void check_operand(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, ": expected a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, ": expected bf16");
  TORCH_CHECK(t.dim() == 2 && t.is_contiguous(), name,
              ": expected a contiguous 2-D tensor");
  TORCH_CHECK(t.size(0) > 0 && t.size(0) % 8 == 0 && t.size(1) > 0 &&
                  t.size(1) % 8 == 0,
              name, ": both sizes must be positive multiples of 8, got ",
              t.sizes());
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              ": data must be 16-byte aligned");
}

inline dim3 tile_grid(long M, long N) {
  const long gx = (N + MB_TILE - 1) / MB_TILE;
  const long gy = (M + MB_TILE * MB_ROW_ITERS - 1) / (MB_TILE * MB_ROW_ITERS);
  TORCH_CHECK(gy <= 65535, "mlp_bwd: too many rows for one launch");
  return dim3((unsigned)gx, (unsigned)gy);
}

inline bf16_t* bptr(const at::Tensor& t) {
  return reinterpret_cast<bf16_t*>(t.data_ptr());
}

// mlp_bwd.hip.  want_store=false returns an empty xT; want_sum=false an
// empty colsum.  With `dst` defined the transpose is stored there instead of
// into a fresh tensor: a contiguous [N, M] bf16 view, for instance a row
// slice of a larger [*, M] buffer.
std::vector<at::Tensor> transpose_colsum_impl(
    const at::Tensor& x, bool want_sum, bool want_store,
    const c10::optional<at::Tensor>& dst = c10::nullopt);

}  // namespace samd
