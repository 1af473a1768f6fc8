// Counter-based keep function of the attention dropout (attn_pdrop) and the
// splitmix64 finalizer it shares with dropout.hip (K6).
//
// Whether probability (b, h, i, j) is kept is a pure function of
// (seed, bh = b*H + h, query row i, key j) and nothing else — not the tile
// shape, the kernel, D, the layout or the padded length — so both forwards,
// the dK/dV kernel, the dQ kernel and the Python twin
// (saturn_amd/ops/flash.py: dropout_keep) agree bit for bit:
//
//   thr  = floor(p * 65536 + 0.5)              16-bit threshold
//   c    = (bh << 40) | (i << 20) | (j >> 2)   one draw per (row, 4 keys)
//   r64  = mix64(seed ^ c)
//   keep = ((r64 >> (16 * (j & 3))) & 0xffff) >= thr
//
// The three fields of c do not overlap while i, j < 2^20 and bh < 2^24 (the
// host checks both), so seed ^ c splits into a per-row part and the key
// group: a lane hashes once per four consecutive keys of one row.
// This header is the only place in the kernels that knows the function.
#pragma once

#include <hip/hip_runtime.h>

namespace samd {

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

constexpr int ATTN_RNG_MAX_T_LOG2 = 20;   // i, j < 2^20
constexpr int ATTN_RNG_MAX_BH_LOG2 = 24;  // bh < 2^24

// seed ^ the (bh, i) fields of the counter
__device__ __forceinline__ unsigned long long attn_rng_row(
    unsigned long long seed, long bh, int i) {
  return seed ^ ((unsigned long long)bh << 40) ^
         ((unsigned long long)(unsigned)i << 20);
}
// the 64-bit draw that covers key j (and the other keys of its aligned 4)
__device__ __forceinline__ unsigned long long attn_rng_draw(
    unsigned long long row_key, int j) {
  return mix64(row_key ^ (unsigned long long)((unsigned)j >> 2));
}
// key j's 16-bit field of its draw against the threshold
__device__ __forceinline__ bool attn_rng_keep(unsigned long long draw, int j,
                                              unsigned thr) {
  return ((unsigned)(draw >> (16 * (j & 3))) & 0xffffu) >= thr;
}
// the same for key j0 + f of an aligned group (j0 % 4 == 0, f = 0..3 a
// compile-time constant where the caller's loop is unrolled)
__device__ __forceinline__ bool attn_rng_keep4(unsigned long long draw, int f,
                                               unsigned thr) {
  return attn_rng_keep(draw, f, thr);
}

}  // namespace samd
