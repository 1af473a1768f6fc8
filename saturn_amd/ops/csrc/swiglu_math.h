// SwiGLU value and derivatives, shared by swiglu.hip and llama_mlp_bwd.hip so
// both compile the same expressions (the fused Llama MLP backward must
// reproduce swiglu_fwd_kernel's and swiglu_bwd_kernel's 16-bit vector paths
// bit for bit).
//
// act    = silu(g) u,            silu(g) = g / (1 + exp(-g))
// d_gate = go u sig (1 + g (1 - sig)),   sig = 1 / (1 + exp(-g))
// d_up   = go g sig              (multiplied left to right, as written)
#pragma once

#include <hip/hip_runtime.h>

namespace samd {

__device__ __forceinline__ float silu_f(float x) {
  return x / (1.f + __expf(-x));
}

__device__ __forceinline__ float sigmoid_f(float g) {
  return 1.f / (1.f + __expf(-g));
}

// d silu(g)/dg = sig * (1 + g * (1 - sig))
__device__ __forceinline__ float swiglu_dgate_f(float go, float g, float u,
                                                float sig) {
  return go * u * sig * (1.f + g * (1.f - sig));
}

__device__ __forceinline__ float swiglu_dup_f(float go, float g, float sig) {
  return go * g * sig;
}

}  // namespace samd
