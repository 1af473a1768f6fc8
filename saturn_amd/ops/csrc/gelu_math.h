// tanh-approx GELU value and derivative, shared by gelu.hip and mlp_bwd.hip
// so both compile the same expressions (the fused MLP backward must
// reproduce gelu_kernel's outputs bit for bit).
//
// gelu(x)  = 0.5 x (1 + tanh(k (x + c x^3))),  k = sqrt(2/pi), c = 0.044715
// dgelu/dx = 0.5 (1 + t) + 0.5 x (1 - t^2) k (1 + 3 c x^2),  t = tanh(...)
//
// tanh via the fast exp intrinsic: tanh(u) = 1 - 2 / (exp(2u) + 1).
#pragma once

#include <hip/hip_runtime.h>

namespace samd {

__device__ __forceinline__ float tanh_fast(float u) {
  return 1.f - 2.f / (__expf(2.f * u) + 1.f);
}

constexpr float GK = 0.7978845608028654f;  // sqrt(2/pi)
constexpr float GC = 0.044715f;

__device__ __forceinline__ float gelu_f(float x) {
  const float t = tanh_fast(GK * (x + GC * x * x * x));
  return 0.5f * x * (1.f + t);
}

__device__ __forceinline__ float dgelu_f(float x) {
  const float u = GK * (x + GC * x * x * x);
  const float t = tanh_fast(u);
  const float du = GK * (1.f + 3.f * GC * x * x);
  return 0.5f * (1.f + t) + 0.5f * x * (1.f - t * t) * du;
}

}  // namespace samd
