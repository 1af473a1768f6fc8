// Fused multi-tensor SGD / Adam for CDNA4.
//
// One launch updates up to MAX_T parameter tensors; the pointer table rides
// in the kernel-argument block (no host->device metadata copies).  The
// element space is walked in 8-element groups (16 B of bf16 per lane —
// guide G13: scalar bf16 loads cost ~2-2.5x) with per-tensor scalar tails;
// grids are capped and grid-stride per guide Guideline 11.
//
// Replaces the reference's stock torch.optim.SGD step
// (examples/wikitext103/simple-verification.py:59) with the fused kernel
// the north star requires.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <vector>

#include "common.h"
#include "ops.h"

namespace samd {

constexpr int MAX_T = 32;
constexpr int GRP = 8;  // elements per group (16 B of bf16)

typedef __attribute__((ext_vector_type(8))) short short8v_;
typedef __attribute__((ext_vector_type(4))) float float4v_;

struct SgdArgs {
  void* p[MAX_T];
  void* g[MAX_T];
  void* m[MAX_T];       // momentum buffers (fp32; nullptr set if unused)
  void* w[MAX_T];       // fp32 master weights (nullptr set if unused)
  long cum[MAX_T + 1];  // cumulative GROUP counts
  long numel[MAX_T];
  int n_tensors;
  float lr, momentum, weight_decay;
  const float* scale;   // {norm, coef, ...} from clip_coef (HAS_S only)
};

// Gradient scale from clip_coef's output: false when the step is skipped
// (non-finite norm).  The multiply by coef is kept out of fp contraction:
// g * coef is rounded on its own, as clip_grad_norm_ followed by the
// optimizer rounds it, and coef == 1 leaves every later operation the one
// the unscaled kernel does.
__device__ __forceinline__ bool load_grad_scale(const float* scale,
                                                float& coef) {
  const float norm = scale[0];
  coef = scale[1];
  return (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
}
__device__ __forceinline__ float scale_grad(float g, float coef) {
#pragma clang fp contract(off)
  return g * coef;
}

template <typename T, bool HAS_M, bool HAS_W, bool HAS_S>
__device__ __forceinline__ void sgd_elem(T* p, const T* g, float* m, float* w,
                                         long j, const SgdArgs& a,
                                         float coef) {
  // HAS_W: the fp32 master is the source of truth; p gets the rounded copy.
  float pv = HAS_W ? w[j] : toF<T>(p[j]);
  float gv = toF<T>(g[j]);
  if (HAS_S) gv = scale_grad(gv, coef);
  if (a.weight_decay != 0.f) gv += a.weight_decay * pv;
  if (HAS_M) {
    float mv = m[j] * a.momentum + gv;
    m[j] = mv;
    gv = mv;
  }
  float nv = pv - a.lr * gv;
  if (HAS_W) w[j] = nv;
  p[j] = fromF<T>(nv);
}

template <typename T, bool HAS_M, bool HAS_W, bool HAS_S>
__global__ void fused_sgd_kernel(SgdArgs a) {
  float coef = 1.f;
  if constexpr (HAS_S) {
    if (!load_grad_scale(a.scale, coef)) return;
  }
  const long total = a.cum[a.n_tensors];  // total groups
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < MAX_T; ++k)
      if (k < a.n_tensors && i >= a.cum[k + 1]) t = k + 1;
    const long grp = i - a.cum[t];
    const long base = grp * GRP;
    T* p = reinterpret_cast<T*>(a.p[t]);
    const T* g = reinterpret_cast<const T*>(a.g[t]);
    float* m = HAS_M ? reinterpret_cast<float*>(a.m[t]) : nullptr;
    float* w = HAS_W ? reinterpret_cast<float*>(a.w[t]) : nullptr;
    const long n = a.numel[t];
    if constexpr (sizeof(T) == 2) {
      if (base + GRP <= n) {
        // vector path: 8 x 16-bit in one 16-B load/store
        short8v_ pv = *reinterpret_cast<short8v_*>(p + base);
        short8v_ gv = *reinterpret_cast<const short8v_*>(g + base);
        float4v_ m0, m1, w0, w1;
        if (HAS_M) {
          m0 = *reinterpret_cast<float4v_*>(m + base);
          m1 = *reinterpret_cast<float4v_*>(m + base + 4);
        }
        if (HAS_W) {
          w0 = *reinterpret_cast<float4v_*>(w + base);
          w1 = *reinterpret_cast<float4v_*>(w + base + 4);
        }
#pragma unroll
        for (int e = 0; e < GRP; ++e) {
          T pe, ge;
          pe.x = (unsigned short)pv[e];
          ge.x = (unsigned short)gv[e];
          float pf = HAS_W ? (e < 4 ? w0[e] : w1[e - 4]) : toF<T>(pe);
          float gf = toF<T>(ge);
          if (HAS_S) gf = scale_grad(gf, coef);
          if (a.weight_decay != 0.f) gf += a.weight_decay * pf;
          if (HAS_M) {
            float mv = (e < 4 ? m0[e] : m1[e - 4]) * a.momentum + gf;
            if (e < 4) m0[e] = mv; else m1[e - 4] = mv;
            gf = mv;
          }
          float nf = pf - a.lr * gf;
          if (HAS_W) {
            if (e < 4) w0[e] = nf; else w1[e - 4] = nf;
          }
          T out = fromF<T>(nf);
          pv[e] = (short)out.x;
        }
        *reinterpret_cast<short8v_*>(p + base) = pv;
        if (HAS_M) {
          *reinterpret_cast<float4v_*>(m + base) = m0;
          *reinterpret_cast<float4v_*>(m + base + 4) = m1;
        }
        if (HAS_W) {
          *reinterpret_cast<float4v_*>(w + base) = w0;
          *reinterpret_cast<float4v_*>(w + base + 4) = w1;
        }
      } else {
        for (long j = base; j < n; ++j)
          sgd_elem<T, HAS_M, HAS_W, HAS_S>(p, g, m, w, j, a, coef);
      }
    } else {
      const long end = (base + GRP <= n) ? base + GRP : n;
      for (long j = base; j < end; ++j)
        sgd_elem<T, HAS_M, HAS_W, HAS_S>(p, g, m, w, j, a, coef);
    }
  }
}

struct AdamArgs {
  void* p[MAX_T];
  void* g[MAX_T];
  void* m[MAX_T];
  void* v[MAX_T];
  void* w[MAX_T];  // fp32 master weights (nullptr set if unused)
  long cum[MAX_T + 1];
  long numel[MAX_T];
  int n_tensors;
  float lr, beta1, beta2, eps, weight_decay, bc1, bc2;
  const float* scale;  // {norm, coef, ...} from clip_coef (HAS_S only)
};

template <typename T, bool HAS_W, bool HAS_S>
__device__ __forceinline__ void adam_elem(T* p, const T* g, float* m, float* v,
                                          float* w, long j, const AdamArgs& a,
                                          float inv_bc1, float inv_bc2,
                                          float coef) {
  float gv = toF<T>(g[j]);
  if (HAS_S) gv = scale_grad(gv, coef);
  float mv = a.beta1 * m[j] + (1.f - a.beta1) * gv;
  float vv = a.beta2 * v[j] + (1.f - a.beta2) * gv * gv;
  m[j] = mv;
  v[j] = vv;
  float denom = sqrtf(vv * inv_bc2) + a.eps;
  float upd = (mv * inv_bc1) / denom;
  float pv = HAS_W ? w[j] : toF<T>(p[j]);
  if (a.weight_decay != 0.f) pv *= (1.f - a.lr * a.weight_decay);
  float nv = pv - a.lr * upd;
  if (HAS_W) w[j] = nv;
  p[j] = fromF<T>(nv);
}

template <typename T, bool HAS_W, bool HAS_S>
__global__ void fused_adam_kernel(AdamArgs a) {
  float coef = 1.f;
  if constexpr (HAS_S) {
    if (!load_grad_scale(a.scale, coef)) return;
  }
  const long total = a.cum[a.n_tensors];
  const long stride = (long)gridDim.x * blockDim.x;
  const float inv_bc1 = 1.f / a.bc1;
  const float inv_bc2 = 1.f / a.bc2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total;
       i += stride) {
    int t = 0;
#pragma unroll
    for (int k = 0; k < MAX_T; ++k)
      if (k < a.n_tensors && i >= a.cum[k + 1]) t = k + 1;
    const long grp = i - a.cum[t];
    const long base = grp * GRP;
    T* p = reinterpret_cast<T*>(a.p[t]);
    const T* g = reinterpret_cast<const T*>(a.g[t]);
    float* m = reinterpret_cast<float*>(a.m[t]);
    float* v = reinterpret_cast<float*>(a.v[t]);
    float* w = HAS_W ? reinterpret_cast<float*>(a.w[t]) : nullptr;
    const long n = a.numel[t];
    if constexpr (sizeof(T) == 2) {
      if (base + GRP <= n) {
        // 16-B loads on p/g; moments are fp32 (2x16-B each)
        short8v_ pv = *reinterpret_cast<short8v_*>(p + base);
        short8v_ gv = *reinterpret_cast<const short8v_*>(g + base);
        float4v_ m0 = *reinterpret_cast<float4v_*>(m + base);
        float4v_ m1 = *reinterpret_cast<float4v_*>(m + base + 4);
        float4v_ v0 = *reinterpret_cast<float4v_*>(v + base);
        float4v_ v1 = *reinterpret_cast<float4v_*>(v + base + 4);
        float4v_ w0, w1;
        if (HAS_W) {
          w0 = *reinterpret_cast<float4v_*>(w + base);
          w1 = *reinterpret_cast<float4v_*>(w + base + 4);
        }
#pragma unroll
        for (int e = 0; e < GRP; ++e) {
          T ge;
          ge.x = (unsigned short)gv[e];
          float gf = toF<T>(ge);
          if (HAS_S) gf = scale_grad(gf, coef);
          float mv = a.beta1 * (e < 4 ? m0[e] : m1[e - 4]) + (1.f - a.beta1) * gf;
          float vv = a.beta2 * (e < 4 ? v0[e] : v1[e - 4]) + (1.f - a.beta2) * gf * gf;
          if (e < 4) { m0[e] = mv; v0[e] = vv; } else { m1[e-4] = mv; v1[e-4] = vv; }
          float denom = sqrtf(vv * inv_bc2) + a.eps;
          float upd = (mv * inv_bc1) / denom;
          T pe;
          pe.x = (unsigned short)pv[e];
          float pf = HAS_W ? (e < 4 ? w0[e] : w1[e - 4]) : toF<T>(pe);
          if (a.weight_decay != 0.f) pf *= (1.f - a.lr * a.weight_decay);
          float nf = pf - a.lr * upd;
          if (HAS_W) {
            if (e < 4) w0[e] = nf; else w1[e - 4] = nf;
          }
          T out = fromF<T>(nf);
          pv[e] = (short)out.x;
        }
        *reinterpret_cast<short8v_*>(p + base) = pv;
        *reinterpret_cast<float4v_*>(m + base) = m0;
        *reinterpret_cast<float4v_*>(m + base + 4) = m1;
        *reinterpret_cast<float4v_*>(v + base) = v0;
        *reinterpret_cast<float4v_*>(v + base + 4) = v1;
        if (HAS_W) {
          *reinterpret_cast<float4v_*>(w + base) = w0;
          *reinterpret_cast<float4v_*>(w + base + 4) = w1;
        }
      } else {
        for (long j = base; j < n; ++j)
          adam_elem<T, HAS_W, HAS_S>(p, g, m, v, w, j, a, inv_bc1, inv_bc2, coef);
      }
    } else {
      const long end = (base + GRP <= n) ? base + GRP : n;
      for (long j = base; j < end; ++j)
        adam_elem<T, HAS_W, HAS_S>(p, g, m, v, w, j, a, inv_bc1, inv_bc2, coef);
    }
  }
}

static int grid_for(long total, int block) {
  // HBM-bound sweep: more resident blocks = more outstanding loads (the
  // 2048 cap measured 4.9 TB/s on the 6B update; 4096 keeps every CU at
  // 2 blocks with a 16-deep grid-stride)
  long g = (total + block - 1) / block;
  return (int)std::min<long>(std::max<long>(g, 1), 4096);
}

static long groups_of(long numel) { return (numel + GRP - 1) / GRP; }

// clip_coef's output tensor, or nullptr when the step is not clipped
static const float* grad_scale_ptr(const c10::optional<at::Tensor>& gs,
                                   const at::Tensor& like) {
  if (!gs.has_value()) return nullptr;
  TORCH_CHECK(gs->scalar_type() == at::kFloat && gs->numel() >= 2 &&
                  gs->is_contiguous() && gs->device() == like.device(),
              "grad_scale must be clip_coef's fp32 output on the parameters' "
              "device");
  return gs->data_ptr<float>();
}

template <typename scalar_t>
static void sgd_launch(std::vector<at::Tensor>& params,
                       std::vector<at::Tensor>& grads,
                       std::vector<at::Tensor>& moms,
                       std::vector<at::Tensor>& masters, double lr,
                       double momentum, double weight_decay,
                       const float* scale) {
  auto stream = at::hip::getCurrentHIPStream();
  const bool has_m = !moms.empty();
  const bool has_w = !masters.empty();
  for (size_t base = 0; base < params.size(); base += MAX_T) {
    SgdArgs a{};
    a.n_tensors = (int)std::min<size_t>(MAX_T, params.size() - base);
    a.lr = (float)lr;
    a.momentum = (float)momentum;
    a.weight_decay = (float)weight_decay;
    a.scale = scale;
    long cum = 0;
    a.cum[0] = 0;
    for (int k = 0; k < a.n_tensors; ++k) {
      a.p[k] = params[base + k].data_ptr();
      a.g[k] = grads[base + k].data_ptr();
      a.m[k] = has_m ? moms[base + k].data_ptr() : nullptr;
      a.w[k] = has_w ? masters[base + k].data_ptr() : nullptr;
      a.numel[k] = params[base + k].numel();
      cum += groups_of(a.numel[k]);
      a.cum[k + 1] = cum;
    }
    const int block = 256;
    dim3 grid(grid_for(cum, block));
#define SAMD_SGD_LAUNCH(M, W, S)                                          \
  hipLaunchKernelGGL((fused_sgd_kernel<scalar_t, M, W, S>), grid,         \
                     dim3(block), 0, stream.stream(), a)
#define SAMD_SGD_MW(S)                                                    \
  do {                                                                    \
    if (has_m && has_w) SAMD_SGD_LAUNCH(true, true, S);                   \
    else if (has_m) SAMD_SGD_LAUNCH(true, false, S);                      \
    else if (has_w) SAMD_SGD_LAUNCH(false, true, S);                      \
    else SAMD_SGD_LAUNCH(false, false, S);                                \
  } while (0)
    if (scale != nullptr) SAMD_SGD_MW(true);
    else SAMD_SGD_MW(false);
#undef SAMD_SGD_MW
#undef SAMD_SGD_LAUNCH
  }
}

void fused_sgd(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
               std::vector<at::Tensor> moms, std::vector<at::Tensor> masters,
               double lr, double momentum, double weight_decay,
               c10::optional<at::Tensor> grad_scale) {
  TORCH_CHECK(!params.empty(), "no params");
  TORCH_CHECK(params.size() == grads.size());
  TORCH_CHECK(moms.empty() || moms.size() == params.size());
  TORCH_CHECK(masters.empty() || masters.size() == params.size());
  for (size_t i = 0; i < params.size(); ++i) {
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous());
    TORCH_CHECK(params[i].scalar_type() == grads[i].scalar_type());
    if (!moms.empty())
      TORCH_CHECK(moms[i].scalar_type() == at::kFloat,
                  "momentum buffers must be fp32");
    if (!masters.empty())
      TORCH_CHECK(masters[i].scalar_type() == at::kFloat &&
                      masters[i].is_contiguous(),
                  "master weights must be contiguous fp32");
  }
  const float* scale = grad_scale_ptr(grad_scale, params[0]);
  switch (params[0].scalar_type()) {
    case at::kBFloat16:
      sgd_launch<c10::BFloat16>(params, grads, moms, masters, lr, momentum,
                                weight_decay, scale);
      break;
    case at::kFloat:
      sgd_launch<float>(params, grads, moms, masters, lr, momentum,
                        weight_decay, scale);
      break;
    case at::kHalf:
      sgd_launch<c10::Half>(params, grads, moms, masters, lr, momentum,
                            weight_decay, scale);
      break;
    default:
      TORCH_CHECK(false, "fused_sgd: unsupported dtype");
  }
}

template <typename scalar_t>
static void adam_launch(std::vector<at::Tensor>& params,
                        std::vector<at::Tensor>& grads,
                        std::vector<at::Tensor>& ms,
                        std::vector<at::Tensor>& vs,
                        std::vector<at::Tensor>& masters, double lr,
                        double beta1, double beta2, double eps,
                        double weight_decay, double bc1, double bc2,
                        const float* scale) {
  auto stream = at::hip::getCurrentHIPStream();
  const bool has_w = !masters.empty();
  for (size_t base = 0; base < params.size(); base += MAX_T) {
    AdamArgs a{};
    a.n_tensors = (int)std::min<size_t>(MAX_T, params.size() - base);
    a.lr = (float)lr;
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.eps = (float)eps;
    a.weight_decay = (float)weight_decay;
    a.bc1 = (float)bc1;
    a.bc2 = (float)bc2;
    a.scale = scale;
    long cum = 0;
    a.cum[0] = 0;
    for (int k = 0; k < a.n_tensors; ++k) {
      a.p[k] = params[base + k].data_ptr();
      a.g[k] = grads[base + k].data_ptr();
      a.m[k] = ms[base + k].data_ptr();
      a.v[k] = vs[base + k].data_ptr();
      a.w[k] = has_w ? masters[base + k].data_ptr() : nullptr;
      a.numel[k] = params[base + k].numel();
      cum += groups_of(a.numel[k]);
      a.cum[k + 1] = cum;
    }
    const int block = 256;
    dim3 grid(grid_for(cum, block));
    if (scale != nullptr) {
      if (has_w)
        hipLaunchKernelGGL((fused_adam_kernel<scalar_t, true, true>), grid,
                           dim3(block), 0, stream.stream(), a);
      else
        hipLaunchKernelGGL((fused_adam_kernel<scalar_t, false, true>), grid,
                           dim3(block), 0, stream.stream(), a);
    } else if (has_w) {
      hipLaunchKernelGGL((fused_adam_kernel<scalar_t, true, false>), grid,
                         dim3(block), 0, stream.stream(), a);
    } else {
      hipLaunchKernelGGL((fused_adam_kernel<scalar_t, false, false>), grid,
                         dim3(block), 0, stream.stream(), a);
    }
  }
}

void fused_adam(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                std::vector<at::Tensor> ms, std::vector<at::Tensor> vs,
                std::vector<at::Tensor> masters, double lr, double beta1,
                double beta2, double eps, double weight_decay, double bc1,
                double bc2, c10::optional<at::Tensor> grad_scale) {
  TORCH_CHECK(!params.empty(), "no params");
  TORCH_CHECK(params.size() == grads.size() && params.size() == ms.size() &&
              params.size() == vs.size());
  TORCH_CHECK(masters.empty() || masters.size() == params.size());
  for (size_t i = 0; i < params.size(); ++i) {
    TORCH_CHECK(params[i].is_contiguous() && grads[i].is_contiguous());
    TORCH_CHECK(ms[i].scalar_type() == at::kFloat &&
                vs[i].scalar_type() == at::kFloat,
                "Adam moments must be fp32");
    if (!masters.empty())
      TORCH_CHECK(masters[i].scalar_type() == at::kFloat &&
                      masters[i].is_contiguous(),
                  "master weights must be contiguous fp32");
  }
  const float* scale = grad_scale_ptr(grad_scale, params[0]);
  switch (params[0].scalar_type()) {
    case at::kBFloat16:
      adam_launch<c10::BFloat16>(params, grads, ms, vs, masters, lr, beta1,
                                 beta2, eps, weight_decay, bc1, bc2, scale);
      break;
    case at::kFloat:
      adam_launch<float>(params, grads, ms, vs, masters, lr, beta1, beta2,
                         eps, weight_decay, bc1, bc2, scale);
      break;
    default:
      TORCH_CHECK(false, "fused_adam: unsupported dtype");
  }
}

}  // namespace samd
