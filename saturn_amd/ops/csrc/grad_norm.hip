// Global gradient-norm reduction and clip coefficient for CDNA4 (K16).
//
// grad_sqsum: sum of squares over a tensor list, fp32.  The list is walked
// the way fused_optim.hip walks it: a pointer table of up to MAX_T tensors
// in the kernel-argument block, 8-element groups (one 16-B load of bf16/fp16,
// two of fp32), per-tensor scalar tails, capped grid with a grid-stride loop.
// Being read-only it has a third of the SGD kernel's bytes per group to hide
// the table lookup behind, so the table is copied to LDS once per block and
// four grid-stride trips are loaded before the first is added.
// Each thread keeps one fp32 accumulator, the block reduces it with
// block_sum, and thread 0 stores the block's partial into the block's own
// slot of a caller-owned buffer.  A second one-block kernel adds the used
// slots in fp64 in a fixed order.  There are no atomics, and which thread
// adds which element in which order depends only on the tensor sizes, so the
// result is bitwise reproducible — also between a tensor and a copy of it
// at another alignment: a tensor whose data pointer is not 16-B aligned
// takes scalar loads for the same groups, added in the same order.
//
// clip_coef: one thread turns the (possibly all-reduced) squared sum into
// out = {norm, coef, skipped_total}.  A non-finite squared sum gives a
// non-finite norm; that is the skip flag the optimizer kernels test.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <cstdint>
#include <utility>
#include <vector>

#include "common.h"
#include "ops.h"

namespace samd {

namespace {

constexpr int SQ_MAX_T = 32;
constexpr int SQ_GRP = 8;
constexpr int SQ_BLOCK = 256;
constexpr int SQ_GRID_CAP = 4096;
constexpr int SQ_UNROLL = 4;  // grid-stride trips in flight per thread
constexpr int FIN_BLOCK = 256;

struct SqArgs {
  const void* g[SQ_MAX_T];
  long cum[SQ_MAX_T + 1];  // cumulative GROUP counts
  long numel[SQ_MAX_T];
  unsigned aligned;        // bit k: g[k] is 16-B aligned
  int n_tensors;
  float* partials;         // this launch's first slot
};

// One group's 8 elements as loaded: 16 B of a 2-byte type, 32 B of fp32.
template <typename T, int BYTES = sizeof(T)>
struct SqGroup {
  short8v v;
  __device__ __forceinline__ void load(const T* g) {
    v = *reinterpret_cast<const short8v*>(g);
  }
  __device__ __forceinline__ float at(int e) const {
    T x;
    x.x = (unsigned short)v[e];
    return toF<T>(x);
  }
};
template <typename T>
struct SqGroup<T, 4> {
  float4v v0, v1;
  __device__ __forceinline__ void load(const T* g) {
    v0 = *reinterpret_cast<const float4v*>(g);
    v1 = *reinterpret_cast<const float4v*>(g + 4);
  }
  __device__ __forceinline__ float at(int e) const {
    return e < 4 ? v0[e] : v1[e - 4];
  }
};

template <typename T>
__global__ void __launch_bounds__(SQ_BLOCK) grad_sqsum_kernel(SqArgs a) {
  __shared__ float lds[SQ_BLOCK / WAVE];
  // The tensor table moves to LDS once per block.  Indexing the kernel
  // arguments by a per-lane tensor number costs a compare-and-select chain
  // over all SQ_MAX_T entries per group, which made this read-only sweep
  // VALU-bound; a group's tensor is found by walking forward from the
  // previous group's instead (a thread's groups only move forward).
  __shared__ long s_cum[SQ_MAX_T + 1];
  __shared__ long s_numel[SQ_MAX_T];
  __shared__ const void* s_ptr[SQ_MAX_T];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < SQ_MAX_T; ++k) {
      s_cum[k] = a.cum[k];
      s_numel[k] = a.numel[k];
      s_ptr[k] = a.g[k];
    }
    s_cum[SQ_MAX_T] = a.cum[SQ_MAX_T];
  }
  __syncthreads();
  const int last = a.n_tensors - 1;
  const long total = s_cum[a.n_tensors];
  const long stride = (long)gridDim.x * blockDim.x;
  float acc = 0.f;
  int t = 0;
  // SQ_UNROLL grid-stride trips at a time: all their vector loads are issued
  // before the first is added (one 16-B load in flight per lane leaves the
  // sweep latency-bound).  The thread still adds its groups in trip order,
  // and every path adds element e of a group as acc = fma(x, x, acc) in
  // element order, so vector and scalar loads give the same bits.
  for (long i0 = blockIdx.x * (long)blockDim.x + threadIdx.x; i0 < total;
       i0 += stride * SQ_UNROLL) {
    SqGroup<T> grp[SQ_UNROLL];
    const T* gp[SQ_UNROLL];
    long base[SQ_UNROLL], n[SQ_UNROLL];
    bool vec[SQ_UNROLL];
#pragma unroll
    for (int u = 0; u < SQ_UNROLL; ++u) {
      const long i = i0 + u * stride;
      vec[u] = false;
      n[u] = 0;
      base[u] = 0;
      gp[u] = nullptr;
      if (i < total) {
        while (t < last && i >= s_cum[t + 1]) ++t;  // i < total = cum[last+1]
        base[u] = (i - s_cum[t]) * SQ_GRP;
        gp[u] = reinterpret_cast<const T*>(s_ptr[t]);
        n[u] = s_numel[t];
        vec[u] = base[u] + SQ_GRP <= n[u] && ((a.aligned >> t) & 1u);
        if (vec[u]) grp[u].load(gp[u] + base[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < SQ_UNROLL; ++u) {
      if (vec[u]) {
#pragma unroll
        for (int e = 0; e < SQ_GRP; ++e) {
          const float x = grp[u].at(e);
          acc = fmaf(x, x, acc);
        }
      } else {
        // tail of a tensor, or a tensor that is not 16-B aligned (n = 0
        // past the end of the list: nothing to add)
        const long end = (base[u] + SQ_GRP <= n[u]) ? base[u] + SQ_GRP : n[u];
        for (long j = base[u]; j < end; ++j) {
          const float x = toF<T>(gp[u][j]);
          acc = fmaf(x, x, acc);
        }
      }
    }
  }
  const float s = block_sum<SQ_BLOCK>(acc, lds);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
}

// One block: fp64 sum of the used slots, each thread over a fixed strided
// subset, then a fixed LDS tree.  fp64 keeps this stage out of the fp32
// error budget however many slots a long tensor list uses.
__global__ void __launch_bounds__(FIN_BLOCK)
grad_sqsum_final_kernel(const float* __restrict__ partials, int n_used,
                        float* __restrict__ out) {
  __shared__ double lds[FIN_BLOCK];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_used; i += FIN_BLOCK)
    acc += (double)partials[i];
  lds[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int off = FIN_BLOCK / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) lds[threadIdx.x] += lds[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = (float)lds[0];
}

__global__ void clip_coef_kernel(const float* __restrict__ sq, float max_norm,
                                 float* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const float s = sq[0];
  const float norm = sqrtf(s);  // inf -> inf, nan -> nan: the skip flag
  const bool finite =
      (__float_as_uint(s) & 0x7f800000u) != 0x7f800000u;
  float coef = 0.f;
  if (finite) coef = fminf(1.f, max_norm / (norm + 1e-6f));
  out[0] = norm;
  out[1] = coef;
  if (!finite) out[2] = out[2] + 1.f;
}

long sq_groups_of(long numel) { return (numel + SQ_GRP - 1) / SQ_GRP; }

int sq_grid_for(long groups) {
  const long g = (groups + SQ_BLOCK - 1) / SQ_BLOCK;
  return (int)std::min<long>(std::max<long>(g, 1), SQ_GRID_CAP);
}

// The launch rule: one launch per SQ_MAX_T tensors, in list order.
std::vector<std::pair<int64_t, int64_t>> sq_plan(
    const std::vector<int64_t>& numels) {
  std::vector<std::pair<int64_t, int64_t>> plan;
  for (size_t base = 0; base < numels.size(); base += SQ_MAX_T) {
    const size_t n = std::min<size_t>(SQ_MAX_T, numels.size() - base);
    long groups = 0;
    for (size_t k = 0; k < n; ++k) groups += sq_groups_of(numels[base + k]);
    plan.emplace_back(sq_grid_for(groups), SQ_BLOCK);
  }
  return plan;
}

template <typename scalar_t>
void sqsum_launch(const std::vector<at::Tensor>& ts, float* partials,
                  hipStream_t stream) {
  int slot = 0;
  for (size_t base = 0; base < ts.size(); base += SQ_MAX_T) {
    SqArgs a{};
    a.n_tensors = (int)std::min<size_t>(SQ_MAX_T, ts.size() - base);
    long cum = 0;
    a.cum[0] = 0;
    for (int k = 0; k < a.n_tensors; ++k) {
      const at::Tensor& t = ts[base + k];
      a.g[k] = t.data_ptr();
      a.numel[k] = t.numel();
      if ((reinterpret_cast<uintptr_t>(a.g[k]) & 15u) == 0)
        a.aligned |= 1u << k;
      cum += sq_groups_of(a.numel[k]);
      a.cum[k + 1] = cum;
    }
    a.partials = partials + slot;
    const int grid = sq_grid_for(cum);
    hipLaunchKernelGGL((grad_sqsum_kernel<scalar_t>), dim3(grid),
                       dim3(SQ_BLOCK), 0, stream, a);
    slot += grid;
  }
}

}  // namespace

std::vector<std::pair<int64_t, int64_t>> grad_sqsum_plan(
    std::vector<int64_t> numels) {
  return sq_plan(numels);
}

int64_t grad_sqsum_slots(int64_t n_tensors) {
  // slots a list of n_tensors can use at most: launches x grid cap
  const int64_t launches = (n_tensors + SQ_MAX_T - 1) / SQ_MAX_T;
  return std::max<int64_t>(launches, 1) * SQ_GRID_CAP;
}

at::Tensor grad_sqsum(std::vector<at::Tensor> tensors, at::Tensor partials) {
  TORCH_CHECK(partials.is_cuda() && partials.scalar_type() == at::kFloat &&
                  partials.is_contiguous(),
              "grad_sqsum: partials must be a contiguous fp32 device tensor");
  std::vector<int64_t> numels;
  numels.reserve(tensors.size());
  for (const at::Tensor& t : tensors) {
    TORCH_CHECK(t.is_cuda() && t.device() == partials.device(),
                "grad_sqsum: tensors and partials must share a device");
    TORCH_CHECK(t.is_contiguous(), "grad_sqsum: tensors must be contiguous");
    TORCH_CHECK(t.scalar_type() == tensors[0].scalar_type(),
                "grad_sqsum: one dtype per call");
    numels.push_back(t.numel());
  }
  int64_t used = 0;
  for (const auto& l : sq_plan(numels)) used += l.first;
  TORCH_CHECK(partials.numel() >= used, "grad_sqsum: partials holds ",
              partials.numel(), " slots, the list needs ", used);
  auto stream = at::hip::getCurrentHIPStream().stream();
  at::Tensor out = at::empty({1}, partials.options());
  float* pp = partials.data_ptr<float>();
  if (!tensors.empty()) {
    switch (tensors[0].scalar_type()) {
      case at::kBFloat16:
        sqsum_launch<c10::BFloat16>(tensors, pp, stream);
        break;
      case at::kHalf:
        sqsum_launch<c10::Half>(tensors, pp, stream);
        break;
      case at::kFloat:
        sqsum_launch<float>(tensors, pp, stream);
        break;
      default:
        TORCH_CHECK(false, "grad_sqsum: unsupported dtype");
    }
  }
  hipLaunchKernelGGL(grad_sqsum_final_kernel, dim3(1), dim3(FIN_BLOCK), 0,
                     stream, pp, (int)used, out.data_ptr<float>());
  return out;
}

void clip_coef(at::Tensor sq, double max_norm, at::Tensor out) {
  TORCH_CHECK(sq.is_cuda() && sq.scalar_type() == at::kFloat &&
                  sq.numel() == 1,
              "clip_coef: sq must be one fp32 element on the device");
  TORCH_CHECK(out.is_cuda() && out.device() == sq.device() &&
                  out.scalar_type() == at::kFloat && out.numel() == 3 &&
                  out.is_contiguous(),
              "clip_coef: out must be fp32[3] on sq's device");
  auto stream = at::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(64), 0, stream,
                     sq.data_ptr<float>(), (float)max_norm,
                     out.data_ptr<float>());
}

}  // namespace samd
