// MoE routing and token dispatch (K13): everything around the expert GEMMs
// of the Mixtral path (models/mixtral.py MoEMLP, parallel/expert.py).
//
//   route   softmax over E experts in fp32 -> top-k -> renormalise, one pass,
//           plus its backward (p recomputed from the logits)
//   sort    stable counting sort of the (token, slot) pairs by expert:
//           block histogram -> scan over [blocks, E] -> ballot ranking
//   permute xs[i] = x[order[i] / k]            (row gather, 16 B per lane)
//   combine out[t] = sum_j w[t,j] * y[pos[t,j]] (balanced gather through the
//           inverse index, fp32 accumulate, one rounding)
//
// No float atomics anywhere: every token has exactly k contributions, so
// each reduction is a fixed-order gather through `pos` (store-then-gather)
// and every result is bitwise reproducible.  The only atomics are integer
// LDS adds in the histogram, whose sum does not depend on arrival order.
//
// Ties in the selection go to the lower expert index: the top-k runs on the
// fp32 logits (softmax is monotone, so this is the order of the
// probabilities) with the comparator (value desc, index asc).
//
// Envelope (checked here, the Python wrapper falls back outside it):
// E <= 64, k <= min(8, E), hidden % 8 == 0, rows bf16/fp16/fp32,
// N*k < 2^31 with 64-bit row offsets.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "common.h"
#include "ops.h"

namespace samd {

namespace {

constexpr int MOE_BLOCK = 256;
constexpr int MOE_MAX_E = 64;
constexpr int MOE_MAX_K = 8;
// sort: each block ranks SORT_ITEMS passes of MOE_BLOCK consecutive pairs
constexpr int SORT_ITEMS = 8;
constexpr int SORT_CHUNK = MOE_BLOCK * SORT_ITEMS;

// 16-byte vector of T (8 x 16-bit or 4 x fp32): one dwordx4 per lane
template <typename T>
struct alignas(16) RowVec {
  static constexpr int N = 16 / sizeof(T);
  T v[N];
};

// reductions over a power-of-two group of G <= 64 adjacent lanes; every lane
// of the group ends with the result, and the order of the adds is fixed
__device__ __forceinline__ float group_sum(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, G);
  return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, G));
  return v;
}

inline int pow2_group(long n) {
  int g = 1;
  while (g < n && g < WAVE) g <<= 1;
  return g;
}

// ---------------------------------------------------------------------------
// routing: one lane per (row, expert), G = pow2 >= E lanes per row
// ---------------------------------------------------------------------------
template <typename TL, typename TW>
__global__ void moe_route_fwd_kernel(const TL* __restrict__ logits,
                                     TW* __restrict__ weights,
                                     int* __restrict__ ids, long N, int E,
                                     int K, int G) {
  const int sub = threadIdx.x & (G - 1);
  const long row = (blockIdx.x * (long)blockDim.x + threadIdx.x) / G;
  const bool real = sub < E;
  const bool live = real && row < N;
  const float x = live ? toF<TL>(logits[row * E + sub]) : -INFINITY;
  const float key = (x == x) ? x : -INFINITY;  // a NaN never wins
  const float m = group_max(key, G);
  // exp(x - m) / Z renormalised over the chosen k: Z cancels, so the
  // weights are e_j / sum_sel(e) with e = exp(x - m)
  const float ex = live ? expf(x - m) : 0.f;

  int slot = -1;
  for (int j = 0; j < K; ++j) {
    // lanes already taken (and the padding lanes) sort behind every free
    // real lane even at equal value, so the winner is always a valid id
    float v = slot >= 0 ? -INFINITY : key;
    int idx = (slot >= 0 || !real) ? sub + MOE_MAX_E : sub;
    for (int off = G >> 1; off > 0; off >>= 1) {
      const float ov = __shfl_xor(v, off, G);
      const int oi = __shfl_xor(idx, off, G);
      if (ov > v || (ov == v && oi < idx)) {
        v = ov;
        idx = oi;
      }
    }
    if (idx == sub) slot = j;
  }
  const float S = group_sum(slot >= 0 ? ex : 0.f, G);
  if (live && slot >= 0) {
    weights[row * K + slot] = fromF<TW>(ex / S);
    ids[row * K + slot] = sub;
  }
}

template <typename TL>
__global__ void moe_route_bwd_kernel(const TL* __restrict__ logits,
                                     const int* __restrict__ ids,
                                     const float* __restrict__ dweights,
                                     TL* __restrict__ dlogits, long N, int E,
                                     int K, int G) {
  const int sub = threadIdx.x & (G - 1);
  const long row = (blockIdx.x * (long)blockDim.x + threadIdx.x) / G;
  const bool live = sub < E && row < N;
  const float x = live ? toF<TL>(logits[row * E + sub]) : -INFINITY;
  const float m = group_max((x == x) ? x : -INFINITY, G);
  const float ex = live ? expf(x - m) : 0.f;
  const float p = ex / group_sum(ex, G);

  bool sel = false;
  float dw = 0.f;
  if (live) {
    for (int j = 0; j < K; ++j) {
      if (ids[row * K + j] == sub) {
        sel = true;
        dw = dweights[row * K + j];
      }
    }
  }
  // S = sum_sel p, w_j = p_j / S, g_j = (dw_j - sum_i dw_i w_i) / S
  const float S = group_sum(sel ? p : 0.f, G);
  const float w = sel ? p / S : 0.f;
  const float dot = group_sum(dw * w, G);
  const float g = sel ? (dw - dot) / S : 0.f;
  const float pg = group_sum(p * g, G);
  if (live) dlogits[row * E + sub] = fromF<TL>(p * (g - pg));
}

// ---------------------------------------------------------------------------
// stable counting sort of pairs by expert
// ---------------------------------------------------------------------------
__global__ void moe_hist_kernel(const int* __restrict__ ids,
                                int* __restrict__ blockhist, long P, int E) {
  __shared__ int h[MOE_MAX_E];
  if (threadIdx.x < MOE_MAX_E) h[threadIdx.x] = 0;
  __syncthreads();
  const long base = blockIdx.x * (long)SORT_CHUNK;
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const long p = base + it * MOE_BLOCK + threadIdx.x;
    if (p < P) {
      const int id = ids[p];
      if ((unsigned)id < (unsigned)E) atomicAdd(&h[id], 1);
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < E)
    blockhist[blockIdx.x * (long)E + threadIdx.x] = h[threadIdx.x];
}

// one block: blockhist[b, e] (counts) -> exclusive offsets in the sorted
// order (expert-major, then block), and the per-expert totals
__global__ void moe_scan_kernel(int* __restrict__ blockhist,
                                int* __restrict__ counts, int nb, int E) {
  __shared__ int seg[MOE_BLOCK];
  __shared__ int total[MOE_MAX_E];
  const int nseg = MOE_BLOCK / E;
  const int e = threadIdx.x % E;
  const int s = threadIdx.x / E;
  const bool active = s < nseg;
  const int per = (nb + nseg - 1) / nseg;
  const int b0 = min(s * per, nb);
  const int b1 = min(b0 + per, nb);
  int sum = 0;
  if (active)
    for (int b = b0; b < b1; ++b) sum += blockhist[b * (long)E + e];
  seg[threadIdx.x] = sum;
  __syncthreads();
  int pre = 0, tot = 0;
  if (active) {
    for (int s2 = 0; s2 < nseg; ++s2) {
      const int v = seg[s2 * E + e];
      if (s2 < s) pre += v;
      tot += v;
    }
    if (s == 0) {
      total[e] = tot;
      counts[e] = tot;
    }
  }
  __syncthreads();
  if (active) {
    int run = pre;
    for (int e2 = 0; e2 < e; ++e2) run += total[e2];
    for (int b = b0; b < b1; ++b) {
      const long i = b * (long)E + e;
      const int v = blockhist[i];
      blockhist[i] = run;
      run += v;
    }
  }
}

// rank of a pair inside its block = pairs of the same expert in earlier
// passes + in earlier waves of this pass + in lower lanes of this wave
// (ballot popcount): lane and wave order, never arrival order
__global__ void moe_rank_kernel(const int* __restrict__ ids,
                                const int* __restrict__ blockoff,
                                int* __restrict__ order, int* __restrict__ pos,
                                long P, int E) {
  constexpr int NW = MOE_BLOCK / WAVE;
  __shared__ int base[MOE_MAX_E];
  __shared__ int wcnt[NW][MOE_MAX_E];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const unsigned long long lt = (1ull << lane) - 1ull;
  if ((int)threadIdx.x < E)
    base[threadIdx.x] = blockoff[blockIdx.x * (long)E + threadIdx.x];
  __syncthreads();
  const long chunk = blockIdx.x * (long)SORT_CHUNK;
  for (int it = 0; it < SORT_ITEMS; ++it) {
    const long p = chunk + it * MOE_BLOCK + threadIdx.x;
    int id = -1;
    if (p < P) {
      id = ids[p];
      if ((unsigned)id >= (unsigned)E) id = -1;  // out of range: dropped
    }
    int rank = 0, cnt = 0;
    for (int e = 0; e < E; ++e) {
      const unsigned long long mask = __ballot(id == e);
      if (id == e) rank = __popcll(mask & lt);
      if (lane == e) cnt = __popcll(mask);
    }
    if (lane < E) wcnt[wave][lane] = cnt;
    __syncthreads();
    if (id >= 0) {
      int off = base[id] + rank;
      for (int w = 0; w < wave; ++w) off += wcnt[w][id];
      if (off < P) {  // always true for a consistent histogram
        order[off] = (int)p;
        pos[p] = off;
      }
    } else if (p < P) {
      pos[p] = -1;
    }
    __syncthreads();
    if ((int)threadIdx.x < E) {
      int add = 0;
#pragma unroll
      for (int w = 0; w < NW; ++w) add += wcnt[w][threadIdx.x];
      base[threadIdx.x] += add;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// permute / combine: rows move as 16-byte chunks, one chunk per lane
// ---------------------------------------------------------------------------
// xs[i] = x[order[i] / k]: a pure copy, so dtype-agnostic
__global__ void moe_permute_fwd_kernel(const float4v* __restrict__ x,
                                       const int* __restrict__ order,
                                       float4v* __restrict__ xs, long P,
                                       long N, int K, int nv) {
  const long total = P * nv;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total;
       c += stride) {
    const long i = c / nv;
    const int col = (int)(c - i * nv);
    const long tok = order[i] / K;
    float4v v = {0.f, 0.f, 0.f, 0.f};
    if (tok >= 0 && tok < N) v = x[tok * nv + col];
    xs[c] = v;
  }
}

// out[t] = sum_j (W ? w[t,j] : 1) * src[pos[t,j]], j ascending, fp32
// accumulate, one rounding (permute backward and combine forward)
template <typename T, bool W>
__global__ void moe_gather_sum_kernel(const T* __restrict__ src,
                                      const T* __restrict__ weights,
                                      const int* __restrict__ pos,
                                      T* __restrict__ out, long N, long P,
                                      int K, int nv) {
  using V = RowVec<T>;
  const long total = N * nv;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long c = blockIdx.x * (long)blockDim.x + threadIdx.x; c < total;
       c += stride) {
    const long t = c / nv;
    const int col = (int)(c - t * nv);
    float acc[V::N];
#pragma unroll
    for (int e = 0; e < V::N; ++e) acc[e] = 0.f;
    for (int j = 0; j < K; ++j) {
      const long r = pos[t * K + j];
      if (r < 0 || r >= P) continue;
      const V v = reinterpret_cast<const V*>(src)[r * nv + col];
      const float w = W ? toF<T>(weights[t * K + j]) : 1.f;
#pragma unroll
      for (int e = 0; e < V::N; ++e) acc[e] += w * toF<T>(v.v[e]);
    }
    V o;
#pragma unroll
    for (int e = 0; e < V::N; ++e) o.v[e] = fromF<T>(acc[e]);
    reinterpret_cast<V*>(out)[c] = o;
  }
}

// dy[pos[t,j]] = w[t,j] * dout[t];  dweights[t,j] = <y[pos[t,j]], dout[t]>
// G = pow2 >= chunks-per-row lanes share a token and reduce the dot product
template <typename T>
__global__ void moe_combine_bwd_kernel(const T* __restrict__ dout,
                                       const T* __restrict__ y,
                                       const T* __restrict__ weights,
                                       const int* __restrict__ pos,
                                       T* __restrict__ dy,
                                       float* __restrict__ dweights, long N,
                                       long P, int K, int nv, int G) {
  using V = RowVec<T>;
  const int sub = threadIdx.x & (G - 1);
  const long t = (blockIdx.x * (long)blockDim.x + threadIdx.x) / G;
  const bool live = t < N;
  for (int j = 0; j < K; ++j) {
    long r = live ? (long)pos[t * K + j] : -1;
    if (r >= P) r = -1;
    float acc = 0.f;
    if (r >= 0) {
      const float w = toF<T>(weights[t * K + j]);
      for (int col = sub; col < nv; col += G) {
        const V d = reinterpret_cast<const V*>(dout)[t * nv + col];
        const V yy = reinterpret_cast<const V*>(y)[r * nv + col];
        V o;
#pragma unroll
        for (int e = 0; e < V::N; ++e) {
          const float df = toF<T>(d.v[e]);
          acc += toF<T>(yy.v[e]) * df;
          o.v[e] = fromF<T>(w * df);
        }
        reinterpret_cast<V*>(dy)[r * nv + col] = o;
      }
    }
    acc = group_sum(acc, G);
    if (live && sub == 0) dweights[t * K + j] = acc;
  }
}

inline dim3 flat_grid(long total) {
  return dim3((unsigned)std::max<long>(
      1, std::min<long>((total + MOE_BLOCK - 1) / MOE_BLOCK, 2048)));
}

inline void check_rows(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() == 2, name,
              ": expected a contiguous 2-D GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16 ||
                  t.scalar_type() == at::kHalf ||
                  t.scalar_type() == at::kFloat,
              name, ": rows must be bf16, fp16 or fp32");
  TORCH_CHECK(t.size(1) % 8 == 0, name, ": hidden must be a multiple of 8");
}

inline void check_index(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kInt,
              name, ": expected a contiguous int32 GPU tensor");
}

inline void check_topk(long N, long E, long K) {
  TORCH_CHECK(E >= 1 && E <= MOE_MAX_E, "moe: n_expert must be in [1, 64]");
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K && K <= E,
              "moe: top_k must be in [1, min(8, n_expert)]");
  TORCH_CHECK(N * K < (1L << 31), "moe: N * top_k must be below 2^31");
}

}  // namespace

std::vector<at::Tensor> moe_route_fwd(at::Tensor logits, int64_t top_k,
                                      at::ScalarType out_dtype) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2);
  const long N = logits.size(0);
  const int E = (int)logits.size(1);
  const int K = (int)top_k;
  check_topk(N, E, K);
  auto weights = at::empty({N, K}, logits.options().dtype(out_dtype));
  auto ids = at::empty({N, K}, logits.options().dtype(at::kInt));
  if (N == 0) return {weights, ids};
  const int G = pow2_group(E);
  const long rpb = MOE_BLOCK / G;
  dim3 grid((unsigned)((N + rpb - 1) / rpb));
  auto stream = at::hip::getCurrentHIPStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, logits.scalar_type(), "moe_route_fwd", [&] {
        using TL = scalar_t;
        AT_DISPATCH_FLOATING_TYPES_AND2(
            at::kBFloat16, at::kHalf, out_dtype, "moe_route_fwd_out", [&] {
              using TW = scalar_t;
              hipLaunchKernelGGL(
                  (moe_route_fwd_kernel<TL, TW>), grid, dim3(MOE_BLOCK), 0,
                  stream.stream(),
                  reinterpret_cast<const TL*>(logits.data_ptr()),
                  reinterpret_cast<TW*>(weights.data_ptr()),
                  ids.data_ptr<int>(), N, E, K, G);
            });
      });
  return {weights, ids};
}

at::Tensor moe_route_bwd(at::Tensor logits, at::Tensor ids,
                         at::Tensor dweights) {
  TORCH_CHECK(logits.is_cuda() && logits.is_contiguous() && logits.dim() == 2);
  check_index(ids, "ids");
  TORCH_CHECK(dweights.is_cuda() && dweights.is_contiguous() &&
                  dweights.scalar_type() == at::kFloat,
              "dweights: expected a contiguous fp32 GPU tensor");
  const long N = logits.size(0);
  const int E = (int)logits.size(1);
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == N);
  const int K = (int)ids.size(1);
  check_topk(N, E, K);
  TORCH_CHECK(dweights.sizes() == ids.sizes());
  auto dlogits = at::empty_like(logits);
  if (N == 0) return dlogits;
  const int G = pow2_group(E);
  const long rpb = MOE_BLOCK / G;
  dim3 grid((unsigned)((N + rpb - 1) / rpb));
  auto stream = at::hip::getCurrentHIPStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, logits.scalar_type(), "moe_route_bwd", [&] {
        hipLaunchKernelGGL(
            moe_route_bwd_kernel<scalar_t>, grid, dim3(MOE_BLOCK), 0,
            stream.stream(),
            reinterpret_cast<const scalar_t*>(logits.data_ptr()),
            ids.data_ptr<int>(), dweights.data_ptr<float>(),
            reinterpret_cast<scalar_t*>(dlogits.data_ptr()), N, E, K, G);
      });
  return dlogits;
}

std::vector<at::Tensor> moe_sort(at::Tensor ids, int64_t n_expert) {
  check_index(ids, "ids");
  TORCH_CHECK(ids.dim() == 2);
  const long N = ids.size(0);
  const int K = (int)ids.size(1);
  const int E = (int)n_expert;
  check_topk(N, E, K);
  const long P = N * K;
  auto order = at::empty({P}, ids.options());
  auto pos = at::empty({N, K}, ids.options());
  if (P == 0) return {order, pos, at::zeros({E}, ids.options())};
  auto counts = at::empty({E}, ids.options());
  const int nb = (int)((P + SORT_CHUNK - 1) / SORT_CHUNK);
  auto blockhist = at::empty({nb, E}, ids.options());
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_hist_kernel, dim3(nb), dim3(MOE_BLOCK), 0,
                     stream.stream(), ids.data_ptr<int>(),
                     blockhist.data_ptr<int>(), P, E);
  hipLaunchKernelGGL(moe_scan_kernel, dim3(1), dim3(MOE_BLOCK), 0,
                     stream.stream(), blockhist.data_ptr<int>(),
                     counts.data_ptr<int>(), nb, E);
  hipLaunchKernelGGL(moe_rank_kernel, dim3(nb), dim3(MOE_BLOCK), 0,
                     stream.stream(), ids.data_ptr<int>(),
                     blockhist.data_ptr<int>(), order.data_ptr<int>(),
                     pos.data_ptr<int>(), P, E);
  return {order, pos, counts};
}

at::Tensor moe_permute_fwd(at::Tensor x, at::Tensor order, int64_t top_k) {
  check_rows(x, "x");
  check_index(order, "order");
  const long N = x.size(0);
  const long H = x.size(1);
  const int K = (int)top_k;
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K);
  TORCH_CHECK(N * K < (1L << 31) && order.dim() == 1 &&
              order.size(0) == N * K);
  const long P = N * K;
  auto xs = at::empty({P, H}, x.options());
  if (P == 0) return xs;
  const int nv = (int)(H * x.element_size() / 16);
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(moe_permute_fwd_kernel, flat_grid(P * nv),
                     dim3(MOE_BLOCK), 0, stream.stream(),
                     reinterpret_cast<const float4v*>(x.data_ptr()),
                     order.data_ptr<int>(),
                     reinterpret_cast<float4v*>(xs.data_ptr()), P, N, K, nv);
  return xs;
}

at::Tensor moe_permute_bwd(at::Tensor dxs, at::Tensor pos) {
  check_rows(dxs, "dxs");
  check_index(pos, "pos");
  TORCH_CHECK(pos.dim() == 2);
  const long N = pos.size(0);
  const int K = (int)pos.size(1);
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K);
  const long P = N * K;
  TORCH_CHECK(P < (1L << 31) && dxs.size(0) == P);
  const long H = dxs.size(1);
  auto dx = at::empty({N, H}, dxs.options());
  if (N == 0) return dx;
  const int nv = (int)(H * dxs.element_size() / 16);
  auto stream = at::hip::getCurrentHIPStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, dxs.scalar_type(), "moe_permute_bwd", [&] {
        hipLaunchKernelGGL(
            (moe_gather_sum_kernel<scalar_t, false>), flat_grid(N * nv),
            dim3(MOE_BLOCK), 0, stream.stream(),
            reinterpret_cast<const scalar_t*>(dxs.data_ptr()),
            static_cast<const scalar_t*>(nullptr), pos.data_ptr<int>(),
            reinterpret_cast<scalar_t*>(dx.data_ptr()), N, P, K, nv);
      });
  return dx;
}

at::Tensor moe_combine_fwd(at::Tensor y, at::Tensor weights, at::Tensor pos) {
  check_rows(y, "y");
  check_index(pos, "pos");
  TORCH_CHECK(pos.dim() == 2);
  const long N = pos.size(0);
  const int K = (int)pos.size(1);
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K);
  const long P = N * K;
  TORCH_CHECK(P < (1L << 31) && y.size(0) == P);
  TORCH_CHECK(weights.is_cuda() && weights.is_contiguous() &&
                  weights.scalar_type() == y.scalar_type() &&
                  weights.sizes() == pos.sizes(),
              "weights: expected [N, k] in the dtype of y");
  const long H = y.size(1);
  auto out = at::empty({N, H}, y.options());
  if (N == 0) return out;
  const int nv = (int)(H * y.element_size() / 16);
  auto stream = at::hip::getCurrentHIPStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, y.scalar_type(), "moe_combine_fwd", [&] {
        hipLaunchKernelGGL(
            (moe_gather_sum_kernel<scalar_t, true>), flat_grid(N * nv),
            dim3(MOE_BLOCK), 0, stream.stream(),
            reinterpret_cast<const scalar_t*>(y.data_ptr()),
            reinterpret_cast<const scalar_t*>(weights.data_ptr()),
            pos.data_ptr<int>(), reinterpret_cast<scalar_t*>(out.data_ptr()),
            N, P, K, nv);
      });
  return out;
}

std::vector<at::Tensor> moe_combine_bwd(at::Tensor dout, at::Tensor y,
                                        at::Tensor weights, at::Tensor pos) {
  check_rows(dout, "dout");
  check_rows(y, "y");
  check_index(pos, "pos");
  TORCH_CHECK(pos.dim() == 2);
  const long N = pos.size(0);
  const int K = (int)pos.size(1);
  TORCH_CHECK(K >= 1 && K <= MOE_MAX_K);
  const long P = N * K;
  const long H = y.size(1);
  TORCH_CHECK(P < (1L << 31) && y.size(0) == P && dout.size(0) == N &&
              dout.size(1) == H && dout.scalar_type() == y.scalar_type());
  TORCH_CHECK(weights.is_cuda() && weights.is_contiguous() &&
                  weights.scalar_type() == y.scalar_type() &&
                  weights.sizes() == pos.sizes(),
              "weights: expected [N, k] in the dtype of y");
  auto dy = at::empty_like(y);
  auto dweights = at::empty({N, K}, y.options().dtype(at::kFloat));
  if (N == 0) return {dy, dweights};
  const int nv = (int)(H * y.element_size() / 16);
  const int G = pow2_group(nv);
  const long rpb = MOE_BLOCK / G;
  dim3 grid((unsigned)((N + rpb - 1) / rpb));
  auto stream = at::hip::getCurrentHIPStream();
  AT_DISPATCH_FLOATING_TYPES_AND2(
      at::kBFloat16, at::kHalf, y.scalar_type(), "moe_combine_bwd", [&] {
        hipLaunchKernelGGL(
            moe_combine_bwd_kernel<scalar_t>, grid, dim3(MOE_BLOCK), 0,
            stream.stream(),
            reinterpret_cast<const scalar_t*>(dout.data_ptr()),
            reinterpret_cast<const scalar_t*>(y.data_ptr()),
            reinterpret_cast<const scalar_t*>(weights.data_ptr()),
            pos.data_ptr<int>(), reinterpret_cast<scalar_t*>(dy.data_ptr()),
            dweights.data_ptr<float>(), N, P, K, nv, G);
      });
  return {dy, dweights};
}

}  // namespace samd
