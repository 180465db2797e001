// Label propagation over the embedding's kNN graph (include/cmlpl.h, "THE DEFINITION OF A PROPAGATED LABELLING"; Zhou et
// al., "Learning with Local and Global Consistency", NIPS 2003).  The graph is W = A + A^T over cmlpl_knn's lists: a node's
// edge list is its forward entries (rank ascending) and then its reverse edges by ascending source, an inverted index.
//
//   lp_count_kernel  : one thread per list entry; an integer atomic per edge counts the in-degrees.
//   lp_scan_kernel   : ONE workgroup; the exclusive scan of the in-degrees is rev_ptr; it clears the counters again.
//   lp_fill_kernel   : one thread per entry; the same integer atomic hands out a slot of the target's segment, the edge id
//                      i k + r goes there.  The order INSIDE a segment is the run's; the next launch removes it.
//   lp_sort_kernel   : one workgroup per node.  Edge ids are unique, so a segment is sorted by counting: up to LP_SORT_LDS
//                      ids sit in LDS and every id counts the smaller ones; a longer segment (a hub: in-degree has no bound)
//                      is not sorted at all but RE-FOUND in order, by a compaction scan over the n k entries of the lists.
//                      Either way source, weight and edge id land in ascending (source, rank) order.  Then thread 0 adds the
//                      node's weights in list order -- one fp32 chain of any length -- and stores cinv.
//   lp_coef_kernel   : one thread per slot: the forward coefficient (c_i a) c_j; the reverse slot's owner by bisection of
//                      rev_ptr, its coefficient (c_i a) c_src in place of the weight; slots past the last edge are cleared,
//                      so every byte of the workspace is a function of the lists.
//   lp_step_kernel<G>: an iteration.  A group of G lanes per node (rowgroup.hpp's G of K), one class per lane; indices and
//                      coefficients are read G at a time, one per lane, and handed round by shuffles; a neighbour's F row is
//                      one contiguous 4 K-byte segment.  One fmaf per edge and class, in list order.
//   lp_finish_kernel : p = F / z, the first maximum, confidence, entropy.
// Integer atomics only; no float atomics, no scratch, no LDS beyond the sort's; nothing synchronises or allocates.
#include <float.h>
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int LP_KMAX = 32, LP_CMAX = 64, LP_GAMMA_MAX = 8, LP_ITERS_MAX = 10000;
constexpr int LP_SORT_LDS = 2048;      // ids of a segment sorted in LDS; longer segments take the compaction scan

// a = s^gamma by repeated multiplication for 0 < s <= FLT_MAX, else 0 (NaN, -inf, negative: the comparison is false)
__device__ __forceinline__ float lp_weight(float s, int gamma) {
  if (!(s > 0.f && s <= FLT_MAX)) return 0.f;
  float a = s;
  for (int g = 1; g < gamma; ++g) a = __fmul_rn(a, s);
  return a;
}

__device__ __forceinline__ bool lp_edge(int j, int i) { return j >= 0 && j != i; }

__global__ __launch_bounds__(256) void lp_count_kernel(const int* __restrict__ idx, int N, int k, int* __restrict__ cnt) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const int j = idx[e];
  if (lp_edge(j, e / k)) atomicAdd(&cnt[j], 1);
}

// exclusive scan of cnt [n] into ptr [n + 1]; cnt is left at zero.  One workgroup of 1024 threads walks the array.
__global__ __launch_bounds__(1024) void lp_scan_kernel(int* __restrict__ cnt, int n, int* __restrict__ ptr) {
  __shared__ int wsum[16];
  __shared__ int carry;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int v = i < n ? cnt[i] : 0;
    int s = v;                                                   // inclusive scan of the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(s, d, 64);
      if (lane >= d) s += t;
    }
    if (lane == 63) wsum[w] = s;
    __syncthreads();
    int off = carry;
    for (int q = 0; q < w; ++q) off += wsum[q];
    if (i < n) { ptr[i] = off + s - v; cnt[i] = 0; }
    __syncthreads();
    if (tid == 1023) carry = off + s;
    __syncthreads();
  }
  if (tid == 0) ptr[n] = carry;
}

__global__ __launch_bounds__(256) void lp_fill_kernel(const int* __restrict__ idx, int N, int k, const int* __restrict__ ptr,
                                                      int* __restrict__ cnt, int* __restrict__ edge) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= N) return;
  const int j = idx[e];
  if (lp_edge(j, e / k)) edge[ptr[j] + atomicAdd(&cnt[j], 1)] = e;
}

struct LpSort {
  const int* idx; const float* sim; int n, k, N, gamma;
  const int* ptr; int* edge; int* src; float* w; float* cinv;
};

__global__ __launch_bounds__(256) void lp_sort_kernel(LpSort a) {
  __shared__ int ids[LP_SORT_LDS];
  __shared__ int wcnt[4][4];
  const int t = blockIdx.x, tid = threadIdx.x;
  const int p0 = a.ptr[t], L = a.ptr[t + 1] - p0;
  if (L <= LP_SORT_LDS) {
    for (int q = tid; q < L; q += 256) ids[q] = a.edge[p0 + q];
    __syncthreads();
    for (int q = tid; q < L; q += 256) {
      const int e = ids[q];
      int rank = 0;
      for (int u = 0; u < L; ++u) rank += ids[u] < e;            // an LDS broadcast per step
      a.edge[p0 + rank] = e;
      a.src[p0 + rank] = e / a.k;
      a.w[p0 + rank] = lp_weight(a.sim[e], a.gamma);
    }
  } else {
    // the hub: walk ALL entries in ascending edge id, 1024 at a time (four per thread, q-major), and compact the ones
    // that point here: positions by ballot + popcount, per (q, wavefront) counts through LDS
    const int lane = tid & 63, wv = tid >> 6;
    int base = 0;
    for (int c0 = 0; c0 < a.N; c0 += 1024) {
      int e[4], pos[4];
      bool hit[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        e[q] = c0 + q * 256 + tid;
        const int j = e[q] < a.N ? a.idx[e[q]] : -1;
        hit[q] = j == t && e[q] / a.k != t;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const unsigned long long m = __ballot(hit[q]);
        pos[q] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[q][wv] = __popcll(m);
      }
      __syncthreads();
      int run = 0, off[4];                                       // counts of the (q, wavefront) pairs in front of this one
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (u == wv) off[q] = run;
          run += wcnt[q][u];
        }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (hit[q]) {
          const int p = p0 + base + off[q] + pos[q];
          a.edge[p] = e[q];
          a.src[p] = e[q] / a.k;
          a.w[p] = lp_weight(a.sim[e[q]], a.gamma);
        }
      base += run;                                               // (the same sum in every thread)
      __syncthreads();
    }
  }
  __threadfence_block();
  __syncthreads();
  if (tid == 0) {                                                // the degree: ONE fp32 chain in list order
    float d = 0.f;
    for (int r = 0; r < a.k; ++r) {
      const int e = t * a.k + r;
      if (lp_edge(a.idx[e], t)) d = __fadd_rn(d, lp_weight(a.sim[e], a.gamma));
    }
    const float* w = a.w + p0;
    for (int q = 0; q < L; ++q) d = __fadd_rn(d, w[q]);
    a.cinv[t] = d > 0.f ? 1.f / sqrtf(d) : 0.f;
  }
}

struct LpCoef {
  const int* idx; const float* sim; int n, k, N, gamma;
  const float* cinv; float* fwd; int* dst; const int* ptr; int* src; float* rev; int* edge;
};

__global__ __launch_bounds__(256) void lp_coef_kernel(LpCoef a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.N) return;
  const int i = e / a.k, j = a.idx[e];
  const bool fe = lp_edge(j, i);
  a.fwd[e] = fe ? __fmul_rn(__fmul_rn(a.cinv[i], lp_weight(a.sim[e], a.gamma)), a.cinv[j]) : 0.f;
  a.dst[e] = fe ? j : -1;
  if (e >= a.ptr[a.n]) {                                         // behind the last reverse edge
    a.src[e] = -1; a.rev[e] = 0.f; a.edge[e] = -1;
    return;
  }
  int lo = 0, hi = a.n;                                          // the owner: the last node whose segment starts at or before e
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (a.ptr[mid] <= e) lo = mid; else hi = mid;
  }
  a.rev[e] = __fmul_rn(__fmul_rn(a.cinv[lo], a.rev[e]), a.cinv[a.src[e]]);
}

struct LpStep {
  const int* idx; const float* fwd; const int* ptr; const int* src; const float* rev;
  const float* Y; const float* in; float* out; unsigned* residual;
  int n, k, K; float alpha, beta;
};

template <int G>
__global__ __launch_bounds__(256) void lp_step_kernel(LpStep a) {
  const int tid = threadIdx.x, c = tid & (G - 1);
  const long long node = (long long)blockIdx.x * (256 / G) + tid / G;
  const bool live = node < a.n;
  const int i = live ? (int)node : a.n - 1;                      // a dead group walks no list and stores nothing
  const int kk = live ? a.k : 0;
  const int cc = c < a.K ? c : a.K - 1;
  float acc = 0.f;
  const int* idx = a.idx + (size_t)i * a.k;
  const float* fwd = a.fwd + (size_t)i * a.k;
  for (int b = 0; b < kk; b += G) {
    const int r = b + c;
    const int jm = r < kk ? idx[r] : -1;
    const float cm = r < kk ? fwd[r] : 0.f;
    const int m = kk - b < G ? kk - b : G;
    for (int u = 0; u < m; ++u) {
      const int j = G == 1 ? jm : __shfl(jm, u, G);
      const float cf = G == 1 ? cm : __shfl(cm, u, G);
      if (j >= 0) acc = fmaf(cf, a.in[(size_t)j * a.K + cc], acc);      // (-1: a pad or a self entry)
    }
  }
  const int p0 = a.ptr[i], p1 = live ? a.ptr[i + 1] : p0;
  for (int b = p0; b < p1; b += G) {
    const int p = b + c;
    const int jm = p < p1 ? a.src[p] : 0;
    const float cm = p < p1 ? a.rev[p] : 0.f;
    const int m = p1 - b < G ? p1 - b : G;
    if (m == G) {
#pragma unroll 8
      for (int u = 0; u < G; ++u) {
        const int j = G == 1 ? jm : __shfl(jm, u, G);
        const float cf = G == 1 ? cm : __shfl(cm, u, G);
        acc = fmaf(cf, a.in[(size_t)j * a.K + cc], acc);
      }
    } else {
      for (int u = 0; u < m; ++u) {
        const int j = G == 1 ? jm : __shfl(jm, u, G);
        const float cf = G == 1 ? cm : __shfl(cm, u, G);
        acc = fmaf(cf, a.in[(size_t)j * a.K + cc], acc);
      }
    }
  }
  const size_t at = (size_t)i * a.K + cc;
  const float v = fmaf(a.alpha, acc, __fmul_rn(a.beta, a.Y[at]));
  if (live && c < a.K) a.out[at] = v;
  if (a.residual) {                                              // the last iteration: max |new - old| on the bit patterns
    unsigned bits = live && c < a.K ? __float_as_uint(fabsf(__fsub_rn(v, a.in[at]))) : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const unsigned o = (unsigned)__shfl_xor((int)bits, d, 64);
      bits = o > bits ? o : bits;
    }
    if ((tid & 63) == 0 && bits) atomicMax(a.residual, bits);
  }
}

struct LpFinish {
  const float* F; int n, K;
  float* probs; long long* labels; float* conf; float* entropy;
};

template <int G>
__global__ __launch_bounds__(256) void lp_finish_kernel(LpFinish a) {
  const int tid = threadIdx.x, c = tid & (G - 1);
  const long long node = (long long)blockIdx.x * (256 / G) + tid / G;
  const bool live = node < a.n;
  const int i = live ? (int)node : a.n - 1;
  const float* row = a.F + (size_t)i * a.K;
  const float f = c < a.K ? row[c] : 0.f;
  float z = 0.f;
  for (int u = 0; u < a.K; ++u) z = __fadd_rn(z, G == 1 ? f : __shfl(f, u, G));      // c ascending
  const bool ok = z > 0.f;
  const float nan = __uint_as_float(0x7fc00000u);
  const float p = ok ? f / z : nan;
  // the first maximum: (p, class), a larger p or an equal p of a lower class wins; a NaN never wins
  float bp = c < a.K && ok ? p : -1.f;
  int bc = c;
#pragma unroll
  for (int d = G >> 1; d >= 1; d >>= 1) {
    const float op = __shfl_xor(bp, d, G);
    const int oc = __shfl_xor(bc, d, G);
    if (op > bp || (op == bp && oc < bc)) { bp = op; bc = oc; }
  }
  const float term = c < a.K && ok && p > 0.f ? __fmul_rn(p, logf(p)) : 0.f;
  float h = 0.f;
  for (int u = 0; u < a.K; ++u) h = __fadd_rn(h, G == 1 ? term : __shfl(term, u, G));
  if (!live) return;
  if (a.probs && c < a.K) a.probs[(size_t)i * a.K + c] = p;
  if (c == 0) {
    if (a.labels) a.labels[i] = ok ? bc : -1;
    if (a.conf) a.conf[i] = ok ? bp : nan;
    if (a.entropy) a.entropy[i] = ok ? -h : nan;
  }
}

struct LpLayout { size_t cinv, fwd, ptr, src, rev, dst, edge, cnt, words; };   // in 4-byte words

LpLayout lp_layout(int n, int k) {
  const size_t N = (size_t)n * k;
  LpLayout l;
  l.cinv = 0; l.fwd = l.cinv + n; l.ptr = l.fwd + N; l.src = l.ptr + n + 1; l.rev = l.src + N; l.dst = l.rev + N; l.edge = l.dst + N;
  l.cnt = l.edge + N; l.words = l.cnt + n;
  return l;
}

bool lp_shape_ok(int n, int k) { return n >= 1 && k >= 1 && k <= LP_KMAX && (long long)n * k < (1ll << 31); }

}  // namespace
}  // namespace cmlpl

extern "C" size_t cmlpl_lp_graph_bytes(int n, int k) {
  using namespace cmlpl;
  return lp_shape_ok(n, k) ? lp_layout(n, k).words * 4 : 0;
}

extern "C" int cmlpl_lp_graph(const int32_t* d_nbr_idx, const float* d_nbr_sim, int n, int k, int gamma, void* d_graph,
                              size_t bytes, void* stream) {
  using namespace cmlpl;
  if (!d_nbr_idx || !d_nbr_sim || !d_graph || !lp_shape_ok(n, k) || gamma < 1 || gamma > LP_GAMMA_MAX) return CMLPL_E_ARG;
  if (!aligned_to(3, d_nbr_idx, d_nbr_sim, d_graph)) return CMLPL_E_ARG;
  if (cmlpl_lp_graph_bytes(n, k) > bytes) return CMLPL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const LpLayout l = lp_layout(n, k);
  const int N = n * k;
  float* wf = (float*)d_graph;
  int* wi = (int*)d_graph;
  int* cnt = wi + l.cnt;
  int* ptr = wi + l.ptr;
  int* edge = wi + l.edge;
  hipError_t e = hipMemsetAsync(cnt, 0, (size_t)n * 4, st);
  if (e != hipSuccess) return (int)e;
  const unsigned eb = (unsigned)((N + 255) / 256);
  hipLaunchKernelGGL(lp_count_kernel, dim3(eb), dim3(256), 0, st, d_nbr_idx, N, k, cnt);
  hipLaunchKernelGGL(lp_scan_kernel, dim3(1), dim3(1024), 0, st, cnt, n, ptr);
  hipLaunchKernelGGL(lp_fill_kernel, dim3(eb), dim3(256), 0, st, d_nbr_idx, N, k, ptr, cnt, edge);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  LpSort s = {};
  s.idx = d_nbr_idx; s.sim = d_nbr_sim; s.n = n; s.k = k; s.N = N; s.gamma = gamma;
  s.ptr = ptr; s.edge = edge; s.src = wi + l.src; s.w = wf + l.rev; s.cinv = wf + l.cinv;
  hipLaunchKernelGGL(lp_sort_kernel, dim3(n), dim3(256), 0, st, s);
  LpCoef c = {};
  c.idx = d_nbr_idx; c.sim = d_nbr_sim; c.n = n; c.k = k; c.N = N; c.gamma = gamma;
  c.cinv = wf + l.cinv; c.fwd = wf + l.fwd; c.ptr = ptr; c.src = wi + l.src; c.rev = wf + l.rev; c.edge = edge; c.dst = wi + l.dst;
  hipLaunchKernelGGL(lp_coef_kernel, dim3(eb), dim3(256), 0, st, c);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int cmlpl_lp_propagate(const void* d_graph, int n, int k, const float* d_Y, int K,
                                  float alpha, int iters, const float* d_F0, float* d_F, float* d_tmp, float* d_probs,
                                  int64_t* d_labels, float* d_conf, float* d_entropy, float* d_residual, void* stream) {
  using namespace cmlpl;
  if (!d_graph || !d_Y || !d_F || !d_tmp || !lp_shape_ok(n, k) || K < 1 || K > LP_CMAX) return CMLPL_E_ARG;
  if (!(alpha >= 0.f && alpha < 1.f) || iters < 1 || iters > LP_ITERS_MAX) return CMLPL_E_ARG;
  if ((long long)n * K >= (1ll << 31)) return CMLPL_E_ARG;
  const float* start = d_F0 ? d_F0 : d_Y;
  if (d_F == d_tmp || start == d_F || start == d_tmp || d_Y == d_F || d_Y == d_tmp) return CMLPL_E_ARG;
  if (!aligned_to(3, d_graph, d_Y, d_F0, d_F, d_tmp, d_probs, d_conf, d_entropy, d_residual)) return CMLPL_E_ARG;
  if (!aligned_to(7, d_labels)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const LpLayout l = lp_layout(n, k);
  const float* wf = (const float*)d_graph;
  const int* wi = (const int*)d_graph;
  hipError_t e;
  if (d_residual && (e = hipMemsetAsync(d_residual, 0, 4, st)) != hipSuccess) return (int)e;
  LpStep s = {};
  s.idx = wi + l.dst; s.fwd = wf + l.fwd; s.ptr = wi + l.ptr; s.src = wi + l.src; s.rev = wf + l.rev;
  s.Y = d_Y; s.n = n; s.k = k; s.K = K; s.alpha = alpha; s.beta = (float)(1.0 - (double)alpha);
  const float* in = start;
  for (int t = 1; t <= iters; ++t) {
    float* out = (iters - t) % 2 == 0 ? d_F : d_tmp;             // the last one writes d_F
    s.in = in; s.out = out; s.residual = t == iters ? reinterpret_cast<unsigned*>(d_residual) : nullptr;
    with_group(K, [&](auto g) { hipLaunchKernelGGL(lp_step_kernel<g>, dim3(group_grid(n, 256, g)), dim3(256), 0, st, s); });
    in = out;
  }
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (d_probs || d_labels || d_conf || d_entropy) {
    LpFinish f = {};
    f.F = d_F; f.n = n; f.K = K; f.probs = d_probs; f.labels = reinterpret_cast<long long*>(d_labels); f.conf = d_conf;
    f.entropy = d_entropy;
    with_group(K, [&](auto g) { hipLaunchKernelGGL(lp_finish_kernel<g>, dim3(group_grid(n, 256, g)), dim3(256), 0, st, f); });
    e = hipGetLastError();
  }
  return e == hipSuccess ? 0 : (int)e;
}
