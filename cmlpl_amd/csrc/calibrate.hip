// Calibration of the prediction products (include/cmlpl.h, "THE DEFINITION OF THE RELIABILITY COUNTERS" and the two calls
// behind it): does a written confidence mean what it says, and the smallest standard remedy, one scalar temperature.
//   cmlpl_reliability   READS a probability map and ADDS to a block of int64 counters.  rowgroup.hpp's lane scheme, a group
//                       of G lanes per item: the row maximum, its first index (the first-maximum rule) and the Brier sum
//                       are its butterflies.  The first lane of a group
//                       scores its item: one LDS atomic per scored row into the workgroup's tile of the bins (int32 count /
//                       hits, int64 conf_sum: 16 KB at 1024 bins), the head counts by ballot and popcount per wave, the
//                       fixed-point sums in its registers.  At the end one 64-bit global integer atomic per NON-ZERO word
//                       (confusion_kernel's scheme).  Integer sums only: exact, order-free, the same bytes on every run.
//   cmlpl_temper_probs  q = softmax(beta log p) per row in the same lane scheme; plain loads and stores, no LDS, no atomics.
//   cmlpl_nll_temps     lanes = candidate values of beta, one wavefront per row at a time: lane c < K takes logf(p_c) once
//                       for the wave, every lane reads class c's value from lane c (c uniform) and walks its own chain, its
//                       int64 sum stays in registers over the wave's rows; one LDS fold per workgroup, one 64-bit global
//                       integer atomic per non-zero word.
// Products that the header keeps apart from the sums behind them are formed by __fmul_rn / __fsub_rn: nothing is contracted
// into a fused multiply-add.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "common.hpp"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int CAL_THREADS = 256;
constexpr int CAL_KMAX = 64;
constexpr int REL_BINS_MAX = 1024;
constexpr int REL_WG_MAX = 1024;      // past REL_WG_MAX workgroups the grid strides over the items (fewer tiles to flush)
constexpr int TMP_WG_MAX = 4096;
constexpr int NLL_SMAX = 64;
constexpr int NLL_WG_MAX = 2048;
constexpr float FIX24 = 16777216.f;   // 2^24
constexpr float FIX20 = 1048576.f;    // 2^20

typedef unsigned long long u64;

// group_argmax with its -1 clamped to 0 (lane 0 of a group always owns a class, so the clamp never acts; the compiler
// cannot see that, and the label indexes a shuffle)
template <int G> __device__ __forceinline__ int gargmax(float v, float mx, bool kv, int shift) {
  const int l = group_argmax<G>(v, mx, kv, shift);
  return l < 0 ? 0 : l;
}

// ------------------------------------------------------------------ the reliability counters
struct RelArgs {
  const float* probs; const long long* row; const long long* truth;
  int n, K, B;
  u64* counts;
};

template <int G> __global__ __launch_bounds__(CAL_THREADS) void reliability_kernel(RelArgs a) {
  constexpr int PPW = CAL_THREADS / G;                  // items per workgroup and trip
  __shared__ int cnt[REL_BINS_MAX];
  __shared__ int hits[REL_BINS_MAX];
  __shared__ u64 csum[REL_BINS_MAX];
  __shared__ u64 head[CMLPL_REL_HEAD];
  const int tid = threadIdx.x;
  const int c = tid & (G - 1);                          // the class this lane owns
  const int shift = (tid & 63) & ~(G - 1);              // the first lane of this group within its wave
  const int K = a.K, n = a.n, B = a.B;
  const bool kv = c < K;
  const float NEG_INF = -INFINITY;
  for (int b = tid; b < B; b += CAL_THREADS) { cnt[b] = 0; hits[b] = 0; csum[b] = 0ull; }
  if (tid < CMLPL_REL_HEAD) head[tid] = 0ull;
  __syncthreads();
  unsigned n_items = 0, n_known = 0, n_ign = 0, n_nan = 0, n_hit = 0, n_inf = 0;   // (the same in every lane of a wave)
  long long s_conf = 0, s_nll = 0, s_brier = 0;                                     // (this lane's items)
  // (the trip count is the same for every lane of a workgroup: the shuffles and ballots meet whole waves)
  // this lane's truth and class value of the trip at `base` (an item past the last: unknown truth, -inf)
  auto fetch = [&](long long base, long long& t, float& p) {
    const long long i = base + tid / G;
    t = -1; p = NEG_INF;
    if (i < n) {
      t = a.truth[i];
      if (kv) p = a.probs[(a.row ? a.row[i] : i) * K + c];
    }
  };
  const long long stride = (long long)gridDim.x * PPW;
  long long t_next; float p_next;
  fetch((long long)blockIdx.x * PPW, t_next, p_next);
  for (long long base = (long long)blockIdx.x * PPW; base < n; base += stride) {
    const bool in = base + tid / G < n;
    const long long t = t_next;
    const float p = p_next;
    // the next trip's loads are in flight while this one is scored: a trip is otherwise one memory latency after another
    if (base + stride < n) fetch(base + stride, t_next, p_next);
    const bool known = in && t >= 0 && t < K;
    const int tt = known ? (int)t : 0;
    const int label = gargmax<G>(p, group_max<G>(p), kv, shift);
    const float conf = __shfl(p, shift + label, 64);
    const float pt = __shfl(p, shift + tt, 64);
    const float d = c == tt ? p - 1.f : p;
    const float brier = group_sum<G>(kv ? __fmul_rn(d, d) : 0.f);
    const bool lead = in && c == 0;
    const bool isnan = known && conf != conf;
    const bool scored = known && !isnan;
    const bool hit = scored && label == tt;
    const bool inf = scored && !(pt > 0.f);
    n_items += (unsigned)__popcll(__ballot(lead));
    n_known += (unsigned)__popcll(__ballot(lead && known));
    n_ign += (unsigned)__popcll(__ballot(lead && !known));
    n_nan += (unsigned)__popcll(__ballot(lead && isnan));
    n_hit += (unsigned)__popcll(__ballot(lead && hit));
    n_inf += (unsigned)__popcll(__ballot(lead && inf));
    if (lead && scored) {
      const float x = conf * (float)B;
      const int b = x >= (float)B ? B - 1 : (x > 0.f ? (int)x : 0);       // (inside 0 .. B - 1 whatever conf is)
      const long long fc = llrintf(conf * FIX24);
      atomicAdd(&cnt[b], 1);
      if (hit) atomicAdd(&hits[b], 1);
      atomicAdd(&csum[b], (u64)fc);
      s_conf += fc;
      if (!inf) s_nll += llrintf((0.f - logf(pt)) * FIX24);
      s_brier += llrintf(brier * FIX24);
    }
  }
  if ((tid & 63) == 0) {
    if (n_items) atomicAdd(&head[0], (u64)n_items);
    if (n_known) atomicAdd(&head[1], (u64)n_known);
    if (n_ign) atomicAdd(&head[2], (u64)n_ign);
    if (n_nan) atomicAdd(&head[3], (u64)n_nan);
    if (n_hit) atomicAdd(&head[4], (u64)n_hit);
    if (n_inf) atomicAdd(&head[7], (u64)n_inf);
  }
  if (s_conf != 0) atomicAdd(&head[5], (u64)s_conf);
  if (s_nll != 0) atomicAdd(&head[6], (u64)s_nll);
  if (s_brier != 0) atomicAdd(&head[8], (u64)s_brier);
  __syncthreads();
  if (tid < CMLPL_REL_HEAD) {
    const u64 v = head[tid];
    if (v != 0ull) atomicAdd(&a.counts[tid], v);
  }
  u64* bins = a.counts + CMLPL_REL_HEAD;
  for (int b = tid; b < B; b += CAL_THREADS) {          // (b < B: inside count[B], hits[B], conf_sum[B])
    const int v = cnt[b], h = hits[b];
    const u64 s = csum[b];
    if (v != 0) atomicAdd(&bins[b], (u64)v);
    if (h != 0) atomicAdd(&bins[B + b], (u64)h);
    if (s != 0ull) atomicAdd(&bins[2 * B + b], s);
  }
}

// ------------------------------------------------------------------ tempered probabilities
struct TmpArgs {
  const float* probs; int n, K; float beta;
  float* out; long long* labels; float* conf; float* entropy;
};

template <int G> __global__ __launch_bounds__(CAL_THREADS) void temper_kernel(TmpArgs a) {
  constexpr int PPW = CAL_THREADS / G;
  const int tid = threadIdx.x;
  const int c = tid & (G - 1);
  const int shift = (tid & 63) & ~(G - 1);
  const int K = a.K, n = a.n;
  const bool kv = c < K;
  const float beta = a.beta;
  for (long long base = (long long)blockIdx.x * PPW; base < n; base += (long long)gridDim.x * PPW) {
    const long long i = base + tid / G;
    const bool live = kv && i < n;                      // (a group past the last row runs on padding and stores nothing)
    const float p = live ? a.probs[i * K + c] : -INFINITY;      // the whole row is read in front of every store of the group
    const float pmx = group_max<G>(p);
    const int label = gargmax<G>(p, pmx, kv, shift);
    const bool bad = group_any<G>(live && (p != p || p < 0.f || p == INFINITY), shift) || !(pmx > 0.f);
    const float l = live ? logf(p) : -INFINITY;         // (padding: -inf into the maximum, 0 into the sum)
    const float m = group_max<G>(l);
    const float e = live ? expf(__fmul_rn(beta, __fsub_rn(l, m))) : 0.f;
    const float s = group_sum<G>(e);
    const float q = bad ? NAN : e / s;
    const float qlab = __shfl(q, shift + label, 64);
    const float t = (q == 0.f) ? 0.f : __fmul_rn(q, logf(q));   // (a NaN q is not 0: it goes through)
    const float ent = 0.f - group_sum<G>(kv ? t : 0.f);
    if (live) {
      if (a.out != nullptr) a.out[i * K + c] = q;
      if (c == 0) {
        if (a.labels != nullptr) a.labels[i] = label;
        if (a.conf != nullptr) a.conf[i] = qlab;
        if (a.entropy != nullptr) a.entropy[i] = ent;
      }
    }
  }
}

// the launch of kernel_of(G), the kernel for the G of a.K (rowgroup.hpp), over a.n rows on at most wg_max workgroups
template <class Args, class KernelOf> hipError_t launch_rows(const Args& a, int wg_max, hipStream_t st, KernelOf kernel_of) {
  return with_group(a.K, [&](auto g) {
    hipLaunchKernelGGL(kernel_of(g), dim3(group_grid(a.n, CAL_THREADS, g, wg_max)), dim3(CAL_THREADS), 0, st, a);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------ the negative log-likelihood at S temperatures
struct NllArgs {
  const float* probs; const long long* row; const long long* truth;
  int n, K, S;
  float beta[NLL_SMAX];
  u64* sums;
};

__global__ __launch_bounds__(CAL_THREADS) void nll_temps_kernel(NllArgs a) {
  __shared__ u64 fold[CAL_THREADS / 64][64];
  __shared__ unsigned left_w[CAL_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = uni32(tid >> 6);
  const int K = a.K, n = a.n, S = a.S;
  const bool kv = lane < K;
  // lane s holds beta_s (selected with constant indices: a run-time index into a kernel argument would send the array
  // through scratch); lanes >= S walk beta = 1 and add nowhere
  float beta = 1.f;
#pragma unroll
  for (int l = 0; l < NLL_SMAX; ++l) beta = (lane == l && l < S) ? a.beta[l] : beta;
  long long acc = 0;
  unsigned left = 0;
  // item i's truth and this lane's class value (i and t are the same in every lane of the wave; padding lanes hold 0:
  // logf(0) = -inf, never the maximum)
  auto fetch = [&](long long i, long long& t, float& p) {
    t = uni64(a.truth[i]);
    const long long r = a.row ? uni64(a.row[i]) : i;
    p = kv ? a.probs[r * K + lane] : 0.f;
  };
  const long long stride = (long long)gridDim.x * (CAL_THREADS / 64);
  long long t_next = -1; float p_next = 0.f;
  if ((long long)blockIdx.x * (CAL_THREADS / 64) + wave < n) fetch((long long)blockIdx.x * (CAL_THREADS / 64) + wave, t_next, p_next);
  for (long long i = (long long)blockIdx.x * (CAL_THREADS / 64) + wave; i < n; i += stride) {
    const long long t = t_next;
    const float p = p_next;
    if (i + stride < n) fetch(i + stride, t_next, p_next);      // in flight while this row's chains run
    if (t < 0 || t >= K) continue;                      // unknown truth: skipped
    const float pt = __shfl(p, (int)t, 64);
    const bool bad = __ballot(kv && (p != p || p < 0.f || p == INFINITY)) != 0ull;
    if (bad || !(pt > 0.f)) { left += 1u; continue; }   // (uniform)
    const float l = logf(p);
    const float m = wave_max(l);                        // (finite: p_t > 0)
    const float lt = __shfl(l, (int)t, 64);
    float z = 0.f;
    for (int c = 0; c < K; ++c) {                       // ascending; c is uniform: class c's logarithm comes from lane c
      const float lc = __shfl(l, c, 64);
      z = z + expf(__fmul_rn(beta, __fsub_rn(lc, m)));
    }
    const float nll = __fsub_rn(logf(z), __fmul_rn(beta, __fsub_rn(lt, m)));
    acc += llrintf(nll * FIX20);
  }
  fold[wave][lane] = (u64)acc;
  if (lane == 0) left_w[wave] = left;
  __syncthreads();
  if (tid < S) {                                        // (S <= 64: inside d_sums[2][S])
    u64 v = 0ull, lo = 0ull;
#pragma unroll
    for (int w = 0; w < CAL_THREADS / 64; ++w) { v += fold[w][tid]; lo += left_w[w]; }
    if (v != 0ull) atomicAdd(&a.sums[tid], v);
    if (lo != 0ull) atomicAdd(&a.sums[S + tid], lo);
  }
}

}  // namespace
}  // namespace cmlpl

extern "C" int cmlpl_reliability(const float* d_probs, int K, const int64_t* d_row, const int64_t* d_truth, int n, int bins,
                                 int64_t* d_counts, void* stream) {
  using namespace cmlpl;
  if (!d_probs || !d_truth || !d_counts || n < 1 || K < 1 || K > CAL_KMAX || bins < 1 || bins > REL_BINS_MAX) return CMLPL_E_ARG;
  if (!aligned_to(3, d_probs) || !aligned_to(7, d_row, d_truth, d_counts)) return CMLPL_E_ARG;
  RelArgs a = {};
  a.probs = d_probs; a.row = reinterpret_cast<const long long*>(d_row); a.truth = reinterpret_cast<const long long*>(d_truth);
  a.n = n; a.K = K; a.B = bins; a.counts = reinterpret_cast<u64*>(d_counts);
  const hipError_t e = launch_rows(a, REL_WG_MAX, (hipStream_t)stream, [](auto g) { return reliability_kernel<g>; });
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int cmlpl_temper_probs(const float* d_probs, int n, int K, float beta, float* d_out_probs, int64_t* d_labels,
                                  float* d_conf, float* d_entropy, void* stream) {
  using namespace cmlpl;
  if (!d_probs || n < 1 || K < 1 || K > CAL_KMAX || !(beta > 0.f) || !std::isfinite(beta)) return CMLPL_E_ARG;
  if (!aligned_to(3, d_probs, d_out_probs, d_conf, d_entropy) || !aligned_to(7, d_labels)) return CMLPL_E_ARG;
  TmpArgs a = {};
  a.probs = d_probs; a.n = n; a.K = K; a.beta = beta;
  a.out = d_out_probs; a.labels = reinterpret_cast<long long*>(d_labels); a.conf = d_conf; a.entropy = d_entropy;
  const hipError_t e = launch_rows(a, TMP_WG_MAX, (hipStream_t)stream, [](auto g) { return temper_kernel<g>; });
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int cmlpl_nll_temps(const float* d_probs, int K, const int64_t* d_row, const int64_t* d_truth, int n,
                               const float* betas, int S, int64_t* d_sums, void* stream) {
  using namespace cmlpl;
  if (!d_probs || !d_truth || !betas || !d_sums || n < 1 || K < 1 || K > CAL_KMAX || S < 1 || S > NLL_SMAX) return CMLPL_E_ARG;
  if (!aligned_to(3, d_probs) || !aligned_to(7, d_row, d_truth, d_sums)) return CMLPL_E_ARG;
  NllArgs a = {};
  for (int s = 0; s < S; ++s) {
    if (!(betas[s] >= 0.0625f && betas[s] <= 16.f)) return CMLPL_E_ARG;     // (a NaN fails the comparison)
    a.beta[s] = betas[s];
  }
  a.probs = d_probs; a.row = reinterpret_cast<const long long*>(d_row); a.truth = reinterpret_cast<const long long*>(d_truth);
  a.n = n; a.K = K; a.S = S; a.sums = reinterpret_cast<u64*>(d_sums);
  long long wgs = ((long long)n + CAL_THREADS / 64 - 1) / (CAL_THREADS / 64);
  if (wgs > NLL_WG_MAX) wgs = NLL_WG_MAX;
  hipLaunchKernelGGL(nll_temps_kernel, dim3((unsigned)wgs), dim3(CAL_THREADS), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
