// The pseudo-label monitor: a step's targets scored against the truth of its unlabelled rows (include/cmlpl.h, "THE
// DEFINITION OF THE PSEUDO-LABEL COUNTERS").  It READS the step's four probability blocks [4][btu][K] (or CPS's hard
// labels [2][btu]) and ADDS to a block of int64 counters; it writes nothing the step reads, so the step is what it is
// without it.
//   One wavefront per row i, four rows per workgroup.
//   Row part: lanes = classes (K <= 64).  The first maximum is the lowest set bit of ballot(value == wave maximum); a NaN
//   anywhere in the row is a ballot too.  The flags of a row are uniform over its wave.
//   Pair part: lanes stride the columns j; q = the fp32 chain of graph_loss_kernel (k ascending, one fmaf per class),
//   every count a popcount of a ballot, kept in scalar registers.
//   A wave leaves its 24 head counters in LDS; threads 0 .. 23 fold the four waves and issue ONE 64-bit integer atomicAdd
//   per non-zero counter and workgroup.  A selected row adds one integer atomic to its confusion cell.  Integer sums only:
//   the result is exact and does not depend on the order the adds arrive in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "common.hpp"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int PL_KMAX = 64;          // the loss block's class limit
constexpr int PL_WAVES = 4;          // rows per workgroup
constexpr int PL_SLOTS = 24;         // head counters a launch can touch: two directions x 8, the graph's 8
constexpr int PL_WG_MAX = 65535;     // past PL_WG_MAX * 4 rows the workgroups stride over the rows

typedef unsigned long long u64;

__device__ __forceinline__ int popc(u64 b) { return __popcll(b); }

// head counters of one direction of one row, from its flags
struct RowFlags { bool nan, sel, hit_raw, hit; int l; };

// p, p0: this lane's class of the row (lanes >= K: -inf, never the first maximum of a row with a finite entry)
__device__ __forceinline__ RowFlags row_flags(float p, float p0, bool kv, int t, float adap_mask) {
  RowFlags f;
  const u64 valid = __ballot(kv);
  f.nan = (__ballot(kv && (p != p || p0 != p0)) != 0ull);
  const float mx = wave_max(p), mx0 = wave_max(p0);
  const u64 b = __ballot(kv && p == mx) & valid, b0 = __ballot(kv && p0 == mx0) & valid;
  if (b == 0ull || b0 == 0ull) f.nan = true;            // (no lane holds the maximum: only a NaN row can do that)
  f.l = f.nan ? 0 : (int)__ffsll((long long)b) - 1;
  const int l0 = f.nan ? 0 : (int)__ffsll((long long)b0) - 1;
  f.sel = !f.nan && mx >= adap_mask;                    // the step's mask: wave_max(p) >= adap_mask in fp32
  f.hit_raw = !f.nan && l0 == t;
  f.hit = !f.nan && f.l == t;
  return f;
}

__global__ __launch_bounds__(64 * PL_WAVES) void pl_stats_kernel(const float* __restrict__ probs, int btu, int K,
                                                                const long long* __restrict__ truth,
                                                                const long long* __restrict__ idx, float adap_mask,
                                                                float pos_thr, float neg_thr, u64* __restrict__ counts) {
  __shared__ unsigned int head[PL_WAVES][PL_SLOTS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool kv = lane < K;
  const float NEGINF = -__builtin_inff();
  unsigned int c[PL_SLOTS];
#pragma unroll
  for (int s = 0; s < PL_SLOTS; ++s) c[s] = 0u;
  const long long blk = (long long)btu * K;             // one probability block
  for (long long i = (long long)blockIdx.x * PL_WAVES + wave; i < btu; i += (long long)gridDim.x * PL_WAVES) {
    // (every load of the row is issued in front of the first use of the truth: the two dependent reads idx -> truth
    //  would otherwise stand in front of everything else)
    float pr[2], pr0[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      pr[d] = kv ? probs[(long long)d * blk + i * K + lane] : NEGINF;
      pr0[d] = kv ? probs[(long long)(2 + d) * blk + i * K + lane] : NEGINF;
    }
    const long long ti = truth[idx ? idx[i] : i];
    if (ti < 0 || ti >= K) continue;                    // unknown truth: the row contributes nothing anywhere
    const int t = (int)ti;
    // ---- the row part, both directions: d = 0 (p_w, p_w0) = blocks 0 and 2, d = 1 (p_s, p_s0) = blocks 1 and 3
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const RowFlags f = row_flags(pr[d], pr0[d], kv, t, adap_mask);
      c[8 * d + 0] += 1u;
      if (f.nan) { c[8 * d + 1] += 1u; continue; }
      c[8 * d + 2] += f.sel ? 1u : 0u;
      c[8 * d + 3] += f.hit_raw ? 1u : 0u;
      c[8 * d + 4] += f.hit ? 1u : 0u;
      c[8 * d + 5] += (f.sel && f.hit) ? 1u : 0u;
      c[8 * d + 6] += (!f.hit_raw && f.hit) ? 1u : 0u;
      c[8 * d + 7] += (f.hit_raw && !f.hit) ? 1u : 0u;
      if (f.sel && lane == 0 && f.l >= 0 && f.l < K)    // (t and l are inside [0, K): the cell is inside cm[d])
        atomicAdd(&counts[CMLPL_PL_HEAD + ((long long)d * K + t) * K + f.l], 1ull);
    }
    // ---- the pair part: ordered pairs (i, j), j != i, both truths known; q = sum_k p_s[i][k] p_w[j][k]
    const float* psi = probs + blk + i * K;
    for (long long j0 = 0; j0 < btu; j0 += 64) {
      const long long j = j0 + lane;
      const long long jc = j < btu ? j : (long long)btu - 1;      // lanes past the last row read it again and count nothing
      // (the chain does not wait for the truth: its loads are in flight beside the two dependent reads idx -> truth)
      const long long tj = truth[idx ? idx[jc] : jc];
      const float* pwj = probs + jc * K;
      float q = 0.f;
      for (int k = 0; k < K; ++k) q = fmaf(psi[k], pwj[k], q);
      const bool on = j < btu && j != i && tj >= 0 && tj < K;
      const bool qnan = q != q, same = tj == ti;
      const bool isp = on && !qnan && q >= pos_thr, isn = on && !qnan && q <= neg_thr;
      c[16] += (unsigned)popc(__ballot(on));
      c[17] += (unsigned)popc(__ballot(on && qnan));
      c[18] += (unsigned)popc(__ballot(isp));
      c[19] += (unsigned)popc(__ballot(isp && same));
      c[20] += (unsigned)popc(__ballot(isn));
      c[21] += (unsigned)popc(__ballot(isn && !same));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < PL_SLOTS; ++s) head[wave][s] = c[s];
  }
  __syncthreads();
  if (tid < PL_SLOTS) {
    u64 v = 0;
#pragma unroll
    for (int w = 0; w < PL_WAVES; ++w) v += head[w][tid];
    if (tid == 22 && blockIdx.x == 0) v = 1;            // launches folded in
    if (v != 0) atomicAdd(&counts[tid], v);
  }
}

// CPS: hard labels [2][btu]; one thread per (direction, row)
__global__ __launch_bounds__(256) void pl_stats_hard_kernel(const long long* __restrict__ pseudo, int btu, int K,
                                                            const long long* __restrict__ truth,
                                                            const long long* __restrict__ idx, u64* __restrict__ counts) {
  __shared__ unsigned int head[4][8];                   // per wave: [d][rows, nan_rows, sel, hit]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  unsigned int c[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) c[s] = 0u;
  const long long total = 2LL * btu;
  // (every lane of a wave makes the same number of trips: the ballots below meet whole waves)
  for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
    const long long e = base + tid;
    const bool in = e < total;
    const int d = (in && e >= btu) ? 1 : 0;
    const long long r = in ? e - (long long)d * btu : 0;
    long long t = -1, l = -1;
    if (in) { t = truth[idx ? idx[r] : r]; l = pseudo[e]; }
    const bool known = in && t >= 0 && t < K;
    const bool bad = known && (l < 0 || l >= K);
    const bool sel = known && !bad, hit = sel && l == t;
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
      c[4 * dd + 0] += (unsigned)popc(__ballot(known && d == dd));
      c[4 * dd + 1] += (unsigned)popc(__ballot(bad && d == dd));
      c[4 * dd + 2] += (unsigned)popc(__ballot(sel && d == dd));
      c[4 * dd + 3] += (unsigned)popc(__ballot(hit && d == dd));
    }
    if (sel) atomicAdd(&counts[CMLPL_PL_HEAD + ((long long)d * K + t) * K + l], 1ull);   // (t and l inside [0, K))
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < 8; ++s) head[wave][s] = c[s];
  }
  __syncthreads();
  if (tid < 16) {
    // slot 8 d + s of the head: rows, nan_rows, sel, then hit_raw = hit = sel_hit; fixed = broken = 0
    const int d = tid >> 3, s = tid & 7;
    const int from = s < 3 ? s : (s < 6 ? 3 : -1);
    u64 v = 0;
    if (from >= 0)
      for (int w = 0; w < 4; ++w) v += head[w][4 * d + from];
    if (v != 0) atomicAdd(&counts[tid], v);
  }
  if (tid == 22 && blockIdx.x == 0) atomicAdd(&counts[22], 1ull);
}

int chk(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

}  // namespace
}  // namespace cmlpl

extern "C" int cmlpl_pl_stats(const float* d_probs, int btu, int K, const int64_t* d_truth, const int64_t* d_idx,
                              float adap_mask, float pos_thr, float neg_thr, int64_t* d_counts, void* stream) {
  using namespace cmlpl;
  if (!d_probs || !d_truth || !d_counts || btu < 1 || K < 1 || K > PL_KMAX) return CMLPL_E_ARG;
  if (!aligned_to(3, d_probs) || !aligned_to(7, d_truth, d_idx, d_counts)) return CMLPL_E_ARG;
  long long wgs = ((long long)btu + PL_WAVES - 1) / PL_WAVES;
  if (wgs > PL_WG_MAX) wgs = PL_WG_MAX;
  hipLaunchKernelGGL(pl_stats_kernel, dim3((unsigned)wgs), dim3(64 * PL_WAVES), 0, (hipStream_t)stream, d_probs, btu, K,
                     (const long long*)d_truth, (const long long*)d_idx, adap_mask, pos_thr, neg_thr, (u64*)d_counts);
  return chk(hipGetLastError());
}

extern "C" int cmlpl_pl_stats_hard(const int64_t* d_pseudo, int btu, int K, const int64_t* d_truth, const int64_t* d_idx,
                                   int64_t* d_counts, void* stream) {
  using namespace cmlpl;
  if (!d_pseudo || !d_truth || !d_counts || btu < 1 || K < 1 || K > PL_KMAX) return CMLPL_E_ARG;
  if (!aligned_to(7, d_pseudo, d_truth, d_idx, d_counts)) return CMLPL_E_ARG;
  long long wgs = (2LL * btu + 255) / 256;
  if (wgs > PL_WG_MAX) wgs = PL_WG_MAX;
  hipLaunchKernelGGL(pl_stats_hard_kernel, dim3((unsigned)wgs), dim3(256), 0, (hipStream_t)stream,
                     (const long long*)d_pseudo, btu, K, (const long long*)d_truth, (const long long*)d_idx, (u64*)d_counts);
  return chk(hipGetLastError());
}
