// Ensemble prediction of 1..4 networks' logits: what lies between the eval forward's logits and a result.  Per pixel i:
//   p_m      = softmax(z_m[i]) in fp32, the maximum subtracted first, expf and a division as in cps_loss.hip --
//              torch.softmax's semantics: a member row that holds a NaN or a +inf is NaN everywhere, -inf logits give 0
//   p        = sum_m w_m p_m, m ascending; the weights arrive by value, normalised on the host (in double, then rounded)
//   label    = the FIRST maximum of p; a NaN counts as the maximum and the first NaN wins (torch.max's rule, as in
//              cmlpl_infer_cube)
//   conf     = p[label]
//   entropy  = -sum_c p_c logf(p_c), 0 log 0 = 0; NaN when p is NaN
//   disagree = the number of members whose own label (the same rule on p_m) is not `label`
//
// A group of G lanes per pixel in rowgroup.hpp's lane scheme: the results are the same bytes on every run, whatever the
// grid.  No LDS, no atomics, no scratch; a grid-stride loop over blocks of 256 / G pixels, whose trip count is the same
// for every lane of a workgroup (the shuffles are never divergent); plain loads and stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int ENS_THREADS = 256;
constexpr int ENS_MAX_MEMBERS = 4;
constexpr int ENS_WG_MAX = 4096;      // past ENS_WG_MAX workgroups the grid strides over the pixels

struct EnsArgs {
  const float* logits; long long member_stride;
  float w[ENS_MAX_MEMBERS];
  int members, n, K;
  long long* labels; float* probs; float* conf; float* entropy; int* disagree;
};

template <int G> __global__ __launch_bounds__(ENS_THREADS) void ensemble_kernel(EnsArgs a) {
  constexpr int PPW = ENS_THREADS / G;                  // pixels per workgroup and trip
  const int tid = threadIdx.x;
  const int c = tid & (G - 1);                          // the class this lane owns
  const int shift = (tid & 63) & ~(G - 1);              // the first lane of this group within its wave
  const int K = a.K, n = a.n;
  const bool kv = c < K;
  const float NEG_INF = -INFINITY;
  for (long long base = (long long)blockIdx.x * PPW; base < n; base += (long long)gridDim.x * PPW) {
    const long long i = base + tid / G;
    const bool live = kv && i < n;                      // (a group past the last pixel runs on padding and stores nothing)
    float p = 0.f;
    int lab_m[ENS_MAX_MEMBERS] = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < ENS_MAX_MEMBERS; ++m) {
      if (m < a.members) {
        const float z = live ? a.logits[m * a.member_stride + i * K + c] : NEG_INF;
        const float mx = group_max<G>(z);
        const float e = live ? expf(z - mx) : 0.f;
        const float s = group_sum<G>(e);
        const float pm = live ? e / s : 0.f;
        lab_m[m] = group_argmax<G>(pm, group_max<G>(pm), kv, shift);
        p += a.w[m] * pm;
      }
    }
    const int label = group_argmax<G>(p, group_max<G>(p), kv, shift);
    const float plab = __shfl(p, shift + label, 64);
    const float t = (p == 0.f) ? 0.f : p * logf(p);     // (a NaN p is not 0: it goes through)
    const float ent = 0.f - group_sum<G>(kv ? t : 0.f);
    if (live) {
      if (a.probs != nullptr) a.probs[i * K + c] = p;
      if (c == 0) {
        a.labels[i] = label;
        if (a.conf != nullptr) a.conf[i] = plab;
        if (a.entropy != nullptr) a.entropy[i] = ent;
        if (a.disagree != nullptr) {
          int d = 0;
#pragma unroll
          for (int m = 0; m < ENS_MAX_MEMBERS; ++m) d += (m < a.members && lab_m[m] != label) ? 1 : 0;
          a.disagree[i] = d;
        }
      }
    }
  }
}

// ---- members x views blocks (test-time augmentation: every member scores several noisy views of a pixel; include/cmlpl.h,
// cmlpl_ensemble_views).  The same lane scheme with a RUN-TIME loop over the blocks, m ascending and within m v ascending:
//   weights   lane l of every wave holds w_l (selected once from the by-value array with constant indices: a run-time
//             index into a kernel argument would send the array through scratch); a member's weight is read from lane m
//   disagree  lane c counts the blocks whose own label is c; the count of the final label's lane is read at the end --
//             64 blocks need no array of their labels
constexpr int ENS_MAX_BLOCKS = 64;
struct EnsViewsArgs {
  const float* logits; long long member_stride, view_stride;
  float w[ENS_MAX_BLOCKS];                // per MEMBER: fl32(w_m / sum w / views)
  int members, views, n, K;
  long long* labels; float* probs; float* conf; float* entropy; int* disagree;
};

template <int G> __global__ __launch_bounds__(ENS_THREADS) void ensemble_views_kernel(EnsViewsArgs a) {
  constexpr int PPW = ENS_THREADS / G;
  const int tid = threadIdx.x;
  const int c = tid & (G - 1);
  const int shift = (tid & 63) & ~(G - 1);
  const int K = a.K, n = a.n;
  const bool kv = c < K;
  const float NEG_INF = -INFINITY;
  float wl = 0.f;
#pragma unroll
  for (int l = 0; l < ENS_MAX_BLOCKS; ++l) wl = ((tid & 63) == l) ? a.w[l] : wl;
  for (long long base = (long long)blockIdx.x * PPW; base < n; base += (long long)gridDim.x * PPW) {
    const long long i = base + tid / G;
    const bool live = kv && i < n;
    float p = 0.f;
    int mine = 0;                                         // blocks whose own label is class c
    for (int m = 0; m < a.members; ++m) {                 // (uniform)
      const float wm = __shfl(wl, m, 64);
      const float* zm = a.logits + m * a.member_stride;
      for (int v = 0; v < a.views; ++v) {
        const float z = live ? zm[v * a.view_stride + i * K + c] : NEG_INF;
        const float mx = group_max<G>(z);
        const float e = live ? expf(z - mx) : 0.f;
        const float s = group_sum<G>(e);
        const float pm = live ? e / s : 0.f;
        mine += (group_argmax<G>(pm, group_max<G>(pm), kv, shift) == c) ? 1 : 0;
        p += wm * pm;
      }
    }
    const int label = group_argmax<G>(p, group_max<G>(p), kv, shift);
    const float plab = __shfl(p, shift + label, 64);
    const int agree = __shfl(mine, shift + label, 64);
    const float t = (p == 0.f) ? 0.f : p * logf(p);
    const float ent = 0.f - group_sum<G>(kv ? t : 0.f);
    if (live) {
      if (a.probs != nullptr) a.probs[i * K + c] = p;
      if (c == 0) {
        a.labels[i] = label;
        if (a.conf != nullptr) a.conf[i] = plab;
        if (a.entropy != nullptr) a.entropy[i] = ent;
        if (a.disagree != nullptr) a.disagree[i] = a.members * a.views - agree;
      }
    }
  }
}

// the launch of kernel_of(G), the kernel for the G of a.K (rowgroup.hpp), over a.n pixels
template <class Args, class KernelOf> hipError_t launch_ens(const Args& a, hipStream_t st, KernelOf kernel_of) {
  return with_group(a.K, [&](auto g) {
    hipLaunchKernelGGL(kernel_of(g), dim3(group_grid(a.n, ENS_THREADS, g, ENS_WG_MAX)), dim3(ENS_THREADS), 0, st, a);
    return hipGetLastError();
  });
}

// w[m] = fl32(weights[m] / sum / views) in double (nullptr: equal weights); false: a weight that is negative or not
// finite (a NaN fails the comparison), or a sum that is not positive
bool ens_weights(const float* weights, int members, int views, float* w) {
  double sum = 0.0;
  for (int m = 0; m < members; ++m) {
    const double v = weights ? (double)weights[m] : 1.0;
    if (!(v >= 0.0) || !std::isfinite(v)) return false;
    sum += v;
  }
  if (!(sum > 0.0) || !std::isfinite(sum)) return false;
  for (int m = 0; m < members; ++m) w[m] = (float)((weights ? (double)weights[m] : 1.0) / sum / (double)views);
  return true;
}

}  // namespace
}  // namespace cmlpl

extern "C" int cmlpl_ensemble(const float* d_logits, int members, int64_t member_stride, const float* weights, int n, int K,
                              int64_t* d_labels, float* d_probs, float* d_conf, float* d_entropy, int32_t* d_disagree,
                              void* stream) {
  if (members < 1 || members > cmlpl::ENS_MAX_MEMBERS || K < 1 || K > 64 || n < 1) return CMLPL_E_ARG;
  if (!d_logits || !d_labels) return CMLPL_E_ARG;
  if (members > 1 && member_stride < (int64_t)n * K) return CMLPL_E_ARG;          // the members' blocks must not overlap
  if (!cmlpl::aligned_to(3, d_logits, d_probs, d_conf, d_entropy, d_disagree) || !cmlpl::aligned_to(7, d_labels))
    return CMLPL_E_ARG;
  cmlpl::EnsArgs a = {};
  if (!cmlpl::ens_weights(weights, members, 1, a.w)) return CMLPL_E_ARG;
  a.logits = d_logits; a.member_stride = members > 1 ? (long long)member_stride : 0;
  a.members = members; a.n = n; a.K = K;
  a.labels = reinterpret_cast<long long*>(d_labels); a.probs = d_probs; a.conf = d_conf; a.entropy = d_entropy;
  a.disagree = d_disagree;
  const hipError_t e = cmlpl::launch_ens(a, (hipStream_t)stream, [](auto g) { return cmlpl::ensemble_kernel<g>; });
  return e == hipSuccess ? 0 : (int)e;
}

extern "C" int cmlpl_ensemble_views(const float* d_logits, int members, int views, int64_t member_stride, int64_t view_stride,
                                    const float* weights, int n, int K, int64_t* d_labels, float* d_probs, float* d_conf,
                                    float* d_entropy, int32_t* d_disagree, void* stream) {
  if (members < 1 || views < 1 || members > cmlpl::ENS_MAX_BLOCKS || views > cmlpl::ENS_MAX_BLOCKS ||
      members * views > cmlpl::ENS_MAX_BLOCKS || K < 1 || K > 64 || n < 1)
    return CMLPL_E_ARG;
  if (!d_logits || !d_labels) return CMLPL_E_ARG;
  {  // the blocks must not overlap: views inside members, or members inside views (a stride whose count is 1 is ignored)
    const int64_t B = (int64_t)n * K;
    const int64_t ms = members > 1 ? member_stride : 0, vs = views > 1 ? view_stride : 0;
    const bool v_in_m = (views == 1 || vs >= B) && (members == 1 || ms >= (views == 1 ? B : (int64_t)views * vs));
    const bool m_in_v = (members == 1 || ms >= B) && (views == 1 || vs >= (members == 1 ? B : (int64_t)members * ms));
    if (!v_in_m && !m_in_v) return CMLPL_E_ARG;
  }
  if (!cmlpl::aligned_to(3, d_logits, d_probs, d_conf, d_entropy, d_disagree) || !cmlpl::aligned_to(7, d_labels))
    return CMLPL_E_ARG;
  cmlpl::EnsViewsArgs a = {};
  if (!cmlpl::ens_weights(weights, members, views, a.w)) return CMLPL_E_ARG;
  a.logits = d_logits;
  a.member_stride = members > 1 ? (long long)member_stride : 0; a.view_stride = views > 1 ? (long long)view_stride : 0;
  a.members = members; a.views = views; a.n = n; a.K = K;
  a.labels = reinterpret_cast<long long*>(d_labels); a.probs = d_probs; a.conf = d_conf; a.entropy = d_entropy;
  a.disagree = d_disagree;
  const hipError_t e = cmlpl::launch_ens(a, (hipStream_t)stream, [](auto g) { return cmlpl::ensemble_views_kernel<g>; });
  return e == hipSuccess ? 0 : (int)e;
}
