// The lane scheme of the per-row prediction products (ensemble.hip, calibrate.hip, superpixel.hip's broadcast,
// labelprop.hip's step and finish), stated and implemented once.
//
// A group of G lanes per row, G the smallest power of two >= K (1 .. 64): a wave holds 64 / G rows, lane c of a group
// owns class c, padding lanes carry -inf into the maxima and 0 into the sums and never store.  Every reduction is a
// __shfl_xor butterfly of width G: both partners of a stage add (or compare) the same two values, so every lane of a
// group ends with the same bits, in an order that depends on G alone -- the results are the same bytes on every run,
// whatever the grid.  A kernel's trip count is the same for every lane of a workgroup, so the shuffles and ballots always
// meet whole waves.  `shift` is the first lane of a group within its wave, (tid & 63) & ~(G - 1).
//
// THE FIRST-MAXIMUM RULE (torch.max(v, 1)[1]): the label of a row is the first index of its maximum; a NaN counts as the
// maximum and the first NaN wins.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

namespace cmlpl {

template <int G> __device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G> __device__ __forceinline__ float group_max(float v) {     // (fmaxf: the maximum of what is not NaN)
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G> __device__ __forceinline__ unsigned long long group_mask() {
  return G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
}
// the first-maximum rule on the row a group holds one class per lane.  mx = group_max(v); kv = this lane owns a class;
// -1 when no lane of the group does
template <int G> __device__ __forceinline__ int group_argmax(float v, float mx, bool kv, int shift) {
  const unsigned long long nanb = (__ballot(kv && v != v) >> shift) & group_mask<G>();
  const unsigned long long eqb = (__ballot(kv && v == mx) >> shift) & group_mask<G>();
  return __ffsll((long long)(nanb ? nanb : eqb)) - 1;
}
template <int G> __device__ __forceinline__ bool group_any(bool f, int shift) {
  return ((__ballot(f) >> shift) & group_mask<G>()) != 0ull;
}

// f(std::integral_constant<int, G>) for the G of K; what f returns
template <class F> auto with_group(int K, F&& f) {
  if (K <= 1) return f(std::integral_constant<int, 1>{});
  if (K <= 2) return f(std::integral_constant<int, 2>{});
  if (K <= 4) return f(std::integral_constant<int, 4>{});
  if (K <= 8) return f(std::integral_constant<int, 8>{});
  if (K <= 16) return f(std::integral_constant<int, 16>{});
  if (K <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

// workgroups of `threads` lanes that hold n rows at threads / G rows each; past wg_max the kernel strides over the rows
inline unsigned group_grid(long long n, int threads, int G, long long wg_max = INT64_MAX) {
  const int rows = threads / G;
  const long long wgs = (n + rows - 1) / rows;
  return (unsigned)(wgs > wg_max ? wg_max : wgs);
}

// no pointer has a bit of `mask` set (a null pointer passes)
template <class... P> bool aligned_to(uintptr_t mask, const P*... ptrs) {
  return ((uintptr_t(0) | ... | reinterpret_cast<uintptr_t>(ptrs)) & mask) == 0;
}

}  // namespace cmlpl
