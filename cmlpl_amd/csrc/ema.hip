// Exponential moving average of the weights, the "teacher" (reference tools/models.py:155-164 WeightEMA_BN):
//   ema[i] = fl( fl(src[i] * oma) + fl(ema[i] * alpha) ),   alpha = (float)a, oma = (float)(1.0 - a)
// THREE separately rounded fp32 operations, as `Base * (1 - alpha) + Ensemble * alpha` on fp32 tensors rounds: two tensor
// products, then their sum.  Contracted into an FMA the result differs from the reference's in 8-13 % of the elements
// (alpha 0.9 .. 0.999, magnitudes 1e-6 .. 1e3; docs/EXPERIMENTS.md), so the arithmetic is compiled with contraction off
// (hipcc's default contracts across statements, and __fmul_rn / __fadd_rn are plain operators here: they do not hold it
// back).
// One contiguous range, streamed once: 16-byte accesses over the part where both pointers are 16-byte aligned together,
// single floats for the head in front of it and the tail behind it -- or for the whole range when the two pointers are
// not aligned alike (the module path hands over single tensors at any 4-byte offset).  Each element is read before it is
// written, by the thread that writes it: d_src == d_ema is allowed.  No atomics, no workspace, no synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "kernels.hpp"

namespace cmlpl {
namespace {

constexpr int EMA_THREADS = 256;
constexpr int EMA_WG_MAX = 2048;      // past EMA_WG_MAX * 256 vectors the grid strides over the range

__device__ __forceinline__ float ema_mix(float s, float e, float alpha, float oma) {
#pragma clang fp contract(off)
  const float a = s * oma;
  const float b = e * alpha;
  return a + b;
}

// elements [0, head) and [head + 4 nvec, count) one float at a time, [head, head + 4 nvec) as nvec float4 (nvec == 0: the
// whole range by single floats)
__global__ __launch_bounds__(EMA_THREADS) void ema_kernel(const float* src, float* ema, long long count, long long head,
                                                          long long nvec, float alpha, float oma) {
  const long long tid = (long long)blockIdx.x * EMA_THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * EMA_THREADS;
  const float4* s4 = reinterpret_cast<const float4*>(src + head);
  float4* e4 = reinterpret_cast<float4*>(ema + head);
  for (long long i = tid; i < nvec; i += stride) {
    const float4 s = s4[i];
    float4 e = e4[i];
    e.x = ema_mix(s.x, e.x, alpha, oma);
    e.y = ema_mix(s.y, e.y, alpha, oma);
    e.z = ema_mix(s.z, e.z, alpha, oma);
    e.w = ema_mix(s.w, e.w, alpha, oma);
    e4[i] = e;
  }
  const long long rest = count - 4 * nvec;
  for (long long i = tid; i < rest; i += stride) {
    const long long j = i < head ? i : i + 4 * nvec;
    ema[j] = ema_mix(src[j], ema[j], alpha, oma);
  }
}

}  // namespace

hipError_t launch_ema(const float* src, float* ema, long long count, float alpha, float oma, hipStream_t st) {
  if (count <= 0) return hipSuccess;
  long long head = 0, nvec = 0;
  const uintptr_t ps = reinterpret_cast<uintptr_t>(src), pe = reinterpret_cast<uintptr_t>(ema);
  if ((ps & 15) == (pe & 15)) {         // aligned alike: the same head brings both to a 16-byte boundary
    head = (long long)(((16 - (pe & 15)) & 15) / 4);
    if (head > count) head = count;
    nvec = (count - head) / 4;
  }
  const long long rest = count - 4 * nvec;
  const long long items = nvec > rest ? nvec : rest;
  long long wgs = (items + EMA_THREADS - 1) / EMA_THREADS;
  if (wgs > EMA_WG_MAX) wgs = EMA_WG_MAX;
  hipLaunchKernelGGL(ema_kernel, dim3((unsigned)wgs), dim3(EMA_THREADS), 0, st, src, ema, count, head, nvec, alpha, oma);
  return hipGetLastError();
}

}  // namespace cmlpl

extern "C" int cmlpl_ema_update(const float* d_src, float* d_ema, int64_t count, double alpha, void* stream) {
  if (count < 0 || !(alpha >= 0.0 && alpha <= 1.0)) return CMLPL_E_ARG;      // (a NaN alpha fails both comparisons)
  if (count == 0) return 0;
  if (!d_src || !d_ema) return CMLPL_E_ARG;
  if ((reinterpret_cast<uintptr_t>(d_src) | reinterpret_cast<uintptr_t>(d_ema)) & 3) return CMLPL_E_ARG;
  const hipError_t e = cmlpl::launch_ema(d_src, d_ema, (long long)count, (float)alpha, (float)(1.0 - alpha),
                                         (hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}
