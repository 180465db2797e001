// Confusion matrix on the device (what the reference rebuilds on the host from a label image: tools/hyper_tools.py
// CalAccuracy; test_acc :372-413 counts its diagonal and row sums batch by batch):
//   cm[net][t][p] += #{ i : truth[i] == t, pred[net][i] == p }      int64, row = true class, column = predicted class
// One K x K int32 tile per workgroup in LDS (16 KB at K = 64), one LDS atomic per row of the list, then one 64-bit global
// atomic add per non-zero cell.  Integer sums: the result does not depend on the order the adds arrive in, so it is exact
// and the same bytes on every run.  The kernel ACCUMULATES (chunks of a list, or the shares of several ranks, add into one
// matrix); the caller zeroes a fresh one.  Rows whose truth is outside 0 .. K - 1 (the label files' "unlabelled") are
// counted in `ignored` and nowhere else.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmlpl.h"

namespace {

constexpr int KMAX = 64;          // classes (the classifier's limit: route_infer, route_net)
constexpr int ROWS_PER_WG = 4096; // list rows a workgroup counts: 16 per thread (a workgroup's int32 cell cannot overflow)
constexpr int WG_MAX = 1024;      // workgroups per network; past WG_MAX * ROWS_PER_WG rows they stride over the list

inline int chk(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

__global__ __launch_bounds__(256) void confusion_kernel(const long long* __restrict__ pred, const long long* __restrict__ truth,
                                                        int n, int K, unsigned long long* __restrict__ cm,
                                                        unsigned long long* __restrict__ ignored) {
  __shared__ int tile[KMAX * KMAX];
  __shared__ int skipped;
  const int tid = threadIdx.x, net = blockIdx.y, KK = K * K;
  for (int i = tid; i < KK; i += 256) tile[i] = 0;
  if (tid == 0) skipped = 0;
  __syncthreads();
  const long long* P = pred + (long long)net * n;
  // a workgroup takes ROWS_PER_WG consecutive rows at a time (coalesced 8-byte loads), then strides by the grid
  for (long long base = (long long)blockIdx.x * ROWS_PER_WG; base < n; base += (long long)gridDim.x * ROWS_PER_WG) {
    const long long end = base + ROWS_PER_WG < n ? base + ROWS_PER_WG : n;
    for (long long i = base + tid; i < end; i += 256) {
      const long long t = truth[i], p = P[i];
      if (t < 0 || t >= K) {
        if (net == 0) atomicAdd(&skipped, 1);
      } else if (p >= 0 && p < K) {          // (an argmax is in range by construction; anything else must not leave the tile)
        atomicAdd(&tile[(int)t * K + (int)p], 1);
      }
    }
  }
  __syncthreads();
  unsigned long long* out = cm + (long long)net * KK;
  for (int i = tid; i < KK; i += 256) {
    const int v = tile[i];
    if (v != 0) atomicAdd(&out[i], (unsigned long long)v);
  }
  if (tid == 0 && ignored != nullptr && skipped != 0) atomicAdd(ignored, (unsigned long long)skipped);
}

}  // namespace

extern "C" int cmlpl_confusion(const int64_t* d_pred, int nets, const int64_t* d_truth, int n, int K, int64_t* d_cm,
                               int64_t* d_ignored, void* stream) {
  if (!d_pred || !d_truth || !d_cm || n < 1 || nets < 1 || nets > 2 || K < 1 || K > KMAX) return CMLPL_E_ARG;
  int wgs = (n + ROWS_PER_WG - 1) / ROWS_PER_WG;
  if (wgs > WG_MAX) wgs = WG_MAX;
  hipLaunchKernelGGL(confusion_kernel, dim3(wgs, nets), dim3(256), 0, (hipStream_t)stream, (const long long*)d_pred,
                     (const long long*)d_truth, n, K, (unsigned long long*)d_cm, (unsigned long long*)d_ignored);
  return chk(hipGetLastError());
}
