// Superpixels and region votes (include/cmlpl.h, "THE DEFINITION OF A SUPERPIXEL MAP" and "THE DEFINITION OF A REGION
// VOTE"): the scene is over-segmented on the device by SLIC's per-pixel form (gSLIC) and every segment votes as one.
//
// cmlpl_sp_segment, per call:
//   pack     once: the G guide channels of every pixel leave the cube ([pixel][C], a stride of 60 .. 200 floats) for a
//            planar [G][n] block of the workspace, and a byte says whether the pixel is regular.  Every iteration reads
//            the planar block: consecutive lanes, consecutive words.
//   init     one thread per segment: the centre of its cell.
//   assign   a workgroup of 256 threads per tile of 32 x 8 pixels, lanes along x.  The centres of the cells the tile can
//            reach -- its own cells and one ring around them, at most 7 x 19 -- are staged into LDS once; every thread
//            walks its 9 candidates da ascending, db ascending within da, with the pixel's guide in registers.
//   update   one wavefront per segment (S >= 12: a workgroup of four, folded through LDS) gathers over the segment's
//            clipped 3S x 3S block (a segment's pixels lie inside its 3 x 3 block of cells), coalesced along x, four map
//            words requested per trip, int64 accumulators in registers, a __shfl_xor butterfly, one lane forms the
//            centre.  No atomics, no memset; the sums are integers, so the order does not matter.
// cmlpl_sp_vote_probs / cmlpl_sp_vote_labels: the map is arbitrary, so the sums are scattered with 64-bit INTEGER atomics
//   into a zeroed [N][K] table; a run of neighbouring lanes with the same segment (a superpixel map has runs of S) is
//   summed inside the wave first and its first lane issues the atomic.  One thread per segment finishes (q, the first
//   maximum, the entropy c ascending), one group of lanes per pixel (rowgroup.hpp) broadcasts.
// Integer sums only: every output is the same bytes on every run.  Nothing is contracted into a fused multiply-add that
// the definition does not name (the pragma below, and __fmul_rn / __fsub_rn where it matters).  No float atomics, no scratch.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "rowgroup.hpp"

#pragma clang fp contract(off)

namespace cmlpl {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_TX = 32, SP_TY = 8;              // the tile of the assignment
constexpr int SP_MAX_G = 8;
constexpr int SP_CELLS = 7 * 19;                  // (floor(7 / S) + 4) x (floor(31 / S) + 4) cells at S = 2
constexpr int SP_WG_MAX = 65536;
constexpr int SP_WIDE_S = 12;                     // from this step on a whole workgroup gathers one segment
constexpr float SP_FIX24 = 16777216.f;            // 2^24
constexpr float SP_GMAX = 1048576.f;              // 2^20: a regular pixel's guide

typedef long long i64;
typedef unsigned long long u64;

struct SpArgs {
  const float* guide; i64 guide_stride;
  int G, rows, cols, S, ny, nx, n, N, tiles_x;
  float w;
  float* plan;                                    // [G][n]
  unsigned char* flag;                            // [n]: 1 = regular
  float* centres;                                 // [N][2 + G]
  int* seg;                                       // [n]
  float* out_centres; int* out_counts;            // the last update's copies (each or null)
};

__global__ __launch_bounds__(SP_THREADS) void sp_pack_kernel(SpArgs a) {
  const int i = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (i >= a.n) return;
  const float* g = a.guide + (i64)i * a.guide_stride;
  bool reg = true;
  for (int ch = 0; ch < a.G; ++ch) {
    const float v = g[ch];
    reg = reg && (fabsf(v) <= SP_GMAX);           // (a NaN fails the comparison)
    a.plan[(i64)ch * a.n + i] = v;
  }
  a.flag[i] = reg ? 1 : 0;
}

__global__ __launch_bounds__(SP_THREADS) void sp_init_kernel(SpArgs a) {
  const int s = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (s >= a.N) return;
  const int ca = s / a.nx, cb = s - ca * a.nx;
  const int py = min(a.rows - 1, ca * a.S + a.S / 2), px = min(a.cols - 1, cb * a.S + a.S / 2);
  const int i = py * a.cols + px;
  float* c = a.centres + (i64)s * (2 + a.G);
  c[0] = (float)py;
  c[1] = (float)px;
  const bool reg = a.flag[i] != 0;
  for (int ch = 0; ch < a.G; ++ch) c[2 + ch] = reg ? a.plan[(i64)ch * a.n + i] : 0.f;
}

__global__ __launch_bounds__(SP_THREADS) void sp_assign_kernel(SpArgs a) {
  __shared__ float cl[SP_CELLS * (2 + SP_MAX_G)];
  const int tid = threadIdx.x;
  const int G = a.G, S = a.S, CW = 2 + G;
  const int tile_y = (int)blockIdx.x / a.tiles_x, tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
  const int x0 = tile_x * SP_TX, y0 = tile_y * SP_TY;
  const int x1 = min(x0 + SP_TX - 1, a.cols - 1), y1 = min(y0 + SP_TY - 1, a.rows - 1);
  // the cells this tile's pixels can name: their own and one ring, inside the grid (<= 7 rows x 19 columns of cells)
  const int ca0 = max(y0 / S - 1, 0), ca1 = min(y1 / S + 1, a.ny - 1);
  const int cb0 = max(x0 / S - 1, 0), cb1 = min(x1 / S + 1, a.nx - 1);
  const int nb = cb1 - cb0 + 1, words = (ca1 - ca0 + 1) * nb * CW;
  for (int e = tid; e < words; e += SP_THREADS) {
    const int cell = e / CW, k = e - cell * CW;
    const int ra = cell / nb, rb = cell - ra * nb;
    cl[e] = a.centres[((i64)(ca0 + ra) * a.nx + cb0 + rb) * CW + k];
  }
  __syncthreads();
  const int x = x0 + (tid & (SP_TX - 1)), y = y0 + (tid >> 5);
  if (x >= a.cols || y >= a.rows) return;         // (behind the barrier)
  const int i = y * a.cols + x;
  const int pa = y / S, pb = x / S;
  int label = pa * a.nx + pb;
  if (a.flag[i] != 0) {
    float gv[SP_MAX_G];
#pragma unroll
    for (int ch = 0; ch < SP_MAX_G; ++ch) gv[ch] = ch < G ? a.plan[(i64)ch * a.n + i] : 0.f;
    const float fy = (float)y, fx = (float)x;
    float best = INFINITY;
    for (int da = -1; da <= 1; ++da) {
      const int ca = pa + da;
      if (ca < 0 || ca >= a.ny) continue;
      for (int db = -1; db <= 1; ++db) {
        const int cb = pb + db;
        if (cb < 0 || cb >= a.nx) continue;
        const float* c = cl + ((ca - ca0) * nb + (cb - cb0)) * CW;
        float dc2 = 0.f;
#pragma unroll
        for (int ch = 0; ch < SP_MAX_G; ++ch) {
          if (ch < G) {                           // (uniform)
            const float d = __fsub_rn(gv[ch], c[2 + ch]);
            dc2 = fmaf(d, d, dc2);
          }
        }
        const float dy = __fsub_rn(fy, c[0]), dx = __fsub_rn(fx, c[1]);
        const float ds2 = fmaf(dx, dx, __fmul_rn(dy, dy));
        const float D = fmaf(ds2, a.w, dc2);
        if (D < best) { best = D; label = ca * a.nx + cb; }     // (strict: a tie keeps the earlier; NaN and +inf never win)
      }
    }
  }
  a.seg[i] = label;
}

__device__ __forceinline__ i64 wave_sum(i64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// WPS wavefronts per segment: 1 (four segments per workgroup, no barrier) or 4 (the workgroup is one segment's: S >= SP_WIDE_S,
// where a lone wave would walk hundreds of trips one behind the other); the sums are integers, so the split changes no bit
template <int WPS> __global__ __launch_bounds__(SP_THREADS) void sp_update_kernel(SpArgs a) {
  constexpr int TPS = 64 * WPS;                   // threads per segment
  __shared__ i64 part[WPS > 1 ? WPS * (3 + SP_MAX_G) : 1];
  const int lane = threadIdx.x & 63, t = (int)threadIdx.x & (TPS - 1);
  const int s = (int)blockIdx.x * (SP_THREADS / TPS) + (int)threadIdx.x / TPS;
  if (WPS == 1 && s >= a.N) return;               // (a whole wave, and no barrier; WPS == 4: the grid is N workgroups)
  const int G = a.G, S = a.S;
  const int ca = s / a.nx, cb = s - ca * a.nx;
  const int yb0 = max((ca - 1) * S, 0), yb1 = min((ca + 2) * S, a.rows);
  const int xb0 = max((cb - 1) * S, 0), xb1 = min((cb + 2) * S, a.cols);
  const int bw = xb1 - xb0, tot = bw * (yb1 - yb0);
  i64 cnt = 0, sy = 0, sx = 0;
  i64 sg[SP_MAX_G] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int e0 = t; e0 < tot; e0 += 4 * TPS) {     // four pixels per trip: their map words are requested together
    int ys[4], xs[4], sv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = e0 + j * TPS;
      const int ry = e / bw;
      ys[j] = yb0 + ry; xs[j] = xb0 + (e - ry * bw);
      sv[j] = e < tot ? a.seg[ys[j] * a.cols + xs[j]] : -1;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = ys[j] * a.cols + xs[j];
      if (sv[j] == s && a.flag[i] != 0) {
        cnt += 1; sy += ys[j]; sx += xs[j];
#pragma unroll
        for (int ch = 0; ch < SP_MAX_G; ++ch)
          if (ch < G) sg[ch] += llrintf(__fmul_rn(a.plan[(i64)ch * a.n + i], SP_FIX24));   // (the product is exact)
      }
    }
  }
  cnt = wave_sum(cnt); sy = wave_sum(sy); sx = wave_sum(sx);
#pragma unroll
  for (int ch = 0; ch < SP_MAX_G; ++ch)
    if (ch < G) sg[ch] = wave_sum(sg[ch]);        // (uniform)
  if (WPS > 1) {
    const int wv = (int)threadIdx.x >> 6;
    if (lane == 0) {
      i64* p = part + wv * (3 + SP_MAX_G);
      p[0] = cnt; p[1] = sy; p[2] = sx;
#pragma unroll
      for (int ch = 0; ch < SP_MAX_G; ++ch) p[3 + ch] = sg[ch];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int w = 1; w < WPS; ++w) {
      const i64* p = part + w * (3 + SP_MAX_G);
      cnt += p[0]; sy += p[1]; sx += p[2];
#pragma unroll
      for (int ch = 0; ch < SP_MAX_G; ++ch) sg[ch] += p[3 + ch];
    }
  }
  if (lane != 0) return;
  float* c = a.centres + (i64)s * (2 + G);
  if (cnt > 0) {
    const double dn = (double)cnt;
    c[0] = (float)((double)sy / dn);
    c[1] = (float)((double)sx / dn);
#pragma unroll
    for (int ch = 0; ch < SP_MAX_G; ++ch)
      if (ch < G) c[2 + ch] = (float)((double)sg[ch] / (dn * 16777216.0));
  }
  if (a.out_counts != nullptr) a.out_counts[s] = (int)cnt;
  if (a.out_centres != nullptr) {
    float* o = a.out_centres + (i64)s * (2 + G);
    for (int k = 0; k < 2 + G; ++k) o[k] = c[k];
  }
}

// ------------------------------------------------------------------ the vote
struct VoteArgs {
  const int* seg; const float* probs; const i64* src;
  int n, K, N, hard;
  i64* P; i64* cnt;                               // [N][K], [N]: zeroed before the accumulation
  float* qtab; i64* slab; float* sconf; float* sent;      // per segment: [N][K], [N], [N], [N]
  i64* out_P; i64* out_cnt; float* out_qtab; i64* out_slab;   // the optional per-segment outputs
  float* out_probs; i64* labels; float* conf; float* entropy; // the per-pixel outputs (each or null)
};

// the runs of equal keys among the 64 lanes: head = first lane of its run, end = its run's last lane
__device__ __forceinline__ u64 wave_runs(i64 key, int lane, bool& head, int& end) {
  const i64 prev = __shfl_up(key, 1, 64);
  head = lane == 0 || prev != key;
  const u64 hm = __ballot(head);
  const u64 next = lane == 63 ? 0ull : (hm >> (lane + 1));
  end = next ? lane + __ffsll((long long)next) - 1 : 63;
  return hm;
}
// v summed from this lane to the end of its run (the head holds the run's sum)
__device__ __forceinline__ i64 run_sum(i64 v, int lane, int end) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const i64 t = __shfl_down(v, o, 64);
    if (lane + o <= end) v += t;
  }
  return v;
}
__device__ __forceinline__ void add64(i64* p, i64 v) { atomicAdd(reinterpret_cast<u64*>(p), (u64)v); }

__global__ __launch_bounds__(SP_THREADS) void sp_vote_probs_kernel(VoteArgs a) {
  const int lane = threadIdx.x & 63, K = a.K;
  const i64 i = (i64)blockIdx.x * SP_THREADS + threadIdx.x;
  int s = -1;
  if (i < a.n) {
    s = a.seg[i];
    if (s < 0 || s >= a.N) s = -1;
  }
  const float* p = a.probs + i * K;
  if (s >= 0) {
    bool ok = true;
    for (int c = 0; c < K; ++c) {
      const float v = p[c];
      ok = ok && (v >= 0.f && v <= 2.f);          // (a NaN or an infinity fails)
    }
    if (!ok) s = -1;
  }
  bool head; int end;
  const bool merge = wave_runs((i64)s, lane, head, end) != ~0ull;   // (uniform: any run longer than one lane)
  const bool put = head && s >= 0;
  i64 one = s >= 0 ? 1 : 0;
  if (merge) one = run_sum(one, lane, end);
  if (put) add64(a.cnt + s, one);
  for (int c = 0; c < K; ++c) {                   // (uniform)
    i64 v = s >= 0 ? (i64)llrintf(__fmul_rn(p[c], SP_FIX24)) : 0;
    if (merge) v = run_sum(v, lane, end);
    if (put && v != 0) add64(a.P + (i64)s * K + c, v);
  }
}

__global__ __launch_bounds__(SP_THREADS) void sp_vote_labels_kernel(VoteArgs a) {
  const int lane = threadIdx.x & 63, K = a.K;
  const i64 i = (i64)blockIdx.x * SP_THREADS + threadIdx.x;
  int s = -1;
  i64 l = 0;
  if (i < a.n) {
    s = a.seg[i];
    l = a.src[i];
    if (s < 0 || s >= a.N || l < 0 || l >= K) s = -1;
  }
  if (s < 0) l = 0;
  bool head; int end;
  bool merge = wave_runs((i64)s, lane, head, end) != ~0ull;
  i64 one = s >= 0 ? 1 : 0;
  if (merge) one = run_sum(one, lane, end);
  if (head && s >= 0) add64(a.cnt + s, one);
  merge = wave_runs((i64)s * 64 + l, lane, head, end) != ~0ull;
  one = s >= 0 ? 1 : 0;
  if (merge) one = run_sum(one, lane, end);
  if (head && s >= 0) add64(a.P + (i64)s * K + l, one);
}

__global__ __launch_bounds__(SP_THREADS) void sp_vote_finish_kernel(VoteArgs a) {
  const int s = (int)blockIdx.x * SP_THREADS + (int)threadIdx.x;
  if (s >= a.N) return;
  const int K = a.K;
  const i64 cnt = a.cnt[s];
  const i64* P = a.P + (i64)s * K;
  float* q = a.qtab + (i64)s * K;
  if (a.out_cnt != nullptr) a.out_cnt[s] = cnt;
  const float qnan = __builtin_nanf("");
  const double den = (double)cnt * (a.hard ? 1.0 : 16777216.0);
  float best = 0.f, sum = 0.f;
  i64 label = 0;
  for (int c = 0; c < K; ++c) {
    const i64 pc = P[c];
    if (a.out_P != nullptr) a.out_P[(i64)s * K + c] = pc;
    const float qc = cnt > 0 ? (float)((double)pc / den) : qnan;
    q[c] = qc;
    if (a.out_qtab != nullptr) a.out_qtab[(i64)s * K + c] = qc;
    if (c == 0) best = qc;
    else if (qc > best) { best = qc; label = c; }             // (the first maximum)
    sum = __fadd_rn(sum, qc == 0.f ? 0.f : __fmul_rn(qc, logf(qc)));
  }
  if (cnt <= 0) label = -1;
  a.slab[s] = label;
  a.sconf[s] = best;
  a.sent[s] = 0.f - sum;
  if (a.out_slab != nullptr) a.out_slab[s] = label;
}

template <int G> __global__ __launch_bounds__(SP_THREADS) void sp_vote_broadcast_kernel(VoteArgs a) {
  constexpr int PPW = SP_THREADS / G;
  const int tid = threadIdx.x, c = tid & (G - 1), K = a.K;
  const float qnan = __builtin_nanf("");
  for (i64 base = (i64)blockIdx.x * PPW; base < a.n; base += (i64)gridDim.x * PPW) {
    const i64 i = base + tid / G;
    if (i >= a.n) continue;
    int s = a.seg[i];
    const bool in = s >= 0 && s < a.N;
    if (!in) s = 0;
    if (c < K && a.out_probs != nullptr) a.out_probs[i * K + c] = in ? a.qtab[(i64)s * K + c] : qnan;
    if (c == 0) {
      if (a.labels != nullptr) a.labels[i] = in ? a.slab[s] : -1;
      if (a.conf != nullptr) a.conf[i] = in ? a.sconf[s] : qnan;
      if (a.entropy != nullptr) a.entropy[i] = in ? a.sent[s] : qnan;
    }
  }
}

size_t vote_ws_bytes(int N, int K) { return (size_t)12 * (size_t)N * (size_t)(K + 2); }

int vote(const int32_t* d_seg, const float* d_probs, const int64_t* d_src, int n, int K, int N, float* d_out_probs,
         int64_t* d_labels, float* d_conf, float* d_entropy, int64_t* d_sums, int64_t* d_cnt, float* d_seg_probs,
         int64_t* d_seg_labels, void* d_ws, size_t ws_bytes, void* stream) {
  if (n < 1 || N < 1 || K < 1 || K > 64 || (int64_t)N * K > INT32_MAX) return CMLPL_E_ARG;
  if (!d_seg || (!d_probs && !d_src) || !d_ws) return CMLPL_E_ARG;
  if (!d_out_probs && !d_labels && !d_conf && !d_entropy && !d_sums && !d_cnt && !d_seg_probs && !d_seg_labels)
    return CMLPL_E_ARG;
  if (!aligned_to(3, d_seg, d_probs, d_out_probs, d_conf, d_entropy, d_seg_probs) ||
      !aligned_to(7, d_src, d_labels, d_sums, d_cnt, d_seg_labels, d_ws))
    return CMLPL_E_ARG;
  if (ws_bytes < vote_ws_bytes(N, K)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t NK = (size_t)N * K;
  VoteArgs a = {};
  a.seg = d_seg; a.probs = d_probs; a.src = reinterpret_cast<const i64*>(d_src);
  a.n = n; a.K = K; a.N = N; a.hard = d_probs ? 0 : 1;
  a.P = reinterpret_cast<i64*>(d_ws); a.cnt = a.P + NK; a.slab = a.cnt + N;
  a.qtab = reinterpret_cast<float*>(a.slab + N); a.sconf = a.qtab + NK; a.sent = a.sconf + N;
  a.out_P = reinterpret_cast<i64*>(d_sums); a.out_cnt = reinterpret_cast<i64*>(d_cnt); a.out_qtab = d_seg_probs;
  a.out_slab = reinterpret_cast<i64*>(d_seg_labels);
  a.out_probs = d_out_probs; a.labels = reinterpret_cast<i64*>(d_labels); a.conf = d_conf; a.entropy = d_entropy;
  hipError_t e = hipMemsetAsync(d_ws, 0, 8 * (NK + (size_t)N), st);       // (a memset node under capture)
  if (e != hipSuccess) return (int)e;
  const unsigned wg_n = (unsigned)(((i64)n + SP_THREADS - 1) / SP_THREADS);
  if (a.hard) hipLaunchKernelGGL(sp_vote_labels_kernel, dim3(wg_n), dim3(SP_THREADS), 0, st, a);
  else hipLaunchKernelGGL(sp_vote_probs_kernel, dim3(wg_n), dim3(SP_THREADS), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sp_vote_finish_kernel, dim3((unsigned)((N + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  if (d_out_probs || d_labels || d_conf || d_entropy) {
    e = with_group(K, [&](auto g) {
      hipLaunchKernelGGL(sp_vote_broadcast_kernel<g>, dim3(group_grid(n, SP_THREADS, g, SP_WG_MAX)), dim3(SP_THREADS), 0, st, a);
      return hipGetLastError();
    });
  }
  return e == hipSuccess ? 0 : (int)e;
}

// the grid of a scene: false when the definition excludes it
bool sp_grid(int rows, int cols, int G, int S, int* ny, int* nx) {
  if (rows < 1 || cols < 1 || G < 0 || G > SP_MAX_G || S < 2 || S > 64 || (int64_t)rows * cols > INT32_MAX) return false;
  *ny = (rows + S - 1) / S; *nx = (cols + S - 1) / S;
  return (int64_t)*ny * *nx < (1 << 24);
}

}  // namespace
}  // namespace cmlpl

extern "C" size_t cmlpl_sp_workspace_bytes(int rows, int cols, int G, int S) {
  int ny, nx;
  if (!cmlpl::sp_grid(rows, cols, G, S, &ny, &nx)) return 0;
  const size_t n = (size_t)rows * cols, N = (size_t)ny * nx;
  return 4 * (N * (2 + G) + (size_t)G * n) + (n + 3) / 4 * 4;
}

extern "C" int cmlpl_sp_segment(const float* d_guide, int64_t guide_stride, int G, int rows, int cols, int S, float m, int iters,
                                int32_t* d_seg, float* d_centres, int32_t* d_counts, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace cmlpl;
  int ny, nx;
  if (!sp_grid(rows, cols, G, S, &ny, &nx) || iters < 1 || iters > 100) return CMLPL_E_ARG;
  if (!std::isfinite(m) || !(m > 0.f)) return CMLPL_E_ARG;
  const float w = (float)(((double)m * (double)m) / ((double)S * (double)S));
  if (!std::isfinite(w) || !(w > 0.f)) return CMLPL_E_ARG;
  if (G > 0 && (!d_guide || guide_stride < G)) return CMLPL_E_ARG;
  if (!d_seg || !d_ws) return CMLPL_E_ARG;
  if (!aligned_to(3, d_guide, d_seg, d_centres, d_counts, d_ws)) return CMLPL_E_ARG;
  if (ws_bytes < cmlpl_sp_workspace_bytes(rows, cols, G, S)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  SpArgs a = {};
  a.guide = G > 0 ? d_guide : nullptr; a.guide_stride = (i64)guide_stride;
  a.G = G; a.rows = rows; a.cols = cols; a.S = S; a.ny = ny; a.nx = nx; a.n = rows * cols; a.N = ny * nx;
  a.tiles_x = (cols + SP_TX - 1) / SP_TX; a.w = w;
  a.centres = reinterpret_cast<float*>(d_ws);
  a.plan = a.centres + (size_t)a.N * (2 + G);
  a.flag = reinterpret_cast<unsigned char*>(a.plan + (size_t)G * a.n);
  a.seg = d_seg;
  const unsigned wg_n = (unsigned)((a.n + SP_THREADS - 1) / SP_THREADS), wg_N = (unsigned)((a.N + SP_THREADS - 1) / SP_THREADS);
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((rows + SP_TY - 1) / SP_TY);
  const bool wide = S >= SP_WIDE_S;
  const unsigned wg_u = wide ? (unsigned)a.N : (unsigned)((a.N + SP_THREADS / 64 - 1) / (SP_THREADS / 64));
  hipError_t e;
  hipLaunchKernelGGL(sp_pack_kernel, dim3(wg_n), dim3(SP_THREADS), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sp_init_kernel, dim3(wg_N), dim3(SP_THREADS), 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  for (int t = 1; t <= iters; ++t) {
    hipLaunchKernelGGL(sp_assign_kernel, dim3(tiles), dim3(SP_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    if (t == iters) { a.out_centres = d_centres; a.out_counts = d_counts; }
    if (wide) hipLaunchKernelGGL(sp_update_kernel<4>, dim3(wg_u), dim3(SP_THREADS), 0, st, a);
    else hipLaunchKernelGGL(sp_update_kernel<1>, dim3(wg_u), dim3(SP_THREADS), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  }
  return 0;
}

extern "C" size_t cmlpl_sp_vote_workspace_bytes(int N, int K) {
  if (N < 1 || K < 1 || K > 64 || (int64_t)N * K > INT32_MAX) return 0;
  return cmlpl::vote_ws_bytes(N, K);
}

extern "C" int cmlpl_sp_vote_probs(const int32_t* d_seg, const float* d_probs, int n, int K, int N, float* d_out_probs,
                                   int64_t* d_labels, float* d_conf, float* d_entropy, int64_t* d_sums, int64_t* d_cnt,
                                   float* d_seg_probs, int64_t* d_seg_labels, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_probs) return CMLPL_E_ARG;
  return cmlpl::vote(d_seg, d_probs, nullptr, n, K, N, d_out_probs, d_labels, d_conf, d_entropy, d_sums, d_cnt, d_seg_probs,
                     d_seg_labels, d_ws, ws_bytes, stream);
}

extern "C" int cmlpl_sp_vote_labels(const int32_t* d_seg, const int64_t* d_src_labels, int n, int K, int N, float* d_out_probs,
                                    int64_t* d_labels, float* d_conf, float* d_entropy, int64_t* d_sums, int64_t* d_cnt,
                                    float* d_seg_probs, int64_t* d_seg_labels, void* d_ws, size_t ws_bytes, void* stream) {
  if (!d_src_labels) return CMLPL_E_ARG;
  return cmlpl::vote(d_seg, nullptr, d_src_labels, n, K, N, d_out_probs, d_labels, d_conf, d_entropy, d_sums, d_cnt, d_seg_probs,
                     d_seg_labels, d_ws, ws_bytes, stream);
}
