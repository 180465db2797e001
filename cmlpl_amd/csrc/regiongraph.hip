// Region graph (include/cmlpl.h, "THE DEFINITION OF A REGION DESCRIPTOR", "... OF A REGION ADJACENCY", "... OF A REGION
// GRAPH"): from a region map to what cmlpl_lp_graph takes -- a mean spectrum per region, the regions' 4-connected neighbours
// by shared boundary length, and one neighbour list per region that joins the kNN lists of the embedding with them.
//
// The pool, eight launches whatever the map holds:
//   zero, histogram   the pixels of every region, 32-bit integer atomics; a run of lanes with one region adds once.
//   sums, scan, offsets   the exclusive prefix of the histogram: per block of 1024 regions a sum, one workgroup scans the
//            block sums (as regions.hip scans its root counts), every block rescans its own entries.
//   scatter  the pixel index by region: a run of lanes takes its slots with one atomic add on the region's cursor.  The
//            order inside a region depends on the run; nothing that is summed over it does, because every term is an integer.
//   pool     a wavefront per region of up to 64 pixels, a workgroup of four per larger region (two launches over the same
//            body; a region belongs to exactly one of them, the other returns at once).  Lanes run along the bands, so a
//            pixel's row is one coalesced read and the row is read ONCE: the same registers decide whether the pixel is
//            pooled (one ballot) and feed the int64 sums, ceil(B / 64) <= 16 per lane.  No atomics on the [M, B] table.
// The adjacency, eight launches:
//   zero, count   the directed contacts of every region: a pixel counts its four neighbours of OTHER regions, a run of
//            lanes with one region is summed in the wave, its first lane adds to boundary[s].
//   sums, scan, offsets   region s gets an open-addressing table of the next power of two >= 2 boundary[s] entries (0 for
//            a region without a contact) inside one workspace: less than 4 boundary[s] each, less than 16 n in all.
//   init     keys -1, counts 0, up to the total the scan left on the device.
//   insert   a pixel inserts its contacts into its OWN region's table: atomicCAS on the key word claims or finds the
//            neighbour's slot, atomicAdd on the count word counts.  A table holds at most boundary[s] distinct keys in at
//            least twice as many slots, so a probe always meets the key or a free slot: no thread waits for another one.
//            Which slot a key lands in depends on the order; the SET of (key, count) pairs does not.
//   select   a wavefront per region: deg = the occupied slots, then A rounds of a wave-wide maximum of the 64-bit integer
//            (count << 32) | (0xFFFFFFFF - id) strictly below the previous pick: count descending, id ascending.  A hub (a
//            region that touches more than A others) takes the same path as any other region.
// The lists, one launch: a wavefront per region copies its kNN slots and forms the dot product of its own 4 KiB row (held
// in registers) with the row of every adjacent region that is no kNN neighbour already.
// Integer atomics only, no float atomics, no scratch; nothing allocates, synchronises or reads back.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_BLOCK = 1024;                    // entries per workgroup of the scan launches
constexpr int RG_WAVE_MAX = 64;                   // a region of more pixels is pooled by a workgroup
constexpr int RG_INIT_BLOCKS = 1024;              // the grid of the table init (a stride loop up to the device's total)
constexpr int RG_A_MAX = 16, RG_NBR_MAX = 32, RG_B_MAX = 1024, RG_D = 1024;
constexpr int64_t RG_N_MAX = (int64_t)1 << 27;    // 16 n table entries are indexed with 31 bits

typedef long long i64;
typedef unsigned long long u64;

// a pixel's region: ids[p] in 0 .. M - 1, else -1 (void)
__device__ __forceinline__ int rg_region(const int* ids, i64 p, int M) {
  const int v = ids[p];
  return (unsigned)v < (unsigned)M ? v : -1;
}

// the runs of equal keys among the 64 lanes (regions.hip's flatten): head = first lane of its run, end = its last lane
__device__ __forceinline__ void wave_runs(int key, int lane, bool& head, int& end) {
  const int prev = __shfl_up(key, 1, 64);
  head = lane == 0 || prev != key;
  const u64 hm = __ballot(head);
  const u64 next = lane == 63 ? 0ull : (hm >> (lane + 1));
  end = next ? lane + __ffsll((long long)next) - 1 : 63;
}
__device__ __forceinline__ int run_sum(int v, int lane, int end) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_down(v, o, 64);
    if (lane + o <= end) v += t;
  }
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ u64 wave_max64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64), lo = __shfl_xor((unsigned)v, o, 64);
    const u64 t = ((u64)hi << 32) | lo;
    v = t > v ? t : v;
  }
  return v;
}

__global__ __launch_bounds__(RG_THREADS) void rg_zero_kernel(int* w, int M) {
  const i64 i = (i64)blockIdx.x * RG_THREADS + threadIdx.x;
  if (i < M) w[i] = 0;
}

// ------------------------------------------------------------------ the exclusive prefix of M terms
// mode 0: the entry itself; mode 1: the table entries of a region with v contacts, the next power of two >= 2 v (0: none)
__device__ __forceinline__ int rg_term(int v, int mode) {
  if (mode == 0) return v;
  return v <= 0 ? 0 : 1 << (32 - __clz(2 * v - 1));
}

__global__ __launch_bounds__(RG_THREADS) void rg_sums_kernel(const int* in, int M, int mode, int* partial) {
  __shared__ int wcnt[RG_THREADS / 64];
  const int tid = threadIdx.x;
  int s = 0;
#pragma unroll
  for (int k = 0; k < RG_BLOCK / RG_THREADS; ++k) {
    const i64 i = (i64)blockIdx.x * RG_BLOCK + k * RG_THREADS + tid;
    if (i < M) s += rg_term(in[i], mode);
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) wcnt[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// one workgroup: partial[b] becomes the sum of the blocks before b; partial[blocks] the total
__global__ __launch_bounds__(RG_THREADS) void rg_scan_kernel(int* partial, int blocks) {
  __shared__ int seg[RG_THREADS];
  const int tid = threadIdx.x;
  const int L = (blocks + RG_THREADS - 1) / RG_THREADS;
  const int b0 = min(tid * L, blocks), b1 = min(b0 + L, blocks);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += partial[b];
  seg[tid] = s;
  __syncthreads();
  int before = 0;
  for (int t = 0; t < tid; ++t) before += seg[t];
  for (int b = b0; b < b1; ++b) {
    const int c = partial[b];
    partial[b] = before;
    before += c;
  }
  if (tid == RG_THREADS - 1) partial[blocks] = before;
}

// entry i of a block: the block's prefix, the waves and lanes in front, the thread's own entries in front; off[M] the total
__global__ __launch_bounds__(RG_THREADS) void rg_offsets_kernel(const int* in, int M, int mode, const int* partial, int* off,
                                                                int* cursor) {
  __shared__ int wcnt[RG_THREADS / 64];
  constexpr int PER = RG_BLOCK / RG_THREADS;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const i64 i0 = (i64)blockIdx.x * RG_BLOCK + tid * PER;
  int v[PER], s = 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    v[k] = i0 + k < M ? rg_term(in[i0 + k], mode) : 0;
    s += v[k];
  }
  int inc = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wcnt[wv] = inc;
  __syncthreads();
  int before = partial[blockIdx.x] + inc - s;
#pragma unroll
  for (int w = 0; w < RG_THREADS / 64; ++w) before += w < wv ? wcnt[w] : 0;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (i0 + k >= M) break;
    off[i0 + k] = before;
    if (cursor != nullptr) cursor[i0 + k] = before;
    before += v[k];
    if (i0 + k == M - 1) off[M] = before;
  }
}

// partial [blocks + 2]; in [M] -> off [M + 1] (and cursor [M], a copy of off's first M words)
inline unsigned rg_blocks(size_t M) { return (unsigned)((M + RG_BLOCK - 1) / RG_BLOCK); }

#define RG_LAUNCH(kernel, grid, ...)                                                            \
  do {                                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(RG_THREADS), 0, st, __VA_ARGS__);               \
    const hipError_t e_ = hipGetLastError();                                                    \
    if (e_ != hipSuccess) return (int)e_;                                                       \
  } while (0)

int rg_prefix(const int* in, int M, int mode, int* partial, int* off, int* cursor, hipStream_t st) {
  const unsigned blocks = rg_blocks((size_t)M);
  RG_LAUNCH(rg_sums_kernel, blocks, in, M, mode, partial);
  RG_LAUNCH(rg_scan_kernel, 1u, partial, (int)blocks);
  RG_LAUNCH(rg_offsets_kernel, blocks, in, M, mode, (const int*)partial, off, cursor);
  return 0;
}

// ------------------------------------------------------------------ the pixel index by region
__global__ __launch_bounds__(RG_THREADS) void rg_hist_kernel(const int* ids, int n, int M, int* cnt) {
  const i64 p = (i64)blockIdx.x * RG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int s = p < n ? rg_region(ids, p, M) : -1;
  bool head; int end;
  wave_runs(s, lane, head, end);
  if (head && s >= 0) atomicAdd(cnt + s, end - lane + 1);
}

__global__ __launch_bounds__(RG_THREADS) void rg_scatter_kernel(const int* ids, int n, int M, int* cursor, int* pix) {
  const i64 p = (i64)blockIdx.x * RG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int s = p < n ? rg_region(ids, p, M) : -1;
  bool head; int end;
  wave_runs(s, lane, head, end);
  const u64 hm = __ballot(head);
  const int start = 63 - __clzll((long long)(hm & (~0ull >> (63 - lane))));       // the head of this lane's run
  int base = 0;
  if (head && s >= 0) base = atomicAdd(cursor + s, end - lane + 1);
  base = __shfl(base, start, 64);
  if (s >= 0) pix[base + lane - start] = (int)p;
}

// ------------------------------------------------------------------ the pool
struct PoolArgs {
  const float* X; i64 stride; int B, M;
  const int* off; const int* pix;
  float* mean; i64* cnt; i64* S;
};

// WAVES 1: a wavefront per region of at most RG_WAVE_MAX pixels (four regions per workgroup); WAVES 4: a workgroup per
// larger region.  NJ = the 64-band chunks a lane holds.
template <int NJ, int WAVES>
__global__ __launch_bounds__(RG_THREADS) void rg_pool_kernel(PoolArgs a) {
  __shared__ i64 red[RG_THREADS / 64][64];
  __shared__ int rcnt[RG_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const i64 s64 = WAVES == 1 ? (i64)blockIdx.x * (RG_THREADS / 64) + wv : (i64)blockIdx.x;
  if (s64 >= a.M) return;                                                         // (WAVES 1 only: no barrier below)
  const int s = (int)s64;
  const int i0 = a.off[s], i1 = a.off[s + 1];
  if (WAVES == 1 ? i1 - i0 > RG_WAVE_MAX : i1 - i0 <= RG_WAVE_MAX) return;        // (uniform over the wave / the workgroup)
  i64 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0;
  int cnt = 0;
  for (int i = i0 + (WAVES == 1 ? 0 : wv); i < i1; i += WAVES) {
    const float* row = a.X + (i64)a.pix[i] * a.stride;
    float x[NJ];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int b = lane + 64 * j;
      x[j] = b < a.B ? row[b] : 0.0f;
      bad |= !(fabsf(x[j]) <= 256.0f);                                            // (NaN and +-inf fail the comparison)
    }
    if (__ballot(bad) != 0ull) continue;
    ++cnt;
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] += llrintf(x[j] * 16777216.0f);           // (the product is exact)
  }
  if (WAVES > 1) {
    if (lane == 0) rcnt[wv] = cnt;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      __syncthreads();                                                            // (red is free again; rcnt is written)
      red[wv][lane] = acc[j];
      __syncthreads();
      if (wv == 0) acc[j] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
    }
    if (wv != 0) return;
    cnt = rcnt[0] + rcnt[1] + rcnt[2] + rcnt[3];
  }
  if (lane == 0) a.cnt[s] = cnt;
  const double den = (double)cnt * 16777216.0;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int b = lane + 64 * j;
    if (b >= a.B) continue;
    const i64 o = (i64)s * a.B + b;
    if (a.S != nullptr) a.S[o] = acc[j];
    a.mean[o] = cnt > 0 ? (float)((double)acc[j] / den) : 0.0f;
  }
}

template <int NJ>
int rg_pool_launch(const PoolArgs& a, hipStream_t st) {
  void (*const by_wave)(PoolArgs) = rg_pool_kernel<NJ, 1>;
  void (*const by_workgroup)(PoolArgs) = rg_pool_kernel<NJ, 4>;
  RG_LAUNCH(by_wave, (unsigned)(((i64)a.M + 3) / 4), a);
  RG_LAUNCH(by_workgroup, (unsigned)a.M, a);
  return 0;
}

// ------------------------------------------------------------------ the adjacency
struct AdjArgs {
  const int* ids; int rows, cols, n, M, A;
  int* boundary; const int* tab_off; int* keys; int* cnts;
  int* adj_idx; int* adj_len; int* deg;
};

// the regions of p's four neighbours that are regions other than s (-1: none there)
__device__ __forceinline__ void rg_contacts(const AdjArgs& a, int p, int s, int t[4]) {
  const int y = p / a.cols, x = p - y * a.cols;
  t[0] = x > 0 ? rg_region(a.ids, p - 1, a.M) : -1;
  t[1] = x < a.cols - 1 ? rg_region(a.ids, p + 1, a.M) : -1;
  t[2] = y > 0 ? rg_region(a.ids, p - a.cols, a.M) : -1;
  t[3] = y < a.rows - 1 ? rg_region(a.ids, (i64)p + a.cols, a.M) : -1;
#pragma unroll
  for (int d = 0; d < 4; ++d) t[d] = t[d] == s ? -1 : t[d];
}

__global__ __launch_bounds__(RG_THREADS) void rg_count_kernel(AdjArgs a) {
  const i64 p = (i64)blockIdx.x * RG_THREADS + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const int s = p < a.n ? rg_region(a.ids, p, a.M) : -1;
  int c = 0;
  if (s >= 0) {
    int t[4];
    rg_contacts(a, (int)p, s, t);
    c = (t[0] >= 0) + (t[1] >= 0) + (t[2] >= 0) + (t[3] >= 0);
  }
  bool head; int end;
  wave_runs(s, lane, head, end);
  c = run_sum(c, lane, end);
  if (head && s >= 0 && c > 0) atomicAdd(a.boundary + s, c);
}

__global__ __launch_bounds__(RG_THREADS) void rg_table_init_kernel(AdjArgs a) {
  const i64 total = a.tab_off[a.M];
  for (i64 i = (i64)blockIdx.x * RG_THREADS + threadIdx.x; i < total; i += (i64)gridDim.x * RG_THREADS) {
    a.keys[i] = -1;
    a.cnts[i] = 0;
  }
}

// (a probe ends: the table has at least twice the slots of the keys it can ever hold, see the header)
__global__ __launch_bounds__(RG_THREADS) void rg_insert_kernel(AdjArgs a) {
  const i64 p = (i64)blockIdx.x * RG_THREADS + threadIdx.x;
  if (p >= a.n) return;
  const int s = rg_region(a.ids, p, a.M);
  if (s < 0) return;
  int t[4];
  rg_contacts(a, (int)p, s, t);
  if (t[0] < 0 && t[1] < 0 && t[2] < 0 && t[3] < 0) return;
  const int base = a.tab_off[s], size = a.tab_off[s + 1] - base;
  if (size < 2) return;                                                           // (cannot be: the pixel has a contact)
  const unsigned mask = (unsigned)size - 1u;
  const int shift = __clz(size) + 1;                                              // 32 - log2(size)
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    if (t[d] < 0) continue;
    unsigned h = ((unsigned)t[d] * 2654435761u) >> shift;
    for (unsigned tries = 0; tries <= mask; ++tries) {
      const int old = atomicCAS(a.keys + base + h, -1, t[d]);
      if (old == -1 || old == t[d]) {
        atomicAdd(a.cnts + base + h, 1);
        break;
      }
      h = (h + 1u) & mask;
    }
  }
}

__global__ __launch_bounds__(RG_THREADS) void rg_select_kernel(AdjArgs a) {
  const int lane = threadIdx.x & 63;
  const i64 s64 = (i64)blockIdx.x * (RG_THREADS / 64) + (threadIdx.x >> 6);
  if (s64 >= a.M) return;
  const int s = (int)s64;
  const int base = a.tab_off[s], size = a.tab_off[s + 1] - base;
  int d = 0;
  for (int i = lane; i < size; i += 64) d += a.keys[base + i] >= 0;
  d = wave_sum(d);
  if (lane == 0) a.deg[s] = d;
  u64 prev = ~0ull;
  for (int r = 0; r < a.A; ++r) {
    u64 best = 0ull;
    for (int i = lane; i < size; i += 64) {
      const int k = a.keys[base + i];
      if (k < 0) continue;
      const u64 key = ((u64)(unsigned)a.cnts[base + i] << 32) | (u64)(0xFFFFFFFFu - (unsigned)k);
      if (key < prev && key > best) best = key;
    }
    best = wave_max64(best);                        // (0: nothing below the previous pick; it stays 0 from there on)
    if (lane == 0) {
      a.adj_idx[(i64)s * a.A + r] = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) : -1;
      a.adj_len[(i64)s * a.A + r] = (int)(best >> 32);
    }
    prev = best;
  }
}

// ------------------------------------------------------------------ the lists
struct ListArgs {
  const float* feat; int M, k, A;
  const int* knn_idx; const float* knn_sim; const int* adj_idx;
  int* nbr_idx; float* nbr_sim;
};

__global__ __launch_bounds__(RG_THREADS) void rg_lists_kernel(ListArgs a) {
  const int lane = threadIdx.x & 63;
  const i64 s = (i64)blockIdx.x * (RG_THREADS / 64) + (threadIdx.x >> 6);
  if (s >= a.M) return;
  const int W = a.k + a.A;
  int mine = -1;
  if (lane < a.k) {
    mine = a.knn_idx[s * a.k + lane];
    a.nbr_idx[s * W + lane] = mine;
    a.nbr_sim[s * W + lane] = a.knn_sim[s * a.k + lane];
  }
  if (a.A == 0) return;
  const float4* own_row = reinterpret_cast<const float4*>(a.feat + s * RG_D);
  float4 own[RG_D / 256];
#pragma unroll
  for (int j = 0; j < RG_D / 256; ++j) own[j] = own_row[lane + 64 * j];
  for (int r = 0; r < a.A; ++r) {
    const int t = a.adj_idx[s * a.A + r];                                         // (one word for the whole wave)
    const bool in_knn = __ballot(lane < a.k && mine == t) != 0ull;
    int out = -1;
    float sim = -__builtin_inff();
    if (t >= 0 && t < a.M && !in_knn) {
      const float4* row = reinterpret_cast<const float4*>(a.feat + (i64)t * RG_D);
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < RG_D / 256; ++j) {
        const float4 v = row[lane + 64 * j];
        acc = fmaf(own[j].x, v.x, acc); acc = fmaf(own[j].y, v.y, acc);
        acc = fmaf(own[j].z, v.z, acc); acc = fmaf(own[j].w, v.w, acc);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
      out = t;
      sim = acc;
    }
    if (lane == 0) {
      a.nbr_idx[s * W + a.k + r] = out;
      a.nbr_sim[s * W + a.k + r] = sim;
    }
  }
}

// ------------------------------------------------------------------ the workspace
bool rg_map(int rows, int cols, int M) {
  return rows >= 1 && cols >= 1 && (int64_t)rows * cols <= RG_N_MAX && M >= 1 && (int64_t)M <= RG_N_MAX;
}

// [count / scratch words 4 M][offsets 4 (M + 1)][cursors 4 M][block prefixes 4 (blocks + 2)][pixel index 4 n]
// [table keys 4 x 16 n][table counts 4 x 16 n], behind a 16-byte boundary found inside it
size_t rg_ws_bytes(size_t n, size_t M) { return 16 + 4 * (3 * M + 1 + rg_blocks(M) + 2 + n + 32 * n); }

struct RgWs { int* cnt; int* off; int* cursor; int* partial; int* pix; int* keys; int* cnts; };
RgWs rg_carve(void* d_ws, size_t n, size_t M) {
  RgWs w;
  w.cnt = reinterpret_cast<int*>((reinterpret_cast<uintptr_t>(d_ws) + 15) & ~uintptr_t(15));
  w.off = w.cnt + M;
  w.cursor = w.off + M + 1;
  w.partial = w.cursor + M;
  w.pix = w.partial + rg_blocks(M) + 2;
  w.keys = w.pix + n;
  w.cnts = w.keys + 16 * n;
  return w;
}

}  // namespace
}  // namespace cmlpl

extern "C" size_t cmlpl_rg_workspace_bytes(int rows, int cols, int M, int A) {
  if (!cmlpl::rg_map(rows, cols, M) || A < 0 || A > cmlpl::RG_A_MAX) return 0;
  return cmlpl::rg_ws_bytes((size_t)rows * cols, (size_t)M);
}

extern "C" int cmlpl_rg_pool(const int32_t* d_ids, int rows, int cols, int M, const float* d_X, int64_t x_stride, int B,
                             float* d_mean, int64_t* d_cnt, int64_t* d_S, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace cmlpl;
  if (!rg_map(rows, cols, M) || B < 1 || B > RG_B_MAX || x_stride < B) return CMLPL_E_ARG;
  if (!d_ids || !d_X || !d_mean || !d_cnt || !d_ws) return CMLPL_E_ARG;
  if (!aligned_to(3, d_ids) || !aligned_to(3, d_X, d_mean) || !aligned_to(7, d_cnt, d_S) || !aligned_to(3, d_ws)) return CMLPL_E_ARG;
  if (ws_bytes < cmlpl_rg_workspace_bytes(rows, cols, M, 0)) return CMLPL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)rows * cols;
  const RgWs w = rg_carve(d_ws, n, (size_t)M);
  const unsigned wg_n = (unsigned)((n + RG_THREADS - 1) / RG_THREADS), wg_M = (unsigned)(((size_t)M + RG_THREADS - 1) / RG_THREADS);
  RG_LAUNCH(rg_zero_kernel, wg_M, w.cnt, M);
  RG_LAUNCH(rg_hist_kernel, wg_n, d_ids, (int)n, M, w.cnt);
  int rc = rg_prefix(w.cnt, M, 0, w.partial, w.off, w.cursor, st);
  if (rc != 0) return rc;
  RG_LAUNCH(rg_scatter_kernel, wg_n, d_ids, (int)n, M, w.cursor, w.pix);
  PoolArgs a = {};
  a.X = d_X; a.stride = x_stride; a.B = B; a.M = M; a.off = w.off; a.pix = w.pix;
  a.mean = d_mean; a.cnt = reinterpret_cast<i64*>(d_cnt); a.S = reinterpret_cast<i64*>(d_S);
  const int chunks = (B + 63) / 64;
  if (chunks <= 1) return rg_pool_launch<1>(a, st);
  if (chunks <= 2) return rg_pool_launch<2>(a, st);
  if (chunks <= 4) return rg_pool_launch<4>(a, st);
  if (chunks <= 8) return rg_pool_launch<8>(a, st);
  return rg_pool_launch<16>(a, st);
}

extern "C" int cmlpl_rg_adjacency(const int32_t* d_ids, int rows, int cols, int M, int A, int32_t* d_adj_idx,
                                  int32_t* d_adj_len, int32_t* d_deg, int32_t* d_boundary, void* d_ws, size_t ws_bytes,
                                  void* stream) {
  using namespace cmlpl;
  if (!rg_map(rows, cols, M) || A < 0 || A > RG_A_MAX) return CMLPL_E_ARG;
  if (!d_ids || !d_deg || !d_boundary || !d_ws || (A > 0 && (!d_adj_idx || !d_adj_len))) return CMLPL_E_ARG;
  if (!aligned_to(3, d_ids, d_adj_idx, d_adj_len, d_deg, d_boundary) || !aligned_to(3, d_ws)) return CMLPL_E_ARG;
  if (ws_bytes < cmlpl_rg_workspace_bytes(rows, cols, M, A)) return CMLPL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)rows * cols;
  const RgWs w = rg_carve(d_ws, n, (size_t)M);
  const unsigned wg_n = (unsigned)((n + RG_THREADS - 1) / RG_THREADS), wg_M = (unsigned)(((size_t)M + RG_THREADS - 1) / RG_THREADS);
  AdjArgs a = {};
  a.ids = d_ids; a.rows = rows; a.cols = cols; a.n = (int)n; a.M = M; a.A = A;
  a.boundary = d_boundary; a.tab_off = w.off; a.keys = w.keys; a.cnts = w.cnts;
  a.adj_idx = d_adj_idx; a.adj_len = d_adj_len; a.deg = d_deg;
  RG_LAUNCH(rg_zero_kernel, wg_M, d_boundary, M);
  RG_LAUNCH(rg_count_kernel, wg_n, a);
  int rc = rg_prefix(d_boundary, M, 1, w.partial, w.off, nullptr, st);
  if (rc != 0) return rc;
  RG_LAUNCH(rg_table_init_kernel, (unsigned)RG_INIT_BLOCKS, a);
  RG_LAUNCH(rg_insert_kernel, wg_n, a);
  RG_LAUNCH(rg_select_kernel, (unsigned)(((size_t)M + 3) / 4), a);
  return 0;
}

extern "C" int cmlpl_rg_lists(const float* d_feat, int M, const int32_t* d_knn_idx, const float* d_knn_sim, int k,
                              const int32_t* d_adj_idx, int A, int32_t* d_nbr_idx, float* d_nbr_sim, void* stream) {
  using namespace cmlpl;
  if (M < 1 || (int64_t)M > RG_N_MAX || k < 0 || A < 0 || A > RG_A_MAX || k + A < 1 || k + A > RG_NBR_MAX) return CMLPL_E_ARG;
  if (!d_feat || !d_nbr_idx || !d_nbr_sim || (k > 0 && (!d_knn_idx || !d_knn_sim)) || (A > 0 && !d_adj_idx)) return CMLPL_E_ARG;
  if (!aligned_to(15, d_feat) || !aligned_to(3, d_knn_idx, d_adj_idx, d_nbr_idx) || !aligned_to(3, d_knn_sim, d_nbr_sim)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  ListArgs a = {};
  a.feat = d_feat; a.M = M; a.k = k; a.A = A; a.knn_idx = d_knn_idx; a.knn_sim = d_knn_sim; a.adj_idx = d_adj_idx;
  a.nbr_idx = d_nbr_idx; a.nbr_sim = d_nbr_sim;
  RG_LAUNCH(rg_lists_kernel, (unsigned)(((size_t)M + 3) / 4), a);
  return 0;
}
