// Connected regions (include/cmlpl.h, "THE DEFINITION OF A COMPONENT MAP" and "THE DEFINITION OF A SIEVED MAP"): the
// components of an int32 map with their sizes and a compact numbering, and the sieve that hands every small component to
// the largest large component it touches.
//
// The labelling is union-find in three launches, whatever the map holds:
//   tile     a workgroup of 256 threads per tile of 32 x 32 pixels, four pixels per thread, lanes along x.  The tile's
//            values and a parent word per pixel live in LDS: 8 KiB per workgroup.  That is a twentieth of the 160 KiB of a
//            CU, so the LDS never limits the resident waves, while a 32 x 32 tile leaves 1 pixel in 8 on a border that the
//            next launch has to unite in global memory (a 32 x 8 tile: 1 in 3).  A larger tile would shorten the global
//            chains further, but 64 x 64 at 16 pixels per thread keeps the whole tile waiting for its longest local chain.
//            Every pixel ends at its tile's root, written as a scene index; the size and target words are zeroed here.
//   border   one thread per pixel; the ones on a tile's first row / column (conn 8: its last column too) unite with their
//            neighbours in the tile before, on the parent words in global memory.
//   flatten  every pixel walks to its root and stores it; a run of lanes with one root is summed inside the wave and its
//            first lane adds the run to the root's size (32-bit integer atomic).  The block's roots are counted for the ids.
// The ids: flatten's per-block root counts, one workgroup scans them (and writes M), a rank launch numbers the roots and a
// broadcast launch hands rank and size to every pixel.
//
// THE UNION IS LOCK-FREE.  A parent word only ever takes a SMALLER index: parent[i] <= i holds from the first store on,
// and the only writes are atomicMin(parent + a, b) with b < a.  find() follows parents, so the index strictly decreases
// along every path and the walk ends at a word that names itself: at most i steps, whatever the other threads do.
// unite(a, b) links the larger of two (believed) roots under the smaller with one atomicMin and reads what the word held:
// if that was the index itself the link is made; otherwise the word already had a smaller parent `old`, and the pair to
// unite becomes (old, b).  Every retry replaces the larger index of the pair by a strictly smaller one, so a + b strictly
// decreases: the loop ends.  A thread only retries on the value its own atomic returned; it never waits for another
// thread to publish anything, so lanes in lockstep cannot hold each other up.  A stale read in find() is harmless: an old
// parent is still an ancestor in the same component, and the atomicMin that follows returns the truth.  Since a link
// always points to the smaller index, the root of a finished component is its smallest pixel index.
//
// The sieve runs T times: tile, border, flatten (sizes at the roots), candidates (a small component's pixels offer their
// large neighbours: a 64-bit integer atomicMax of (size << 32) | (0xFFFFFFFF - root) per small root), apply (relabel,
// and the pass's four counters summed per wave, one 32-bit atomicAdd each).  A target is a LARGE component and only small
// ones move, so the word apply reads at the target's root is never one that the pass writes: the pass may run in place.
// Integer atomics only, no float atomics, no scratch; every output is the same bytes on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_T = 32;                          // the tile: CC_T x CC_T pixels
constexpr int CC_PPT = CC_T * CC_T / CC_THREADS;  // pixels per thread (4)
constexpr int CC_BLOCK = 1024;                    // pixels per workgroup of the 1-D launches that count (flatten, rank)
constexpr int CC_MAX_PASSES = 16;

typedef long long i64;
typedef unsigned long long u64;

struct CcArgs {
  const int* map;                                 // [n]
  int rows, cols, n, conn, tiles_x;
  int* comp;                                      // [n]: the parent words, then the roots
  int* size;                                      // [n]: at the roots after flatten; everywhere after broadcast
  u64* best;                                      // [n] or null: the sieve's target word per root
  int* partial;                                   // [blocks + 1] or null: roots per block of CC_BLOCK pixels, then their prefix
  int* id;                                        // [n] or null
  int* M;                                         // [1]
  int want_size;                                  // broadcast: size to every pixel
  // the sieve
  int min_size;
  int* out;                                       // [n]
  int* stats;                                     // [4] of this pass
  const float* probs; int K; float* conf;
};

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_lds(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// (the index strictly decreases: see the header)
__device__ __forceinline__ int find(const int* parent, int x) {
  for (int p; (p = ld(parent + x)) != x;) x = p;
  return x;
}
__device__ __forceinline__ int find_lds(const int* parent, int x) {
  for (int p; (p = ld_lds(parent + x)) != x;) x = p;
  return x;
}
// (a + b strictly decreases: see the header)
__device__ __forceinline__ void unite(int* parent, int a, int b) {
  a = find(parent, a); b = find(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    a = old;
  }
}
__device__ __forceinline__ void unite_lds(int* parent, int a, int b) {
  a = find_lds(parent, a); b = find_lds(parent, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);
    if (old == a) break;
    a = old;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(CcArgs a) {
  __shared__ int val[CC_T * CC_T];
  __shared__ int par[CC_T * CC_T];
  const int tid = threadIdx.x, lx = tid & (CC_T - 1), ly0 = tid >> 5;
  const int tile_y = (int)blockIdx.x / a.tiles_x, tile_x = (int)blockIdx.x - tile_y * a.tiles_x;
  const int x0 = tile_x * CC_T, y0 = tile_y * CC_T;
  const int gx = x0 + lx;
  if (blockIdx.x == 0 && tid < 4 && a.stats != nullptr) a.stats[tid] = 0;       // (the pass's counters: apply adds later)
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int ly = ly0 + k * (CC_THREADS / CC_T), l = ly * CC_T + lx, gy = y0 + ly;
    val[l] = (gx < a.cols && gy < a.rows) ? a.map[gy * a.cols + gx] : -1;
    par[l] = l;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int ly = ly0 + k * (CC_THREADS / CC_T), l = ly * CC_T + lx;
    const int v = val[l];
    if (v < 0) continue;
    if (lx > 0 && val[l - 1] == v) unite_lds(par, l, l - 1);
    if (ly > 0 && val[l - CC_T] == v) unite_lds(par, l, l - CC_T);
    if (a.conn == 8 && ly > 0) {
      if (lx > 0 && val[l - CC_T - 1] == v) unite_lds(par, l, l - CC_T - 1);
      if (lx < CC_T - 1 && val[l - CC_T + 1] == v) unite_lds(par, l, l - CC_T + 1);
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const int ly = ly0 + k * (CC_THREADS / CC_T), l = ly * CC_T + lx, gy = y0 + ly;
    if (gx >= a.cols || gy >= a.rows) continue;
    const int g = gy * a.cols + gx;
    int root = -1;
    if (val[l] >= 0) {
      const int r = find_lds(par, l);             // (local and scene indices order a tile's pixels alike)
      root = (y0 + (r >> 5)) * a.cols + x0 + (r & (CC_T - 1));
    }
    a.comp[g] = root;
    a.size[g] = 0;
    if (a.best != nullptr) a.best[g] = 0ull;
  }
}

__global__ __launch_bounds__(CC_THREADS) void cc_border_kernel(CcArgs a) {
  const i64 i64i = (i64)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i64i >= a.n) return;
  const int i = (int)i64i;
  const int y = i / a.cols, x = i - y * a.cols;
  const int lx = x & (CC_T - 1), ly = y & (CC_T - 1);
  const bool c8 = a.conn == 8;
  if (lx != 0 && ly != 0 && !(c8 && lx == CC_T - 1)) return;
  const int v = a.map[i];
  if (v < 0) return;
  if (lx == 0 && x > 0 && a.map[i - 1] == v) unite(a.comp, i, i - 1);
  if (ly == 0 && y > 0 && a.map[i - a.cols] == v) unite(a.comp, i, i - a.cols);
  if (c8 && y > 0) {
    if ((lx == 0 || ly == 0) && x > 0 && a.map[i - a.cols - 1] == v) unite(a.comp, i, i - a.cols - 1);
    if ((lx == CC_T - 1 || ly == 0) && x < a.cols - 1 && a.map[i - a.cols + 1] == v) unite(a.comp, i, i - a.cols + 1);
  }
}

// the runs of equal keys among the 64 lanes (superpixel.hip's vote): head = first lane of its run, end = its last lane
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

// a block of CC_BLOCK pixels, pixel k * 256 + tid of it per trip: every trip is taken by whole waves
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(CcArgs a) {
  __shared__ int wcnt[CC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63;
  int roots = 0;
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const i64 i = (i64)blockIdx.x * CC_BLOCK + k * CC_THREADS + tid;
    int r = -1;
    if (i < a.n) {
      r = ld(a.comp + i);
      if (r >= 0) {
        r = find(a.comp, r);
        __hip_atomic_store(a.comp + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);    // (an ancestor, at any moment)
        roots += r == (int)i;
      }
    }
    bool head; int end;
    wave_runs(r, lane, head, end);
    const int cnt = run_sum(r >= 0 ? 1 : 0, lane, end);
    if (head && r >= 0) atomicAdd(a.size + r, cnt);
  }
  if (a.partial == nullptr) return;               // (uniform)
  roots = wave_sum(roots);
  if (lane == 0) wcnt[tid >> 6] = roots;
  __syncthreads();
  if (tid == 0) a.partial[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
}

// one workgroup: partial[b] becomes the number of roots in the blocks before b; *M the number of roots
__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(CcArgs a, int blocks) {
  __shared__ int seg[CC_THREADS];
  const int tid = threadIdx.x;
  const int L = (blocks + CC_THREADS - 1) / CC_THREADS;
  const int b0 = min(tid * L, blocks), b1 = min(b0 + L, blocks);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += a.partial[b];
  seg[tid] = s;
  __syncthreads();
  int before = 0;
  for (int t = 0; t < tid; ++t) before += seg[t];
  for (int b = b0; b < b1; ++b) {
    const int c = a.partial[b];
    a.partial[b] = before;
    before += c;
  }
  if (tid == CC_THREADS - 1) *a.M = before;
}

// a root's id = the roots in front of it: the block's prefix, the trips and waves in front, the lanes in front
__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(CcArgs a) {
  __shared__ int wcnt[CC_PPT][CC_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  bool root[CC_PPT];
  int within[CC_PPT];
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
    const i64 i = (i64)blockIdx.x * CC_BLOCK + k * CC_THREADS + tid;
    root[k] = i < a.n && a.comp[i] == (int)i;
    const u64 m = __ballot(root[k]);
    within[k] = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[k][wv] = __popcll(m);
  }
  __syncthreads();
  int before = a.partial[blockIdx.x];
#pragma unroll
  for (int k = 0; k < CC_PPT; ++k) {
#pragma unroll
    for (int w = 0; w < CC_THREADS / 64; ++w) {
      if (root[k] && w == wv) a.id[(i64)blockIdx.x * CC_BLOCK + k * CC_THREADS + tid] = before + within[k];
      before += wcnt[k][w];
    }
  }
}

// every pixel takes its root's id and size (a root's own words are read, never written here); void: -1 and 0
__global__ __launch_bounds__(CC_THREADS) void cc_broadcast_kernel(CcArgs a) {
  const i64 i = (i64)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const int r = a.comp[i];
  if (r == (int)i) return;
  if (a.id != nullptr) a.id[i] = r < 0 ? -1 : a.id[r];
  if (a.want_size) a.size[i] = r < 0 ? 0 : a.size[r];
}

// ------------------------------------------------------------------ the sieve
__global__ __launch_bounds__(CC_THREADS) void sv_candidates_kernel(CcArgs a) {
  const i64 i64i = (i64)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i64i >= a.n) return;
  const int i = (int)i64i;
  const int r = a.comp[i];
  if (r < 0 || a.size[r] >= a.min_size) return;
  const int y = i / a.cols, x = i - y * a.cols;
  u64 key = 0ull;
  for (int dy = -1; dy <= 1; ++dy) {
    for (int dx = -1; dx <= 1; ++dx) {
      if ((dy == 0 && dx == 0) || (a.conn == 4 && dy != 0 && dx != 0)) continue;
      const int yy = y + dy, xx = x + dx;
      if (yy < 0 || yy >= a.rows || xx < 0 || xx >= a.cols) continue;
      const int rj = a.comp[yy * a.cols + xx];
      if (rj < 0 || rj == r) continue;
      const int sj = a.size[rj];
      if (sj < a.min_size) continue;
      const u64 kj = ((u64)(unsigned)sj << 32) | (u64)(0xFFFFFFFFu - (unsigned)rj);
      key = kj > key ? kj : key;
    }
  }
  if (key != 0ull) atomicMax(a.best + r, key);
}

__global__ __launch_bounds__(CC_THREADS) void sv_apply_kernel(CcArgs a) {
  const i64 i = (i64)blockIdx.x * CC_THREADS + threadIdx.x;
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  if (i < a.n) {
    const int r = a.comp[i];
    int v = a.map[i];
    if (r >= 0) {
      const int sz = a.size[r];
      const bool small = sz < a.min_size;
      const u64 key = small ? a.best[r] : 0ull;
      if (key != 0ull) v = a.map[0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull)];     // (a large root's word: no pass writes it)
      if (r == (int)i) { c0 = 1; c1 = small; c2 = key != 0ull; c3 = key != 0ull ? sz : 0; }
    }
    a.out[i] = v;
  }
  c0 = wave_sum(c0); c1 = wave_sum(c1); c2 = wave_sum(c2); c3 = wave_sum(c3);
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(a.stats + 0, c0);
    if (c1) atomicAdd(a.stats + 1, c1);
    if (c2) atomicAdd(a.stats + 2, c2);
    if (c3) atomicAdd(a.stats + 3, c3);
  }
}

__global__ __launch_bounds__(CC_THREADS) void sv_conf_kernel(CcArgs a) {
  const i64 i = (i64)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= a.n) return;
  const int l = a.out[i];
  a.conf[i] = (l >= 0 && l < a.K) ? a.probs[i * a.K + l] : __builtin_nanf("");
}

// rows x cols inside the definition
bool cc_scene(int rows, int cols) { return rows >= 1 && cols >= 1 && (int64_t)rows * cols <= INT32_MAX; }
inline size_t cc_blocks(size_t n) { return (n + CC_BLOCK - 1) / CC_BLOCK; }

// the workspace: [target words 8 n][parents 4 n][sizes 4 n][block prefixes 4 (blocks + 2)][counters 4 x 68], behind an
// 8-byte boundary found inside it
size_t cc_ws_bytes(size_t n) { return 8 + 16 * n + 4 * (cc_blocks(n) + 2) + 4 * 68; }

struct CcWs { u64* best; int* comp; int* size; int* partial; int* words; };
CcWs cc_carve(void* d_ws, size_t n) {
  CcWs w;
  w.best = reinterpret_cast<u64*>((reinterpret_cast<uintptr_t>(d_ws) + 7) & ~uintptr_t(7));
  w.comp = reinterpret_cast<int*>(w.best + n);
  w.size = w.comp + n;
  w.partial = w.size + n;
  w.words = w.partial + cc_blocks(n) + 2;
  return w;
}

#define CC_LAUNCH(kernel, grid, ...)                                                            \
  do {                                                                                          \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(CC_THREADS), 0, st, __VA_ARGS__);               \
    const hipError_t e_ = hipGetLastError();                                                    \
    if (e_ != hipSuccess) return (int)e_;                                                       \
  } while (0)

// tile, border, flatten: a.comp the roots, a.size the sizes at the roots
int label_core(const CcArgs& a, hipStream_t st) {
  const unsigned tiles = (unsigned)a.tiles_x * (unsigned)((a.rows + CC_T - 1) / CC_T);
  const unsigned wg_n = (unsigned)(((i64)a.n + CC_THREADS - 1) / CC_THREADS);
  CC_LAUNCH(cc_tile_kernel, tiles, a);
  CC_LAUNCH(cc_border_kernel, wg_n, a);
  CC_LAUNCH(cc_flatten_kernel, (unsigned)cc_blocks((size_t)a.n), a);
  return 0;
}

}  // namespace
}  // namespace cmlpl

extern "C" size_t cmlpl_cc_workspace_bytes(int rows, int cols) {
  if (!cmlpl::cc_scene(rows, cols)) return 0;
  return cmlpl::cc_ws_bytes((size_t)rows * cols);
}

extern "C" int cmlpl_cc_label(const int32_t* d_map, int rows, int cols, int conn, int32_t* d_comp, int32_t* d_size,
                              int32_t* d_id, int32_t* d_M, void* d_ws, size_t ws_bytes, void* stream) {
  using namespace cmlpl;
  if (!cc_scene(rows, cols) || (conn != 4 && conn != 8)) return CMLPL_E_ARG;
  if (!d_map || !d_comp || !d_ws) return CMLPL_E_ARG;
  if (!aligned_to(3, d_map, d_comp, d_size, d_id, d_M) || !aligned_to(3, d_ws)) return CMLPL_E_ARG;
  if (ws_bytes < cmlpl_cc_workspace_bytes(rows, cols)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)rows * cols;
  const CcWs w = cc_carve(d_ws, n);
  CcArgs a = {};
  a.map = d_map; a.rows = rows; a.cols = cols; a.n = (int)n; a.conn = conn; a.tiles_x = (cols + CC_T - 1) / CC_T;
  a.comp = d_comp; a.size = d_size ? d_size : w.size;
  const bool ids = d_id != nullptr || d_M != nullptr;
  a.partial = ids ? w.partial : nullptr;
  a.id = d_id; a.M = d_M ? d_M : w.words; a.want_size = d_size != nullptr;
  int rc = label_core(a, st);
  if (rc != 0) return rc;
  const unsigned blocks = (unsigned)cc_blocks(n);
  if (ids) CC_LAUNCH(cc_scan_kernel, 1u, a, (int)blocks);
  if (d_id) CC_LAUNCH(cc_rank_kernel, blocks, a);
  if (d_id || d_size) CC_LAUNCH(cc_broadcast_kernel, (unsigned)((n + CC_THREADS - 1) / CC_THREADS), a);
  return 0;
}

extern "C" int cmlpl_cc_sieve(const int32_t* d_map, int rows, int cols, int conn, int min_size, int passes, int32_t* d_out,
                              int32_t* d_stats, const float* d_probs, int K, float* d_conf, void* d_ws, size_t ws_bytes,
                              void* stream) {
  using namespace cmlpl;
  if (!cc_scene(rows, cols) || (conn != 4 && conn != 8)) return CMLPL_E_ARG;
  if (min_size < 1 || passes < 1 || passes > CC_MAX_PASSES) return CMLPL_E_ARG;
  if (!d_map || !d_out || !d_ws) return CMLPL_E_ARG;
  if ((d_probs == nullptr) != (d_conf == nullptr) || (d_probs && K < 1)) return CMLPL_E_ARG;
  if (!aligned_to(3, d_map, d_out, d_stats) || !aligned_to(3, d_probs, d_conf) || !aligned_to(3, d_ws)) return CMLPL_E_ARG;
  if (ws_bytes < cmlpl_cc_workspace_bytes(rows, cols)) return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t n = (size_t)rows * cols;
  const CcWs w = cc_carve(d_ws, n);
  const unsigned wg_n = (unsigned)((n + CC_THREADS - 1) / CC_THREADS);
  CcArgs a = {};
  a.rows = rows; a.cols = cols; a.n = (int)n; a.conn = conn; a.tiles_x = (cols + CC_T - 1) / CC_T;
  a.comp = w.comp; a.size = w.size; a.best = w.best;
  a.min_size = min_size; a.out = d_out;
  a.probs = d_probs; a.K = K; a.conf = d_conf;
  for (int t = 0; t < passes; ++t) {
    a.map = t == 0 ? d_map : d_out;               // (u_(t-1); from the second pass on the pass runs in place)
    a.stats = (d_stats ? d_stats : w.words + 4) + 4 * t;
    int rc = label_core(a, st);
    if (rc != 0) return rc;
    CC_LAUNCH(sv_candidates_kernel, wg_n, a);
    CC_LAUNCH(sv_apply_kernel, wg_n, a);
  }
  if (d_conf) CC_LAUNCH(sv_conf_kernel, wg_n, a);
  return 0;
}
