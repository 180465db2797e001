// Weighted kNN vote over the spectral embedding (include/cmlpl.h, "THE DEFINITION OF A kNN VOTE"; Wu et al., "Unsupervised
// Feature Learning via Non-Parametric Instance Discrimination", CVPR 2018, section 3.4).  Similarity product, candidate
// masks and top-k selection in ONE streaming pass: the [n][m] similarity matrix never exists.
//
//   knn_split_kernel : every row (query and gallery), ONCE, as two fp16 pieces at the fixed scale 2^12 -- x 2^12 = hi + lo,
//                      hi = fp16(x 2^12), lo = fp16(x 2^12 - hi) -- written as the fragments v_mfma_f32_32x32x16_f16
//                      reads: per 32-row tile and 16-wide k-step one 1-KiB plane per piece, lane l = (row l & 31, elements
//                      8 (l >> 5) .. + 7) at byte 16 l.  A fragment load is one coalesced 1-KiB read; rows past the end
//                      of a list are planes of zeros.
//   knn_scan_kernel  : a workgroup of four waves takes 128 queries and walks its share of the gallery 128 rows at a time;
//                      each wave a 64 x 64 tile (2 x 2 accumulators), 64 k-steps, per k-step and accumulator the three
//                      products lo.hi, hi.lo, hi.hi in that order, fp32 accumulate, 2^-24 folded in at the end.  The order
//                      is the same for every tile, so the bits of s_ij depend on the two rows alone.  The QUERIES are the
//                      MFMA's B operand: an accumulator's column, i.e. the lane, is a query, its 16 values are 16 gallery
//                      rows of that query.  Selection is one compare per value against the lane's own k-th best (a
//                      register); the lists live in LDS as [rank][slot], slot = thread, conflict-free.  A lane sees its
//                      gallery rows in ascending order, so a value that EQUALS the threshold never displaces it: the
//                      compare is `>`.  An insertion replaces the list's worst entry and rescans the k entries for the
//                      new worst -- rare after the first few tiles.  A query's rows are spread over 4 x splits partial
//                      lists (gallery split, wave column, half-wave); they go to the workspace.
//   knn_vote_kernel  : one wave per query: the <= 4 x splits x k partial entries are ranked by counting in the defined
//                      order (s descending, j ascending), ranks < k are the neighbours; then the vote, one lane per class.
// No float atomics anywhere; every output is a function of the query row, the gallery and the arguments alone.
#include <float.h>
#include <math.h>

#include "common.hpp"
#include "kernels.hpp"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int KNN_KS = FD / 16;                              // k-steps of a row
constexpr size_t KNN_TILE = (size_t)KNN_KS * 2 * 1024;       // bytes of one 32-row tile: [k-step][piece][lane][16]
constexpr int KNN_BLOCK = 128;                               // queries of a workgroup / gallery rows of a step
constexpr int KNN_SLOTS = 512;                               // partial lists of a workgroup: 256 threads x 2 query tiles
constexpr int KNN_SPLIT_MAX = 8;                             // gallery shares
constexpr int KNN_KMAX = 32, KNN_CMAX = 64;

__device__ __forceinline__ uint32_t knn_pair(_Float16 a, _Float16 b) {
  return (uint32_t)__builtin_bit_cast(uint16_t, a) | ((uint32_t)__builtin_bit_cast(uint16_t, b) << 16);
}

// thread = (tile, 8-element group g8, row r of the tile): 32 consecutive threads write 512 consecutive bytes
__global__ __launch_bounds__(256) void knn_split_kernel(const float* __restrict__ x, int rows, int rows_pad,
                                                        char* __restrict__ out) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  const int r = (int)(t & 31), g8 = (int)((t >> 5) & 127);
  const long long tile = t >> 12, row = tile * 32 + r;
  if (row >= rows_pad) return;
  float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (row < rows) {
    const float4* p = (const float4*)(x + row * FD + g8 * 8);
    const float4 a = p[0], b = p[1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  uint32_t h[4], l[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float a = v[2 * j] * 4096.f, b = v[2 * j + 1] * 4096.f;
    const _Float16 ha = (_Float16)a, hb = (_Float16)b;
    h[j] = knn_pair(ha, hb);
    l[j] = knn_pair((_Float16)(a - (float)ha), (_Float16)(b - (float)hb));
  }
  char* o = out + (size_t)tile * KNN_TILE + (size_t)(g8 >> 1) * 2048 + ((g8 & 1) * 32 + r) * 16;
  *(uint4*)o = make_uint4(h[0], h[1], h[2], h[3]);
  *(uint4*)(o + 1024) = make_uint4(l[0], l[1], l[2], l[3]);
}

struct KnnScan {
  const char* q; const char* g;                  // fragment planes of the queries / the gallery
  const long long* label; const long long* skip;
  float* ps; int* pj;                            // partial lists [n][P][k]
  int n, m, K, k, P, steps, per;                 // steps: 128-row gallery steps in all; per: steps of one share
};

struct KnnFrags { uint4 qh[2], ql[2], gh[2], gl[2]; };

__global__ __launch_bounds__(256) void knn_scan_kernel(KnnScan a) {
  extern __shared__ __attribute__((aligned(16))) char knn_smem[];
  const int k = a.k, m = a.m, K = a.K;
  float* ls = (float*)knn_smem;                                   // [k][KNN_SLOTS]
  int* lj = (int*)(knn_smem + (size_t)k * KNN_SLOTS * 4);         // [k][KNN_SLOTS]
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wq = wave & 1, wg = wave >> 1;
  const long long* __restrict__ label = a.label;
  // a thread touches its own two slots only: no barrier anywhere in this kernel
  for (int r = 0; r < k; ++r) {
    ls[r * KNN_SLOTS + tid] = -INFINITY; ls[r * KNN_SLOTS + 256 + tid] = -INFINITY;
    lj[r * KNN_SLOTS + tid] = -1; lj[r * KNN_SLOTS + 256 + tid] = -1;
  }
  int qi[2], pos[2], skipj[2];
  float thr[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    qi[f] = ((int)blockIdx.x * 4 + wq * 2 + f) * 32 + l31;
    pos[f] = 0;
    thr[f] = qi[f] < a.n ? -INFINITY : INFINITY;                   // a padding query takes nothing
    long long sk = -1;
    if (a.skip != nullptr && qi[f] < a.n) sk = a.skip[qi[f]];
    skipj[f] = (sk >= 0 && sk < m) ? (int)sk : -1;
  }
  const char* qp = a.q + (size_t)((int)blockIdx.x * 4 + wq * 2) * KNN_TILE + lane * 16;
  const char* gp = a.g + (size_t)(wg * 2) * KNN_TILE + lane * 16;
  const int it0 = (int)blockIdx.y * a.per, it1 = it0 + a.per < a.steps ? it0 + a.per : a.steps;
  auto load = [&](int it, int ks, KnnFrags& f) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const char* pq = qp + (size_t)t * KNN_TILE + (size_t)ks * 2048;
      const char* pg = gp + (size_t)(it * 4 + t) * KNN_TILE + (size_t)ks * 2048;
      f.qh[t] = *(const uint4*)pq; f.ql[t] = *(const uint4*)(pq + 1024);
      f.gh[t] = *(const uint4*)pg; f.gl[t] = *(const uint4*)(pg + 1024);
    }
  };
  KnnFrags cur;
  load(it0, 0, cur);
  for (int it = it0; it < it1; ++it) {
    f32x16 acc[2][2];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[f][t] = zero16();
#pragma unroll 2
    for (int ks = 0; ks < KNN_KS; ++ks) {
      // the next k-step's fragments are in flight under this one's twelve MFMAs (past the end: this share's last tile again)
      KnnFrags nx;
      const bool wrap = ks + 1 == KNN_KS;
      load(wrap ? (it + 1 < it1 ? it + 1 : it) : it, wrap ? 0 : ks + 1, nx);
#pragma unroll
      for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          acc[f][t] = mfma_h16(cur.gl[t], cur.qh[f], acc[f][t]);
          acc[f][t] = mfma_h16(cur.gh[t], cur.ql[f], acc[f][t]);
          acc[f][t] = mfma_h16(cur.gh[t], cur.qh[f], acc[f][t]);
        }
      cur = nx;
    }
    const int j0 = (it * 4 + wg * 2) * 32 + 4 * hh;
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float s = acc[f][t][r] * 0x1p-24f;
          if (s > thr[f]) {                                        // (a NaN fails it)
            const int j = j0 + t * 32 + (r & 3) + 8 * (r >> 2);
            bool ok = j < m && j != skipj[f] && s <= FLT_MAX;
            if (ok && label != nullptr) {
              const long long lb = label[j];
              ok = lb >= 0 && lb < K;
            }
            if (ok) {
              const int slot = f * 256 + tid;
              ls[pos[f] * KNN_SLOTS + slot] = s; lj[pos[f] * KNN_SLOTS + slot] = j;
              float ws = ls[slot];
              int wj = lj[slot], wp = 0;
              for (int e = 1; e < k; ++e) {                        // the new worst: smallest s, then largest j
                const float s2 = ls[e * KNN_SLOTS + slot];
                const int j2 = lj[e * KNN_SLOTS + slot];
                if (s2 < ws || (s2 == ws && j2 > wj)) { ws = s2; wj = j2; wp = e; }
              }
              pos[f] = wp; thr[f] = ws;
            }
          }
        }
  }
#pragma unroll
  for (int f = 0; f < 2; ++f)
    if (qi[f] < a.n) {
      const size_t base = ((size_t)qi[f] * a.P + ((int)blockIdx.y * 4 + wg * 2 + hh)) * k;
      const int slot = f * 256 + tid;
      for (int r = 0; r < k; ++r) { a.ps[base + r] = ls[r * KNN_SLOTS + slot]; a.pj[base + r] = lj[r * KNN_SLOTS + slot]; }
    }
}

struct KnnVote {
  const float* ps; const int* pj; const long long* label;
  int n, K, k, E;                                // E = P k partial entries of a query
  float inv_T;
  int* nbr_idx; float* nbr_sim; float* probs; long long* labels;
};

__global__ __launch_bounds__(64) void knn_vote_kernel(KnnVote a) {
  __shared__ float es[4 * KNN_SPLIT_MAX * KNN_KMAX];
  __shared__ int ej[4 * KNN_SPLIT_MAX * KNN_KMAX];
  __shared__ float ss[KNN_KMAX];
  __shared__ int sj[KNN_KMAX], sl[KNN_KMAX];
  __shared__ float pp[KNN_CMAX];
  const int i = blockIdx.x, lane = threadIdx.x, k = a.k, E = a.E, K = a.K;
  for (int e = lane; e < E; e += 64) { es[e] = a.ps[(size_t)i * E + e]; ej[e] = a.pj[(size_t)i * E + e]; }
  if (lane < KNN_KMAX) { ss[lane] = -INFINITY; sj[lane] = -1; sl[lane] = -1; }
  __syncthreads();
  int cnt = 0;
  for (int e = lane; e < E; e += 64) {
    const int j = ej[e];
    if (j < 0) continue;
    ++cnt;
    const float s = es[e];
    int rank = 0;
    for (int e2 = 0; e2 < E; ++e2) {
      const float s2 = es[e2];
      const int j2 = ej[e2];
      rank += (j2 >= 0 && (s2 > s || (s2 == s && j2 < j))) ? 1 : 0;
    }
    if (rank < k) { ss[rank] = s; sj[rank] = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  const int kk = cnt < k ? cnt : k;
  __syncthreads();
  if (lane < k) {
    if (a.nbr_idx != nullptr) a.nbr_idx[(size_t)i * k + lane] = sj[lane];
    if (a.nbr_sim != nullptr) a.nbr_sim[(size_t)i * k + lane] = ss[lane];
  }
  if (a.label == nullptr) return;
  if (lane < kk) sl[lane] = (int)a.label[sj[lane]];               // (a candidate's label lies in 0 .. K - 1)
  __syncthreads();
  float den = 0.f, sc = 0.f;
  const float s0 = ss[0];
  for (int r = 0; r < kk; ++r) {
    const float w = expf(__fmul_rn(ss[r] - s0, a.inv_T));
    den = __fadd_rn(den, w);
    if (sl[r] == lane) sc = __fadd_rn(sc, w);
  }
  const float p = kk > 0 ? sc / den : NAN;
  if (lane < K) {
    pp[lane] = p;
    if (a.probs != nullptr) a.probs[(size_t)i * K + lane] = p;
  }
  __syncthreads();
  if (lane == 0 && a.labels != nullptr) {
    int best = 0;
    for (int c = 1; c < K; ++c)
      if (pp[c] > pp[best]) best = c;
    a.labels[i] = kk > 0 ? best : -1;
  }
}

size_t knn_up256(size_t b) { return (b + 255) & ~(size_t)255; }
int knn_pad(int rows) { return (rows + KNN_BLOCK - 1) / KNN_BLOCK * KNN_BLOCK; }

// the gallery shares of a call: enough workgroups for the chip when the query list alone gives few
void knn_plan(int n, int m, int* splits, int* per) {
  const int steps = knn_pad(m) / KNN_BLOCK, qblocks = knn_pad(n) / KNN_BLOCK;
  int s = (512 + qblocks - 1) / qblocks;
  if (s > KNN_SPLIT_MAX) s = KNN_SPLIT_MAX;
  if (s > steps) s = steps;
  *per = (steps + s - 1) / s;
  *splits = (steps + *per - 1) / *per;            // (no empty share)
}

}  // namespace
}  // namespace cmlpl

extern "C" size_t cmlpl_knn_workspace_bytes(int n, int m, int k) {
  using namespace cmlpl;
  if (n < 1 || m < 1 || k < 1 || k > KNN_KMAX) return 0;
  int splits, per;
  knn_plan(n, m, &splits, &per);
  return knn_up256((size_t)knn_pad(n) * FD * 4) + knn_up256((size_t)knn_pad(m) * FD * 4) +
         2 * knn_up256((size_t)n * splits * 4 * k * 4);
}

extern "C" int cmlpl_knn(const float* d_query, int n, const float* d_gallery, int m, const int64_t* d_gallery_label, int K,
                         const int64_t* d_skip, int k, float inv_T, int32_t* d_nbr_idx, float* d_nbr_sim, float* d_probs,
                         int64_t* d_labels, void* d_workspace, size_t workspace_bytes, void* stream) {
  using namespace cmlpl;
  if (!d_query || !d_gallery || !d_workspace || n < 1 || m < 1 || k < 1 || k > KNN_KMAX) return CMLPL_E_ARG;
  if (d_gallery_label ? (K < 1 || K > KNN_CMAX || !(inv_T > 0.f) || !std::isfinite(inv_T))
                      : (K != 0 || d_probs || d_labels)) return CMLPL_E_ARG;
  if (!aligned_to(15, d_query, d_gallery, d_workspace) || !aligned_to(7, d_gallery_label, d_skip, d_labels) ||
      !aligned_to(3, d_nbr_idx, d_nbr_sim, d_probs)) return CMLPL_E_ARG;
  if (cmlpl_knn_workspace_bytes(n, m, k) > workspace_bytes) return CMLPL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int splits, per;
  knn_plan(n, m, &splits, &per);
  const int npad = knn_pad(n), mpad = knn_pad(m);
  char* w = (char*)d_workspace;
  char* qf = w; w += knn_up256((size_t)npad * FD * 4);
  char* gf = w; w += knn_up256((size_t)mpad * FD * 4);
  const size_t lb = knn_up256((size_t)n * splits * 4 * k * 4);
  float* ps = (float*)w; w += lb;
  int* pj = (int*)w;
  const bool same = d_query == d_gallery && n == m;               // leave-one-out: one set of planes
  hipLaunchKernelGGL(knn_split_kernel, dim3(mpad / 2), dim3(256), 0, st, d_gallery, m, mpad, gf);
  if (!same) hipLaunchKernelGGL(knn_split_kernel, dim3(npad / 2), dim3(256), 0, st, d_query, n, npad, qf);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  KnnScan a = {};
  a.q = same ? gf : qf; a.g = gf;
  a.label = reinterpret_cast<const long long*>(d_gallery_label); a.skip = reinterpret_cast<const long long*>(d_skip);
  a.ps = ps; a.pj = pj; a.n = n; a.m = m; a.K = K; a.k = k; a.P = splits * 4; a.steps = mpad / KNN_BLOCK; a.per = per;
  const size_t lds = (size_t)k * KNN_SLOTS * 8;
  static DevOnce attr_once;
  if ((e = ensure_max_lds(attr_once, knn_scan_kernel)) != hipSuccess) return (int)e;
  hipLaunchKernelGGL(knn_scan_kernel, dim3(npad / KNN_BLOCK, splits), dim3(256), lds, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  KnnVote v = {};
  v.ps = ps; v.pj = pj; v.label = a.label; v.n = n; v.K = K; v.k = k; v.E = a.P * k; v.inv_T = inv_T;
  v.nbr_idx = d_nbr_idx; v.nbr_sim = d_nbr_sim; v.probs = d_probs; v.labels = reinterpret_cast<long long*>(d_labels);
  hipLaunchKernelGGL(knn_vote_kernel, dim3(n), dim3(64), 0, st, v);
  e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
