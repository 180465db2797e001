// Edge-preserving spatial smoothing of class probability maps (include/cmlpl.h, "THE DEFINITION OF A SMOOTHED MAP"):
// the one kernel of the library that looks at a prediction as an IMAGE.  Per scene pixel i = (y, x):
//   q[i][c] = sum_j w_ij p[j][c] / sum_j w_ij over the taps j = (y + dy, x + dx), |dy|, |dx| <= R, inside the scene,
//   w_ij    = expf(-(fmaf(d2, b, fl(s a)))),  s = dy^2 + dx^2,  d2 = the squared guide distance (an fmaf chain)
// and from q the label / confidence / entropy by cmlpl_ensemble's rules.
//
// A workgroup of 256 threads owns a tile of 32 x 8 output pixels, one pixel per thread, lanes running along x.  It stages
// the tile and its halo of R pixels ONCE into LDS, channel-planar ([guide channel | class][halo row][halo column]): the
// global loads walk the [pixel][K] rows in address order (one lane per (pixel, class), consecutive lanes consecutive
// words), a tap is then one ds_read_b32 per plane in which the 32 lanes of a half-wave read 32 consecutive words --
// conflict-free whatever the radius.  The plane stride is 4 mod 32 words, which keeps the staging stores at two lanes
// per bank or fewer.  Each thread walks its taps dy ascending, dx ascending within dy, forms each weight once with
// one expf and accumulates up to 16 classes in registers; the centre pixel's guide stays in registers.  K > 16 runs in
// chunks of 16 classes over the guide staged once: the weights are formed again per chunk (the same bits), the sums of
// every chunk stay in registers until the pixel's row is complete (the NaN rule needs the whole row).
//
// A pixel's arithmetic does not look at the tile: taps outside the scene are staged as 0 and weighted 0, which adds
// exactly nothing, so the result is a function of the scene alone and the same bytes on every run.  No atomics, no
// scratch, no read outside the two input buffers (every global load is guarded by its scene coordinate and channel).
//
// LDS and occupancy (bytes = (G + KC) planes x ((32 + 2R)(8 + 2R) rounded to 4 mod 32) words; KC = the class registers):
//   R = 8, K = 16, G = 8   24 planes x 1156 words = 108 KiB   1 workgroup (4 waves) per CU
//   R = 8, K = 9,  G = 3   15 planes x 1156 words =  68 KiB   2 workgroups per CU
//   R = 4, K = 9,  G = 3   15 planes x  644 words =  38 KiB   4 workgroups per CU
//   R = 2, K = 9,  G = 3   15 planes x  452 words =  27 KiB   6 workgroups per CU (4 with K = 16, G = 3)
//   R = 1, K = 9,  G = 3   15 planes x  356 words =  21 KiB   7 workgroups per CU
// (registers: 20 .. 50 VGPRs up to K = 16, 102 at most for K = 64: LDS is what limits in every row above.)
// Open: the guide channels are a run-time count walked under uniform branches, one LDS round trip behind the other;
// guide planes as a template parameter would put a tap's G + K reads in flight together.  The output rows are stored
// by their owning thread; a transpose through the freed LDS would coalesce them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdint.h>

#include "../../include/cmlpl.h"
#include "kernels.hpp"
#include "rowgroup.hpp"

namespace cmlpl {
namespace {

constexpr int SM_THREADS = 256;
constexpr int SM_TX = 32, SM_TY = 8;      // the tile: one output pixel per thread, a wave is two rows of 32
constexpr int SM_MAX_G = 8;               // guide channels
constexpr int SM_MAX_R = 8;
constexpr int SM_CHUNK = 16;              // classes per chunk when K > 16

struct SmoothArgs {
  const float* probs; const float* guide; long long guide_stride;
  int G, rows, cols, K, R;
  int tiles_x;
  int hw_inv;                             // ceil(2^16 / (32 + 2R)): halo pixel -> halo row without a division
  float a, b;
  float* out; long long* labels; float* conf; float* entropy;
};

__host__ __device__ inline int smooth_plane_words(int R) {
  const int n = (SM_TX + 2 * R) * (SM_TY + 2 * R);
  return (n - 4 + 31) / 32 * 32 + 4;      // >= n, and 4 mod 32
}

// KC: class registers of a chunk (planes staged per chunk; classes past K are staged as 0 and never stored);
// NCH: chunks (1: K <= KC; else KC == 16 and K <= 16 NCH)
template <int KC, int NCH> __global__ __launch_bounds__(SM_THREADS) void smooth_kernel(SmoothArgs s) {
  extern __shared__ __align__(16) float sm_lds[];
  const int tid = threadIdx.x;
  const int R = s.R, G = s.G, K = s.K, rows = s.rows, cols = s.cols;
  const int HW = SM_TX + 2 * R, HH = SM_TY + 2 * R, HP = HW * HH;
  const int PS = smooth_plane_words(R);
  const int tile_y = (int)blockIdx.x / s.tiles_x, tile_x = (int)blockIdx.x - tile_y * s.tiles_x;
  const int hx0 = tile_x * SM_TX - R, hy0 = tile_y * SM_TY - R;      // scene coordinates of the halo's first pixel
  float* gl = sm_lds;                     // [G][PS]
  float* pl = sm_lds + G * PS;            // [KC][PS]

  // ---- the guide of tile + halo, once: lane = (halo pixel, channel of 8), channels past G idle
  if (G > 0) {
#pragma unroll 4
    for (int e = tid; e < HP * SM_MAX_G; e += SM_THREADS) {
      const int hp = e >> 3, c = e & 7;
      const int hy = (hp * s.hw_inv) >> 16, hx = hp - hy * HW;      // (exact: hp (32 + 2R) < 2^16)
      const int y = hy0 + hy, x = hx0 + hx;
      if (c < G) {
        float v = 0.f;
        if ((unsigned)y < (unsigned)rows && (unsigned)x < (unsigned)cols)
          v = s.guide[((long long)y * cols + x) * s.guide_stride + c];
        gl[c * PS + hp] = v;
      }
    }
  }

  const int tx = tid & (SM_TX - 1), ty = tid >> 5;
  const int x = tile_x * SM_TX + tx, y = tile_y * SM_TY + ty;
  const int ci = (ty + R) * HW + tx + R;  // this thread's pixel in a plane
  float acc[NCH][KC];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int c = 0; c < KC; ++c) acc[ch][c] = 0.f;
  float den = 0.f;
  float gc[SM_MAX_G] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    const int c0 = ch * KC;
    if (ch > 0) __syncthreads();          // the previous chunk's taps are read
    // ---- the probabilities of tile + halo, classes c0 .. c0 + KC - 1: lane = (halo pixel, class)
#pragma unroll 4
    for (int e = tid; e < HP * KC; e += SM_THREADS) {
      const int hp = e / KC, c = e - hp * KC;
      const int hy = (hp * s.hw_inv) >> 16, hx = hp - hy * HW;
      const int yy = hy0 + hy, xx = hx0 + hx;
      float v = 0.f;
      if ((unsigned)yy < (unsigned)rows && (unsigned)xx < (unsigned)cols && c0 + c < K)
        v = s.probs[((long long)yy * cols + xx) * K + c0 + c];
      pl[c * PS + hp] = v;
    }
    __syncthreads();
    if (ch == 0) {
#pragma unroll
      for (int g = 0; g < SM_MAX_G; ++g) gc[g] = g < G ? gl[g * PS + ci] : 0.f;
    }
    // ---- the taps: dy ascending, dx ascending within dy
    for (int dy = -R; dy <= R; ++dy) {
      const bool yin = (unsigned)(y + dy) < (unsigned)rows;
      const int orow = ci + dy * HW;
      for (int dx = -R; dx <= R; ++dx) {
        const int o = orow + dx;
        float d2 = 0.f;
#pragma unroll
        for (int g = 0; g < SM_MAX_G; ++g) {
          if (g < G) {                    // (uniform)
            const float d = gc[g] - gl[g * PS + o];
            d2 = fmaf(d, d, d2);
          }
        }
        const float ex = fmaf(d2, s.b, __fmul_rn((float)(dy * dy + dx * dx), s.a));
        const bool in = yin && (unsigned)(x + dx) < (unsigned)cols;
        const float w = in ? expf(-ex) : 0.f;
        if (ch == 0) den += w;
#pragma unroll
        for (int c = 0; c < KC; ++c) acc[ch][c] = fmaf(w, pl[c * PS + o], acc[ch][c]);
      }
    }
  }

  if (x >= cols || y >= rows) return;     // (behind the last barrier)
  const long long pix = (long long)y * cols + x;
  bool bad = false;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      acc[ch][c] = acc[ch][c] / den;
      if (ch * KC + c < K) bad = bad || (acc[ch][c] != acc[ch][c]);
    }
  const float qnan = __builtin_nanf("");
  float best = 0.f, sum = 0.f;
  int label = 0;
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      const int k = ch * KC + c;
      if (k < K) {                        // (uniform)
        const float q = bad ? qnan : acc[ch][c];
        if (s.out != nullptr) s.out[pix * K + k] = q;
        // the first maximum; a NaN counts as the maximum and the first NaN wins
        if (k == 0) best = q;
        else if (best == best && (q != q || q > best)) { best = q; label = k; }
        sum += (q == 0.f) ? 0.f : q * logf(q);
      }
    }
  if (s.labels != nullptr) s.labels[pix] = label;
  if (s.conf != nullptr) s.conf[pix] = best;
  if (s.entropy != nullptr) s.entropy[pix] = 0.f - sum;
}

template <int KC, int NCH> hipError_t launch_kc(const SmoothArgs& s, hipStream_t st) {
  const size_t lds = (size_t)(s.G + KC) * smooth_plane_words(s.R) * sizeof(float);
  const long long tiles = (long long)s.tiles_x * ((s.rows + SM_TY - 1) / SM_TY);
  hipLaunchKernelGGL((smooth_kernel<KC, NCH>), dim3((unsigned)tiles), dim3(SM_THREADS), lds, st, s);
  return hipGetLastError();
}

hipError_t launch_smooth(const SmoothArgs& s, hipStream_t st) {
  static DevOnce once;                    // R = 8 with 16 classes and a guide stages more than 64 KiB
  const hipError_t e = ensure_max_lds(once, smooth_kernel<1, 1>, smooth_kernel<2, 1>, smooth_kernel<4, 1>,
                                      smooth_kernel<8, 1>, smooth_kernel<12, 1>, smooth_kernel<16, 1>,
                                      smooth_kernel<16, 2>, smooth_kernel<16, 3>, smooth_kernel<16, 4>);
  if (e != hipSuccess) return e;
  if (s.K <= 1) return launch_kc<1, 1>(s, st);
  if (s.K <= 2) return launch_kc<2, 1>(s, st);
  if (s.K <= 4) return launch_kc<4, 1>(s, st);
  if (s.K <= 8) return launch_kc<8, 1>(s, st);
  if (s.K <= 12) return launch_kc<12, 1>(s, st);
  if (s.K <= 16) return launch_kc<16, 1>(s, st);
  if (s.K <= 32) return launch_kc<SM_CHUNK, 2>(s, st);
  if (s.K <= 48) return launch_kc<SM_CHUNK, 3>(s, st);
  return launch_kc<SM_CHUNK, 4>(s, st);
}

}  // namespace
}  // namespace cmlpl

extern "C" int cmlpl_smooth_probs(const float* d_probs, const float* d_guide, int64_t guide_stride, int guide_ch,
                                  int rows, int cols, int K, int radius, float sigma_s, float sigma_r,
                                  float* d_out_probs, int64_t* d_labels, float* d_conf, float* d_entropy, void* stream) {
  using namespace cmlpl;
  if (K < 1 || K > 64 || radius < 1 || radius > SM_MAX_R || guide_ch < 0 || guide_ch > SM_MAX_G || rows < 1 || cols < 1)
    return CMLPL_E_ARG;
  if ((int64_t)rows * cols > INT32_MAX) return CMLPL_E_ARG;
  if (guide_ch > 0 && (!d_guide || guide_stride < guide_ch)) return CMLPL_E_ARG;
  if (!std::isfinite(sigma_s) || !(sigma_s > 0.f)) return CMLPL_E_ARG;
  if (!(sigma_r > 0.f)) return CMLPL_E_ARG;                         // (a NaN fails the comparison; +inf is legal: b = 0)
  if (!d_probs || (!d_out_probs && !d_labels)) return CMLPL_E_ARG;
  if (!aligned_to(3, d_probs, d_guide, d_out_probs, d_conf, d_entropy) || !aligned_to(7, d_labels)) return CMLPL_E_ARG;
  const int64_t count = (int64_t)rows * cols * K;
  if (d_out_probs && d_out_probs < d_probs + count && d_probs < d_out_probs + count) return CMLPL_E_ARG;   // not in place
  SmoothArgs s = {};
  s.a = (float)(1.0 / (2.0 * (double)sigma_s * (double)sigma_s));
  s.b = (float)(1.0 / (2.0 * (double)sigma_r * (double)sigma_r));
  if (!std::isfinite(s.a) || !std::isfinite(s.b)) return CMLPL_E_ARG;   // a sigma so small that the centre tap would be 0 x inf
  s.probs = d_probs; s.guide = guide_ch > 0 ? d_guide : nullptr; s.guide_stride = (long long)guide_stride;
  s.G = guide_ch; s.rows = rows; s.cols = cols; s.K = K; s.R = radius;
  s.tiles_x = (cols + SM_TX - 1) / SM_TX;
  s.hw_inv = (65536 + SM_TX + 2 * radius - 1) / (SM_TX + 2 * radius);
  s.out = d_out_probs; s.labels = reinterpret_cast<long long*>(d_labels); s.conf = d_conf; s.entropy = d_entropy;
  const hipError_t e = launch_smooth(s, (hipStream_t)stream);
  return e == hipSuccess ? 0 : (int)e;
}
