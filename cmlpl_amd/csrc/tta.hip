// Test-time augmentation: the noisy VIEWS of a scene pixel's window and spectrum as tensors in HBM (include/cmlpl.h,
// "THE DEFINITION OF A VIEW").  The fused cube-fed forward forms the same window values in registers while it stages its
// slab (conv3x3.hip: conv3x3_kernel with TAIL 4 / 5) and never needs the window tensor; these two kernels serve
//   tta_patches_kernel : the by-patches path (windows the fused forward does not take, the reference's 20 x 20 x 60) and
//                        whoever wants to LOOK at a view -- cmlpl_extract_patches plus the view's noise,
//                        out[s][ch][i][j] = cube[mirror(r + i' - hw)][mirror(c + j' - hw)][ch] + sigma z,
//                        (i', j') = the view's spatial element applied to (i, j) (sym_source; the identity by default)
//   tta_spectra_kernel : the spectral branch's rows of a view, [n][bands], into the workspace in front of launch_spe_fwd.
// One workgroup per list entry.  The gather's item is EIGHT consecutive bands of one window pixel -- contiguous in the
// band-last cube, and by the definition one hash call (noise_normal8: pair p QP / 2 + octet) -- into an LDS tile
// [window pixel][C | 1] (odd pixel stride); the scatter then writes the band-major window along its contiguous pixel axis.
#include "common.hpp"
#include "kernels.hpp"

namespace cmlpl {

struct TtaPatchArgs {
  const float* cube; int rows, cols, C, w;
  const long long* pix; int n;
  float* out;
  float sigma; uint64_t seed; uint32_t view;
  int sym;                                                // the view's spatial element, 0..7
};

__global__ __launch_bounds__(256) void tta_patches_kernel(TtaPatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [w * w][C | 1]
  const int tid = threadIdx.x;
  const int s = blockIdx.x;
  const int C = a.C, w = a.w, hw = w >> 1, ww = w * w, rows = a.rows, cols = a.cols;
  const int CS = C | 1;
  const long long last = (long long)rows * cols - 1;
  long long P = uni64(a.pix[s]);
  P = P < 0 ? 0 : (P > last ? last : P);                    // (clamped: the list is data on the device)
  const int r = (int)(P / cols), c = (int)(P - (long long)r * cols);
  const int NO = (C + 7) >> 3;                              // band octets per window pixel
  const int HQ = 2 * ((C + 15) >> 4);                       // QP / 2: hash calls (pairs of band quads) per window pixel
  const float sigma = a.sigma;
  for (int it = tid; it < ww * NO; it += 256) {
    const int p = it / NO, o = it - p * NO, i = p / w, j = p - i * w;
    int si, sj;                                             // output pixel p shows the window's own pixel T_sym(p); the noise stays keyed by p
    sym_source(a.sym, w, w, i, j, si, sj);
    int rr = r + si - hw, cc = c + sj - hw;
    rr = rr < 0 ? -rr - 1 : (rr >= rows ? 2 * rows - 1 - rr : rr);
    cc = cc < 0 ? -cc - 1 : (cc >= cols ? 2 * cols - 1 - cc : cc);
    const float* src = a.cube + ((long long)rr * cols + cc) * C;
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int b = 8 * o + q; x[q] = src[b < C ? b : C - 1]; }
    if (sigma != 0.f) {
      float4 lo, hi;
      noise_normal8(a.seed, (uint64_t)a.view, STREAM_TTA_XP, (uint64_t)P, (uint32_t)(p * HQ + o), lo, hi);
      const float z[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) x[q] = fmaf(z[q], sigma, x[q]);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) { const int b = 8 * o + q; if (b < C) tile[p * CS + b] = x[q]; }
  }
  __syncthreads();
  float* o = a.out + (long long)s * C * ww;
  for (int e = tid; e < C * ww; e += 256) {
    const int ch = e / ww, px = e - ch * ww;
    o[e] = tile[px * CS + ch];
  }
}

// out[i][k] = view of spectrum row (rows ? rows[i] : i) of `spectra`, keyed by scene pixel P = pix ? clamp(pix[i]) : pix0 + i;
// a thread per (item, band quad) = one noise_normal4 call
__global__ __launch_bounds__(256) void tta_spectra_kernel(const float* __restrict__ spectra, const long long* __restrict__ rows,
                                                          const long long* __restrict__ pix, long long pix0, long long last,
                                                          int n, int bands, float* __restrict__ out, float sigma,
                                                          uint64_t seed, uint32_t view) {
  const int NQ = (bands + 3) >> 2;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)n * NQ) return;
  const int i = (int)(idx / NQ), q = (int)(idx - (long long)i * NQ);
  long long P = pix0 + i;
  if (pix != nullptr) { P = pix[i]; P = P < 0 ? 0 : (P > last ? last : P); }
  const long long row = rows != nullptr ? rows[i] : (long long)i;
  const float* src = spectra + row * bands;
  float* dst = out + (long long)i * bands;
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (sigma != 0.f) z = noise_normal4(seed, (uint64_t)view, STREAM_TTA_X, noise_ctr((uint64_t)P, (uint32_t)q));
  const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 4 * q + e;
    if (k < bands) dst[k] = sigma != 0.f ? fmaf(zz[e], sigma, src[k]) : src[k];
  }
}

size_t tta_patches_lds(int C, int w) { return (size_t)w * w * (C | 1) * 4; }

hipError_t launch_tta_patches(const float* cube, int rows, int cols, int C, int w, const long long* pix, int n, float* out,
                              const ViewKey& view, hipStream_t st) {
  const size_t lds = tta_patches_lds(C, w);
  if (lds > LDS_MAX || n < 1) return hipErrorInvalidValue;
  static DevOnce attr_once;
  {
    hipError_t e = ensure_max_lds(attr_once, tta_patches_kernel);
    if (e != hipSuccess) return e;
  }
  TtaPatchArgs a;
  a.cube = cube; a.rows = rows; a.cols = cols; a.C = C; a.w = w; a.pix = pix; a.n = n; a.out = out;
  a.sigma = view.sigma; a.seed = view.seed; a.view = view.view; a.sym = (int)(view.sym & 7u);
  hipLaunchKernelGGL(tta_patches_kernel, dim3(n), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t launch_tta_spectra(const float* spectra, const long long* spec_rows, const long long* pix, long long pix0,
                              long long scene_pixels, int n, int bands, float* out, const ViewKey& view, hipStream_t st) {
  if (n < 1 || bands < 1) return hipErrorInvalidValue;
  const long long items = (long long)n * ((bands + 3) >> 2);
  hipLaunchKernelGGL(tta_spectra_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, spectra, spec_rows, pix, pix0,
                     scene_pixels - 1, n, bands, out, view.sigma, view.seed, view.view);
  return hipGetLastError();
}

}  // namespace cmlpl
