// The cube-fed step's patch source (cmlpl_batch.d_cube, ABI 6): the augmented patch rows of BOTH networks formed
// straight from the resident scene cube [rows][cols][C] -- no [rows][C][H][W] window tensor exists in HBM.
//   xn[net][s][ch][i][j] = cube[mirror(r + i - hw)][mirror(c + j - hw)][ch] + sigma * N(0,1),
//   pixel r * cols + c = pix[idx[s]] (lab_pix / unl_pix through the batch's RowSel), hw = w / 2, the symmetric
//   (edge-repeating) mirror of MirrowCut / ExtractPatches (tools/hyper_tools.py:35-55, :226-243).
// One workgroup per batch row:
//   gather   as extract_patches_kernel (augment.hip) does: the cube is read along its contiguous channel axis -- a
//            window off the column margin as w spans of w * C consecutive floats, 16-byte loads, eight per thread in
//            flight; a window on the margin pixel by pixel (a wave per pixel, lanes = channels) -- into an LDS tile
//            [window pixel][C | 1] (odd pixel stride);
//   augment  a thread takes the eight consecutive elements 8c .. 8c + 7 of the band-major row: ONE hash call gives their
//            eight normals (noise_normal8, counter (global sample, c): the values augment_kernel, conv0a_fwd_kernel and
//            the fused forward form from the same counters), or the explicit draws of parity mode are read; one row is
//            stored per network, 16 bytes at a time.  (The tile reads of a wave hit 4 banks -- lane stride 8 pixels --
//            which costs ~1.5 k LDS cycles per row against ~5 k cycles of generator work per SIMD: not the bound.)
//            With a spatial mode (sym_mask: include/cmlpl.h, "THE DEFINITION OF A SPATIAL ELEMENT") the row takes one
//            element g of the dihedral group -- one hash call per workgroup, the same for both networks -- and output
//            pixel pix reads the tile at T_g(pix): the gather above stays the contiguous one, the noise stays keyed by
//            the output position, and without a mode (g == 0, uniform) the reads are the ones they were.
// The forward then takes xn as already-augmented plain rows (xsrc_plain) and does not write it again; the backward reads
// it as it always does.
#include "common.hpp"
#include "kernels.hpp"

namespace cmlpl {

struct CubeFeedArgs {
  const float* cube; int rows, cols, C, w;
  const long long* lab_pix; const long long* unl_pix;     // pixel of split row i (row-major index into the scene)
  const float* nz_lab[2]; const float* nz_unl[2];         // explicit N(0,1) draws per network ([bt][C*w*w] / [btu][C*w*w]), or null
  float* xn;                                              // [2][bt + btu][C * w * w]
  int bt, btu, lab0, unl_base;                            // local rows and their global sample indices
  float sigma; uint64_t seed, step;
  RowSel sel;
  int sym_mask;                                           // spatial elements per row less one: 0 none, 3 flips, 7 d4 (include/cmlpl.h)
};

__device__ __forceinline__ int mirror_index(int v, int n) { return v < 0 ? -v - 1 : (v >= n ? 2 * n - 1 - v : v); }

__global__ __launch_bounds__(512) void cube_feed_kernel(CubeFeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) float tile[];   // [w * w][CS]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x;                                 // local batch row
  const int C = a.C, w = a.w, hw = w >> 1, ww = w * w, rows = a.rows, cols = a.cols;
  const int CS = C | 1;                                     // LDS floats per window pixel
  const bool lab = s < a.bt;
  const int sl = lab ? s : s - a.bt;
  const long long k = uni64((lab ? a.lab_pix : a.unl_pix)[rowsel_index(a.sel, lab, sl)]);
  const int r = (int)(k / cols), c = (int)(k - (long long)r * cols);
  const float* cube = a.cube;
  // ---- gather: cube -> tile
  if (c - hw >= 0 && c - hw + w <= cols) {                  // workgroup-uniform: no column of the window is mirrored
    const int NF = w * C, n4 = NF >> 2, NI = w * n4, rem = NF & 3;
    const float inv4 = 1.0f / (float)(n4 > 0 ? n4 : 1), invC = 1.0f / (float)C;
    constexpr int GB = 8;
    // (the placeholder item tc = 0 below is a real 16-byte item of the span: w >= 4 here (make_dims), so n4 >= 1 --
    // extract_patches_kernel, which takes w * C < 4, skips its loads when NI == 0)
    for (int t0 = 0; t0 < NI; t0 += 512 * GB) {
      float4 v[GB];
#pragma unroll
      for (int q = 0; q < GB; ++q) {
        const int t = t0 + tid + 512 * q, tc = t < NI ? t : 0;
        // row of the item: exact for t < 2^22 / n4 (the quotient is at least 0.5 / n4 away from an integer)
        const int i = (int)(((float)tc + 0.5f) * inv4), e4 = tc - i * n4;
        const int rr = mirror_index(r + i - hw, rows);
        v[q] = *(const float4*)(cube + ((long long)rr * cols + (c - hw)) * C + 4 * e4);
      }
#pragma unroll
      for (int q = 0; q < GB; ++q) {
        const int t = t0 + tid + 512 * q;
        if (t < NI) {
          const int i = (int)(((float)t + 0.5f) * inv4), e0 = 4 * (t - i * n4);
          int j = (int)(((float)e0 + 0.5f) * invC), ch = e0 - j * C;
          const float x[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            tile[(i * w + j) * CS + ch] = x[e];
            if (++ch == C) { ch = 0; ++j; }
          }
        }
      }
    }
    if (tid < w * rem) {                                    // the floats of each span beyond its 16-byte items
      const int i = tid / rem, e = (NF & ~3) + (tid - i * rem);
      const int rr = mirror_index(r + i - hw, rows);
      const int j = e / C, ch = e - j * C;
      tile[(i * w + j) * CS + ch] = cube[((long long)rr * cols + (c - hw)) * C + e];
    }
  } else {
    // column margin: a wave takes whole pixels (the mirrored source pixel and its address are wave-uniform),
    // lanes = channels, eight pixels of a wave in flight at once
    constexpr int PB = 8;
    for (int pix0 = wave; pix0 < ww; pix0 += 8 * PB) {
      for (int ch0 = 0; ch0 < C; ch0 += 128) {
        float x[PB][2];
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          const int pix = pix0 + 8 * q, pc = pix < ww ? pix : 0;                        // wave-uniform
          const int i = pc / w, j = pc - i * w;
          const int rr = mirror_index(r + i - hw, rows), cc = mirror_index(c + j - hw, cols);
          const float* src = cube + ((long long)rr * cols + cc) * C;
#pragma unroll
          for (int h = 0; h < 2; ++h) { const int ch = ch0 + 64 * h + lane; x[q][h] = src[ch < C ? ch : 0]; }
        }
#pragma unroll
        for (int q = 0; q < PB; ++q) {
          const int pix = pix0 + 8 * q;
          if (pix < ww) {
#pragma unroll
            for (int h = 0; h < 2; ++h) { const int ch = ch0 + 64 * h + lane; if (ch < C) tile[pix * CS + ch] = x[q][h]; }
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- augment + store: band-major rows of both networks
  const int per = C * ww, npair = (per + 7) >> 3;
  const long long n_all = a.bt + a.btu;
  uint64_t rstep = a.step;
  const cmlpl_dyn* dynr = dyn_row(a.sel.dyn);
  if (dynr != nullptr) rstep = (uint64_t)uni64((long long)dynr->step);
  const uint64_t gs = (uint64_t)(lab ? a.lab0 + sl : a.unl_base + sl);
  const float sigma = a.sigma;
  const float* nz0 = lab ? a.nz_lab[0] : a.nz_unl[0];
  const float* nz1 = lab ? a.nz_lab[1] : a.nz_unl[1];
  const bool expl = nz0 != nullptr;                         // (uniform)
  if (expl) { nz0 += (long long)sl * per; nz1 += (long long)sl * per; }
  float* d0 = a.xn + (long long)s * per;
  float* d1 = d0 + n_all * per;
  // the row's spatial element (workgroup-uniform, the same for both networks): output pixel pix reads the tile at
  // T_g(pix); the noise below stays keyed by the output position
  int g = 0;
  if (a.sym_mask != 0)
    g = __builtin_amdgcn_readfirstlane((int)((noise_hash(a.seed, rstep, STREAM_SYM, noise_ctr(gs, 0)).x >> 29) & (uint32_t)a.sym_mask));
  for (int p = tid; p < npair; p += 512) {
    const int e0 = 8 * p;
    int ch = e0 / ww, pix = e0 - ch * ww;
    int wi = 0, wj = 0;
    if (g != 0) { wi = pix / w; wj = pix - wi * w; }
    float x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      int sp = pix;
      if (g != 0) {
        int si, sj;
        sym_source(g, w, w, wi, wj, si, sj);
        sp = si * w + sj;
        if (++wj == w) { wj = 0; if (++wi == w) wi = 0; }
      }
      x[q] = tile[(e0 + q < per) ? sp * CS + ch : 0];
      if (++pix == ww) { pix = 0; ++ch; }
    }
    const bool full = e0 + 8 <= per;
    float y0[8], y1[8];
    if (sigma != 0.f) {
      float4 l0, h0, l1, h1;
      if (expl) {
        if (full) {
          l0 = *(const float4*)(nz0 + e0); h0 = *(const float4*)(nz0 + e0 + 4);
          l1 = *(const float4*)(nz1 + e0); h1 = *(const float4*)(nz1 + e0 + 4);
        } else {
          float t0[8], t1[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) { const int e = e0 + q < per ? e0 + q : per - 1; t0[q] = nz0[e]; t1[q] = nz1[e]; }
          l0 = make_float4(t0[0], t0[1], t0[2], t0[3]); h0 = make_float4(t0[4], t0[5], t0[6], t0[7]);
          l1 = make_float4(t1[0], t1[1], t1[2], t1[3]); h1 = make_float4(t1[4], t1[5], t1[6], t1[7]);
        }
      } else {
        noise_normal8(a.seed, rstep, STREAM_NOISE_XP, gs, (uint32_t)p, l0, h0);
        noise_normal8(a.seed, rstep, STREAM_NOISE_XP + 1, gs, (uint32_t)p, l1, h1);
      }
      const float z0[8] = {l0.x, l0.y, l0.z, l0.w, h0.x, h0.y, h0.z, h0.w};
      const float z1[8] = {l1.x, l1.y, l1.z, l1.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
      for (int q = 0; q < 8; ++q) { y0[q] = fmaf(z0[q], sigma, x[q]); y1[q] = fmaf(z1[q], sigma, x[q]); }
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) { y0[q] = x[q]; y1[q] = x[q]; }
    }
    if (full) {
      *(float4*)(d0 + e0) = make_float4(y0[0], y0[1], y0[2], y0[3]);
      *(float4*)(d0 + e0 + 4) = make_float4(y0[4], y0[5], y0[6], y0[7]);
      *(float4*)(d1 + e0) = make_float4(y1[0], y1[1], y1[2], y1[3]);
      *(float4*)(d1 + e0 + 4) = make_float4(y1[4], y1[5], y1[6], y1[7]);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q)
        if (e0 + q < per) { d0[e0 + q] = y0[q]; d1[e0 + q] = y1[q]; }
    }
  }
}

size_t cube_feed_lds(int C, int w) { return (size_t)w * w * (C | 1) * 4; }

hipError_t launch_cube_feed(const float* cube, int rows, int cols, int C, int w, const long long* lab_pix,
                            const long long* unl_pix, int bt, int btu, int lab0, int unl_base,
                            const float* const* noise8, float sigma, uint64_t seed, uint64_t step, float* xn,
                            const RowSel* sel, hipStream_t st, int sym_mode) {
  const size_t lds = cube_feed_lds(C, w);
  if (lds > LDS_MAX || bt + btu < 1 || sym_mode < 0 || sym_mode > 2) return hipErrorInvalidValue;
  static DevOnce attr_once;
  {
    hipError_t e = ensure_max_lds(attr_once, cube_feed_kernel);
    if (e != hipSuccess) return e;
  }
  CubeFeedArgs a;
  a.cube = cube; a.rows = rows; a.cols = cols; a.C = C; a.w = w;
  a.lab_pix = lab_pix; a.unl_pix = unl_pix;
  for (int i = 0; i < 2; ++i) {                             // the patch draws of the reference's order (cmlpl_augment)
    a.nz_lab[i] = noise8 ? noise8[2 * i] : nullptr;
    a.nz_unl[i] = noise8 ? noise8[4 + 2 * i] : nullptr;
  }
  a.xn = xn; a.bt = bt; a.btu = btu; a.lab0 = lab0; a.unl_base = unl_base;
  a.sigma = sigma; a.seed = seed; a.step = step;
  a.sel = sel != nullptr ? *sel : RowSel();
  a.sym_mask = sym_mode == 0 ? 0 : (sym_mode == 1 ? 3 : 7);
  hipLaunchKernelGGL(cube_feed_kernel, dim3(bt + btu), dim3(512), lds, st, a);
  return hipGetLastError();
}

}  // namespace cmlpl
