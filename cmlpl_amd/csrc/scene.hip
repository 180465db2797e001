// Scene preprocessing on the device (reference sample_generation.py:21-73 -> tools/hyper_tools.py:285-292 SampleGen):
// from the raw scene X [N pixels][B bands] (its .mat dtype) to the z-scored PCA cube and the z-scored spectra, in fp64
// as numpy computes them:
//   mu = mean(X) per band;  G = (X - mu)^T (X - mu)  [B][B]                    (PCANorm, :25-32; np.cov = G / (N - 1))
//   -- host: U = svd(G / (N - 1))[0] (the reference's LAPACK call, so the singular-vector signs are the reference's) --
//   P = (X - mu) U[:, :n_PC];  cube = fp32((P - mean(P)) / std(P))             (featureNormalize(., 1), :8-22)
//   spectra = (X - mu) / std(X) in fp64, std(X)_b = sqrt(G_bb / N)             (what the reference saves as X.npy)
// Both products run on v_mfma_f64_16x16x4_f64.  Every reduction is deterministic: the pixels are cut into chunks of
// CHUNK (a constant, not a function of the CU count), each chunk writes its partial to the workspace, and one fold
// kernel sums the partials in chunk order.  No atomics: the same input gives a bit-identical cube on every run.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/cmlpl.h"

namespace {

constexpr int CHUNK = 2048;   // pixels per reduction partial
constexpr int MAXB = 256;     // bands a scene may have (padded to 16 for the Gram tiles)
constexpr int KS = 16;        // pixels per LDS stage of the Gram kernel
constexpr int PW = 64;        // pixels per projection workgroup (4 waves x 16)

typedef double f64x4 __attribute__((ext_vector_type(4)));

inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
inline int pad16(int v) { return (v + 15) & ~15; }
inline long long nchunks(long long n) { return (n + CHUNK - 1) / CHUNK; }
inline int chk(hipError_t e) { return e == hipSuccess ? 0 : (int)e; }

// ------------------------------------------------------------------------------------------------
// part[chunk][j] = sum over the chunk's pixels, in order, of x[p][j] (SQ = 0) or (x[p][j] - center[j])^2 (SQ = 1),
// j < ncols <= 256.  Four groups of 256 threads take a quarter of the chunk each; the four sums are added in group
// order.
// ------------------------------------------------------------------------------------------------
template <typename T, int SQ>
__global__ __launch_bounds__(1024) void colsum_kernel(const T* __restrict__ x, long long n, int ld, int ncols,
                                                      const double* __restrict__ center, double* __restrict__ part) {
  __shared__ double red[4][MAXB];
  const int j = threadIdx.x & (MAXB - 1), g = threadIdx.x >> 8;
  const long long q0 = (long long)blockIdx.x * CHUNK + g * (CHUNK / 4);
  const long long q1 = q0 + CHUNK / 4 < n ? q0 + CHUNK / 4 : n;
  double acc = 0.0;
  if (j < ncols) {
    const double c = SQ ? center[j] : 0.0;
#pragma unroll 8
    for (long long p = q0; p < q1; ++p) {
      double v = (double)x[p * ld + j];
      if (SQ) {
        v -= c;
        v *= v;
      }
      acc += v;
    }
  }
  red[g][j] = acc;
  __syncthreads();
  if (g == 0 && j < ncols) part[(long long)blockIdx.x * ncols + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// out[o] = (sum over c < nparts, in order, of part[c * part_ld + (o / ocols) * in_ld + o % ocols]) / div,
// o < orows * ocols
__global__ __launch_bounds__(256) void fold_kernel(const double* __restrict__ part, long long nparts, long long part_ld,
                                                   int orows, int ocols, int in_ld, double div, double* __restrict__ out) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= orows * ocols) return;
  const int r = o / ocols;
  const long long i = (long long)r * in_ld + (o - r * ocols);
  double acc = 0.0;
#pragma unroll 8
  for (long long c = 0; c < nparts; ++c) acc += part[c * part_ld + i];
  out[o] = acc / div;
}

// ------------------------------------------------------------------------------------------------
// Gram partial of one chunk and one 16-band row strip: part[chunk][16 ti + i][j] = sum over the chunk's pixels p of
// (x[p][16 ti + i] - mu) (x[p][j] - mu), j < Bp (bands beyond B and pixels beyond N are zero).  The chunk is staged
// KS pixels at a time in LDS, centred, as st[k][b]; wave w owns the column tiles tj = w, w + 4, w + 8, w + 12.
// v_mfma_f64_16x16x4_f64 (k = 4 pixels): lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
// its four results are C/D[row = (l >> 4) + 4 r][col = l & 15], r = 0..3 -- the f64 layout, NOT the f32 one.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gram_kernel(const T* __restrict__ x, long long n, int B, int Bp,
                                                   const double* __restrict__ mu, double* __restrict__ part) {
  __shared__ double st[KS * (MAXB + 1)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ti = blockIdx.y, nt = Bp >> 4, LS = Bp + 1;
  const int kr = lane >> 4, kc = lane & 15;
  const long long p0 = (long long)blockIdx.x * CHUNK;
  const long long p1 = p0 + CHUNK < n ? p0 + CHUNK : n;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (long long s = p0; s < p1; s += KS) {
    __syncthreads();                                   // the previous stage has been read
    for (int e = tid; e < KS * Bp; e += 256) {
      const int k = e / Bp, b = e - k * Bp;
      const long long p = s + k;
      double v = 0.0;
      if (p < p1 && b < B) v = (double)x[p * B + b] - mu[b];
      st[k * LS + b] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < KS; k0 += 4) {
      const double a = st[(k0 + kr) * LS + ti * 16 + kc];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int tj = wave + 4 * t;
        if (tj < nt) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, st[(k0 + kr) * LS + tj * 16 + kc], acc[t], 0, 0, 0);
      }
    }
  }
  double* out = part + (long long)blockIdx.x * Bp * Bp;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tj = wave + 4 * t;
    if (tj < nt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(long long)(ti * 16 + kr + 4 * r) * Bp + tj * 16 + kc] = acc[t][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Projection P[p][c] = sum_b (x[p][b] - mu[b]) U[b][c] for c < npcp (U [B][npc] row-major; columns beyond npc are
// zero).  Wave w of workgroup (bx, by) takes pixels 64 bx + 16 w .. +16 and the component tiles 4 by .. 4 by + 3;
// k = 4 bands per MFMA: A[i = pixel][k = band], B[k = band][j = component], results as in gram_kernel.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void project_kernel(const T* __restrict__ x, long long n, int B,
                                                      const double* __restrict__ mu, const double* __restrict__ U,
                                                      int npc, int npcp, double* __restrict__ P) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int kr = lane >> 4, kc = lane & 15;
  const long long pw = (long long)blockIdx.x * PW + wave * 16;
  if (pw >= n) return;                                 // wave-uniform
  const long long pa = pw + kc;
  const int tc0 = blockIdx.y * 4;
  f64x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  for (int b0 = 0; b0 < B; b0 += 4) {
    const int b = b0 + kr;
    const double a = (pa < n && b < B) ? (double)x[pa * B + b] - mu[b] : 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int c = (tc0 + t) * 16 + kc;
      if ((tc0 + t) * 16 < npcp) {
        const double u = (b < B && c < npc) ? U[(long long)b * npc + c] : 0.0;
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, u, acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if ((tc0 + t) * 16 < npcp) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long p = pw + kr + 4 * r;
        if (p < n) P[p * npcp + (tc0 + t) * 16 + kc] = acc[t][r];
      }
    }
  }
}

// spectra[p][b] = (x[p][b] - mu[b]) / sqrt(G[b][b] / N)   (np.std: the root of the mean square deviation)
template <typename T>
__global__ __launch_bounds__(256) void spectra_kernel(const T* __restrict__ x, long long n, int B,
                                                      const double* __restrict__ mu, const double* __restrict__ G,
                                                      double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * B) return;
  const int b = (int)(i % B);
  out[i] = ((double)x[i] - mu[b]) / sqrt(G[(long long)b * B + b] / (double)n);
}

// cube[p][c] = fp32((P[p][c] - m[c]) / sqrt(v[c])), c < npc
__global__ __launch_bounds__(256) void cube_kernel(const double* __restrict__ P, long long n, int npc, int npcp,
                                                   const double* __restrict__ m, const double* __restrict__ v,
                                                   float* __restrict__ cube) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * npc) return;
  const long long p = i / npc;
  const int c = (int)(i - p * npc);
  cube[i] = (float)((P[p * npcp + c] - m[c]) / sqrt(v[c]));
}

unsigned grid1(long long elems) { return (unsigned)((elems + 255) / 256); }

bool scene_ok(int dtype, long long n, int B, int npc) {
  return dtype >= CMLPL_SCENE_U16 && dtype <= CMLPL_SCENE_F64 && n >= 2 && B >= 1 && B <= MAXB &&
         npc >= 0 && npc <= B && n * B < (1LL << 40);
}

struct ProjWs { double *P, *part, *m, *v; };

ProjWs project_ws(void* base, long long n, int npcp) {
  char* p = (char*)base;
  ProjWs w;
  w.P = (double*)p;      p += up256((size_t)n * npcp * 8);
  w.part = (double*)p;   p += up256((size_t)nchunks(n) * npcp * 8);
  w.m = (double*)p;      p += up256((size_t)npcp * 8);
  w.v = (double*)p;
  return w;
}

template <typename T>
hipError_t gram_run(const T* x, long long n, int B, double* mu, double* G, double* part, hipStream_t st) {
  const long long nch = nchunks(n);
  const int Bp = pad16(B);
  hipLaunchKernelGGL((colsum_kernel<T, 0>), dim3((unsigned)nch), dim3(1024), 0, st, x, n, B, B, (const double*)nullptr,
                     part);
  hipLaunchKernelGGL(fold_kernel, dim3(grid1(B)), dim3(256), 0, st, part, nch, (long long)B, 1, B, 0, (double)n, mu);
  hipLaunchKernelGGL(gram_kernel<T>, dim3((unsigned)nch, (unsigned)(Bp / 16)), dim3(256), 0, st, x, n, B, Bp,
                     (const double*)mu, part);
  hipLaunchKernelGGL(fold_kernel, dim3(grid1((long long)B * B)), dim3(256), 0, st, part, nch, (long long)Bp * Bp, B, B,
                     Bp, 1.0, G);
  return hipGetLastError();
}

template <typename T>
hipError_t project_run(const T* x, long long n, int B, const double* mu, const double* G, const double* U, int npc,
                       float* cube, double* spectra, void* ws, hipStream_t st) {
  const long long nch = nchunks(n);
  const int npcp = pad16(npc);
  if (spectra) hipLaunchKernelGGL(spectra_kernel<T>, dim3(grid1(n * B)), dim3(256), 0, st, x, n, B, mu, G, spectra);
  if (npc == 0) return hipGetLastError();
  const ProjWs w = project_ws(ws, n, npcp);
  hipLaunchKernelGGL(project_kernel<T>, dim3((unsigned)((n + PW - 1) / PW), (unsigned)((npcp / 16 + 3) / 4)), dim3(256),
                     0, st, x, n, B, mu, U, npc, npcp, w.P);
  hipLaunchKernelGGL((colsum_kernel<double, 0>), dim3((unsigned)nch), dim3(1024), 0, st, (const double*)w.P, n, npcp,
                     npcp, (const double*)nullptr, w.part);
  hipLaunchKernelGGL(fold_kernel, dim3(grid1(npcp)), dim3(256), 0, st, (const double*)w.part, nch, (long long)npcp, 1,
                     npcp, 0, (double)n, w.m);
  hipLaunchKernelGGL((colsum_kernel<double, 1>), dim3((unsigned)nch), dim3(1024), 0, st, (const double*)w.P, n, npcp,
                     npcp, (const double*)w.m, w.part);
  hipLaunchKernelGGL(fold_kernel, dim3(grid1(npcp)), dim3(256), 0, st, (const double*)w.part, nch, (long long)npcp, 1,
                     npcp, 0, (double)n, w.v);
  hipLaunchKernelGGL(cube_kernel, dim3(grid1(n * npc)), dim3(256), 0, st, (const double*)w.P, n, npc, npcp,
                     (const double*)w.m, (const double*)w.v, cube);
  return hipGetLastError();
}

}  // namespace

extern "C" {

size_t cmlpl_scene_workspace_bytes(int64_t pixels, int bands, int n_pc) {
  if (!scene_ok(CMLPL_SCENE_U16, pixels, bands, n_pc)) return 0;
  const long long nch = nchunks(pixels);
  const int Bp = pad16(bands), npcp = pad16(n_pc);
  const size_t gram = up256((size_t)nch * Bp * Bp * 8);
  const size_t proj = up256((size_t)pixels * npcp * 8) + up256((size_t)nch * npcp * 8) + 2 * up256((size_t)npcp * 8);
  return gram > proj ? gram : proj;
}

int cmlpl_scene_gram(const void* d_raw, int dtype, int64_t pixels, int bands, double* d_mean, double* d_gram,
                     void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_raw || !d_mean || !d_gram || !d_workspace) return CMLPL_E_ARG;
  if (!scene_ok(dtype, pixels, bands, 0)) return CMLPL_E_SHAPE;
  if (cmlpl_scene_workspace_bytes(pixels, bands, 0) > workspace_bytes) return CMLPL_E_WORKSPACE;
  double* part = (double*)d_workspace;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CMLPL_SCENE_U16: return chk(gram_run((const uint16_t*)d_raw, pixels, bands, d_mean, d_gram, part, st));
    case CMLPL_SCENE_I16: return chk(gram_run((const int16_t*)d_raw, pixels, bands, d_mean, d_gram, part, st));
    case CMLPL_SCENE_F32: return chk(gram_run((const float*)d_raw, pixels, bands, d_mean, d_gram, part, st));
    default: return chk(gram_run((const double*)d_raw, pixels, bands, d_mean, d_gram, part, st));
  }
}

int cmlpl_scene_project(const void* d_raw, int dtype, int64_t pixels, int bands, const double* d_mean,
                        const double* d_gram, const double* d_basis, int n_pc, float* d_cube, double* d_spectra,
                        void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_raw || !d_mean || !d_gram || !d_basis || !d_cube || !d_workspace || n_pc < 1) return CMLPL_E_ARG;
  if (!scene_ok(dtype, pixels, bands, n_pc)) return CMLPL_E_SHAPE;
  if (cmlpl_scene_workspace_bytes(pixels, bands, n_pc) > workspace_bytes) return CMLPL_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  switch (dtype) {
    case CMLPL_SCENE_U16:
      return chk(project_run((const uint16_t*)d_raw, pixels, bands, d_mean, d_gram, d_basis, n_pc, d_cube, d_spectra,
                             d_workspace, st));
    case CMLPL_SCENE_I16:
      return chk(project_run((const int16_t*)d_raw, pixels, bands, d_mean, d_gram, d_basis, n_pc, d_cube, d_spectra,
                             d_workspace, st));
    case CMLPL_SCENE_F32:
      return chk(project_run((const float*)d_raw, pixels, bands, d_mean, d_gram, d_basis, n_pc, d_cube, d_spectra,
                             d_workspace, st));
    default:
      return chk(project_run((const double*)d_raw, pixels, bands, d_mean, d_gram, d_basis, n_pc, d_cube, d_spectra,
                             d_workspace, st));
  }
}

}  // extern "C"
