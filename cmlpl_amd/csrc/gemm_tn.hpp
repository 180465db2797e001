// The small transposed-A GEMM block shared by several launches (dense.hip: spectral forward and weight gradients;
// loss.hip: the contrastive feature gradients + the scalar block; conv0.hip: weight-gradient reduce + GEMMs).
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace cmlpl {

// One workgroup per 32x32 output tile; the reduction index r is split over the 4 waves (each takes a
// contiguous quarter), every wave keeps 16 operand pairs (32 loads) in flight, and the four partial
// accumulators are folded through LDS.  These GEMMs are tiny (R = batch rows): what matters is the
// number of dependent memory round trips per wave, which this shape cuts to R/128.
constexpr int GT_DEPTH = 16;

struct GemmTN2 { GemmTN p[2]; int nblk0; };
struct GemmTNShared { __attribute__((aligned(16))) float red[3][16][64]; float ared[4][64]; };

// ---- the Adam update as the optimizer launch (optim.hip) and the fused gradient fold (conv0.hip) both run it
// ONE rounded fp32 multiply whose result the compiler may not fuse into what follows (a * b - c would otherwise become
// one fma, and x * 1.0f would no longer leave the update the bits of the plain one): the product goes through an empty
// asm, after which the update sees it as it sees a loaded value
__device__ __forceinline__ float mul_alone(float a, float b) {
  float r = a * b;
  asm volatile("" : "+v"(r));
  return r;
}

// A: AdamArgs (optim.hip) or AdamFuse (kernels.hpp) -- the six scalars of the step
// CHUNK: called from adam_conv_chunk (the elementwise part otherwise) -- it matters to the variant only
template <bool OPT, bool CHUNK, class A>
__device__ __forceinline__ float adam_update(float& mm, float& vv, float p, float g, const A& a, float coef, float keep) {
  if (OPT) {
    g = mul_alone(g, coef);                              // clip_grad_norm_: grad.mul_(coef)
    p = mul_alone(p, keep);                              // AdamW: param.mul_(1 - lr * weight_decay)
    // The plain instantiation below leaves the fusing of its products into fmas to the compiler, which has two ways to
    // fuse v's sum of two products and takes one in the chunk workgroups (the square is fused) and the other in the
    // elementwise part (the decay of v is fused).  The variant spells out the same fmas, so that coef == keep == 1.0f
    // leaves the plain step's bits (tests/test_gpu_optim.py holds the two instantiations to each other).
    mm = fmaf(a.w1, g - mm, mm);
    vv = CHUNK ? fmaf(g, a.w2 * g, vv * a.b2) : fmaf(vv, a.b2, (a.w2 * g) * g);
    const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
    return fmaf(-a.step_size, mm / denom, p);
  }

  mm = mm + a.w1 * (g - mm);                             // exp_avg.lerp_(grad, 1-beta1)
  vv = vv * a.b2 + (a.w2 * g) * g;                       // exp_avg_sq.mul_(beta2).addcmul_(g, g, 1-beta2)
  const float denom = sqrtf(vv) / a.bc2_sqrt + a.eps;
  return p - a.step_size * (mm / denom);                 // param.addcdiv_(exp_avg, denom, -step_size)
}

// UPD (the fused fold + update launch, conv0.hip): C and the bias are gradients inside the flat buffer f->gbase, and
// the parameters, m and v of the tile are updated right behind the stores of the sums (the nt == 0 block: those of the
// bias row too, with the pad floats behind it that the optimizer launch walks).  The four waves SHARE the tile's
// epilogue then -- wave w finishes accumulator rows 4 w .. 4 w + 3, wave 0's own accumulators meeting the others in LDS
// (x0, [16][64]), the same sum in the same order: one wave with sixteen updates per lane (a square root and two
// divisions each) was a 2-us tail on every tile.  These tensors have no packed copy.
template <bool UPD = false>
__device__ __forceinline__ void gemm_tn_block(const GemmTN2& t, int bid, GemmTNShared& sh, const AdamFuse* f = nullptr,
                                              float (*x0)[64] = nullptr) {
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, hh = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // linear block id -> (problem, nt, mt, batch)
  const int pi = (bid >= t.nblk0) ? 1 : 0;
  const GemmTN g = t.p[pi];
  int b = bid - (pi ? t.nblk0 : 0);
  const int NTg = (g.N + 31) >> 5, MTg = (g.M + 31) >> 5;
  const int nt = b % NTg; b /= NTg;
  const int mt = b % MTg;
  const int bz = b / MTg;
  const float* A = g.A + (long long)bz * g.a_bstride;
  const float* B = g.B + (long long)bz * g.b_bstride;
  const int i = mt * 32 + l31, j = nt * 32 + l31;
  const bool iv = i < g.M, jv = j < g.N;
  const float* ap = A + (iv ? i : 0);
  const float* bp = B + (jv ? j : 0);
  const int R = g.R;
  const int pairs = (R + 1) >> 1;
  const int ppw = (pairs + 3) >> 2;                    // pairs per wave
  const int t0 = wave * ppw, t1 = (t0 + ppw < pairs) ? t0 + ppw : pairs;
  f32x16 acc = zero16();
  float asum = 0.f;
  // UPD: every wave asks for its m / v / p in front of the operand loop (no extra round trip behind it)
  float um[4], uv[4], up[4], bm = 0.f, bv2 = 0.f, bpar = 0.f, bg = 0.f;
  long long uoff = 0, boff = 0;
  bool bias_upd = false;
  if (UPD) {
    uoff = (long long)bz * f->pstride + (g.C - f->gbase);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int row = mt * 32 + acc_row(4 * wave + rr, lane);
      const long long o = uoff + ((jv && row < g.M) ? (long long)row * g.ldc + j : 0);
      um[rr] = f->m[o]; uv[rr] = f->v[o]; up[rr] = f->params[o];
    }
    bias_upd = wave == 0 && g.bias != nullptr && nt == 0 && hh == 0 && i < ((g.M + 3) & ~3);
    if (bias_upd) {
      boff = (long long)bz * f->pstride + (g.bias - f->gbase) + i;
      bm = f->m[boff]; bv2 = f->v[boff]; bpar = f->params[boff];
      if (!iv) bg = g.bias[(long long)bz * g.bias_bstride + i];        // a pad float: its gradient is what the buffer holds
    }
  }
  for (int tb = t0; tb < t1; tb += GT_DEPTH) {
    float av[GT_DEPTH], bv[GT_DEPTH];
    // segmented B (rows spread over rank-major blocks): one division per batch, then carried (rows advance by 2)
    int seg = 0, off = 0;
    if (g.b_seg_rows > 0) { const int r0 = 2 * tb + hh; seg = r0 / g.b_seg_rows; off = r0 - seg * g.b_seg_rows; }
#pragma unroll
    for (int q = 0; q < GT_DEPTH; ++q) {
      const int r = 2 * (tb + q) + hh;
      const bool rv = (tb + q < t1) && (r < R);
      const int rc = rv ? r : 0;
      const long long bo = g.b_seg_rows > 0 ? (rv ? (long long)seg * g.b_seg_stride + (long long)off * g.ldb : 0)
                                            : (long long)rc * g.ldb;
      const float a = ap[(long long)rc * g.lda], b = bp[bo];
      av[q] = (rv && iv) ? a : 0.f;
      bv[q] = (rv && jv) ? b : 0.f;
      off += 2;
      while (g.b_seg_rows > 0 && off >= g.b_seg_rows) { off -= g.b_seg_rows; ++seg; }
    }
#pragma unroll
    for (int q = 0; q < GT_DEPTH; ++q) {
      asum += av[q];
      acc = mfma32(av[q], bv[q], acc);
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) sh.red[wave - 1][r][lane] = acc[r];
  }
  if (UPD && wave == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) x0[r][lane] = acc[r];
  }
  sh.ared[wave][lane] = asum;
  __syncthreads();
  if (UPD) {
    float* C = g.C + (long long)bz * g.c_bstride;
    if (jv) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int r = 4 * wave + rr, row = mt * 32 + acc_row(r, lane);
        float v = (((x0[r][lane] + sh.red[0][r][lane]) + sh.red[1][r][lane]) + sh.red[2][r][lane]) * g.scale;
        if (g.bias_in != nullptr) v += g.bias_in[(long long)bz * g.bias_in_bstride + j];
        if (g.relu) v = relu_nan(v);
        if (row < g.M) {
          const long long o = uoff + (long long)row * g.ldc + j;
          C[(long long)row * g.ldc + j] = v;
          const float pn = adam_update<true, false>(um[rr], uv[rr], up[rr], v, *f, 1.f, f->keep);
          f->m[o] = um[rr]; f->v[o] = uv[rr]; f->params[o] = pn;
        }
      }
    }
    if (wave == 0 && g.bias != nullptr && nt == 0) {
      float tot = (sh.ared[0][lane] + sh.ared[1][lane]) + (sh.ared[2][lane] + sh.ared[3][lane]);
      tot += __shfl_xor(tot, 32, 64);
      if (hh == 0 && iv) g.bias[(long long)bz * g.bias_bstride + i] = tot * g.scale;
      if (bias_upd) {
        const float pn = adam_update<true, false>(bm, bv2, bpar, iv ? tot * g.scale : bg, *f, 1.f, f->keep);
        f->m[boff] = bm; f->v[boff] = bv2; f->params[boff] = pn;
      }
    }
    return;
  }
  if (wave == 0) {
    float* C = g.C + (long long)bz * g.c_bstride;
    if (jv) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = mt * 32 + acc_row(r, lane);
        float v = (((acc[r] + sh.red[0][r][lane]) + sh.red[1][r][lane]) + sh.red[2][r][lane]) * g.scale;
        if (g.bias_in != nullptr) v += g.bias_in[(long long)bz * g.bias_in_bstride + j];
        if (g.relu) v = relu_nan(v);
        if (row < g.M) C[(long long)row * g.ldc + j] = v;
      }
    }
    if (g.bias != nullptr && nt == 0) {
      float tot = (sh.ared[0][lane] + sh.ared[1][lane]) + (sh.ared[2][lane] + sh.ared[3][lane]);
      tot += __shfl_xor(tot, 32, 64);
      if (hh == 0 && iv) g.bias[(long long)bz * g.bias_bstride + i] = tot * g.scale;
    }
  }
}

inline int gemm_tn_blocks(const GemmTN& g) { return ((g.M + 31) / 32) * ((g.N + 31) / 32) * g.batches; }

}  // namespace cmlpl
