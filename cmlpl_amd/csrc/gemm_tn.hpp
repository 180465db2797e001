// The small transposed-A GEMM block shared by several launches (dense.hip: spectral forward and weight gradients;
// loss.hip: the contrastive feature gradients + the scalar block; conv0.hip: weight-gradient reduce + GEMMs).
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace cmlpl {

// One workgroup per 32x32 output tile; the reduction index r is split over the 4 waves (each takes a
// contiguous quarter) in batches of 16 operand pairs (32 dword loads, then 16 MFMAs), and the four partial
// accumulators are folded through LDS.  These GEMMs are tiny (R = batch rows): what matters is the number of
// dependent memory round trips per wave.  The loop guarantees (gemm_tn_rows below; read from the gfx950 ISA, which
// no test holds):
//   - a batch of unsegmented B is a straight line of loads: carried row offsets, no branch and no division between
//     its first and its last load;
//   - every load of a batch is issued in front of the batch's first MFMA -- held by __builtin_amdgcn_sched_barrier(0)
//     between the phases (hipcc otherwise sinks a batch's last pair below its MFMAs: two waits per batch);
//   - two batches are requested ahead: a wave waits for memory ONCE while R <= 256 (32 pairs per wave), and once
//     more per further batch.
// Segmented B (GemmTN::b_seg_rows > 0) is decided once per block and keeps its carry loop in an instantiation of its own.
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

// ---- a wave's walk over its operand pairs t0 .. t1 - 1: pair k holds rows 2 k and 2 k + 1 of A and B (half-wave hh
// reads row 2 k + hh), sixteen pairs make a batch.  A lane's pairs that exist are k < klim; a pair past them is read at
// row 0 and zeroed by select, so a batch is issued without a branch.  SEG: B's rows lie in rank-major segments
// (GemmTN::b_seg_rows, block-uniform); one division per wave, then (segment, offset) are carried -- the walk requests
// the batches in order.
template <bool SEG>
struct GemmTNWalk {
  const float* ap; const float* bp;                    // row 0 of the lane's column of A and of B
  long long oa, ob, sa, sb;                            // the next pair's row offsets and their steps (2 lda, 2 ldb)
  int kn, klim;                                        // the next pair to request
  int seg, off, seg_rows, ldb; long long seg_stride;   // SEG
  bool iv, jv;

  __device__ __forceinline__ GemmTNWalk(const GemmTN& g, const float* ap_, const float* bp_, bool iv_, bool jv_, int hh,
                                        int t0, int t1)
      : ap(ap_), bp(bp_), oa((long long)(2 * t0 + hh) * g.lda), ob((long long)(2 * t0 + hh) * g.ldb), sa(2LL * g.lda),
        sb(2LL * g.ldb), kn(t0), seg(0), off(0), seg_rows(g.b_seg_rows), ldb(g.ldb), seg_stride(g.b_seg_stride),
        iv(iv_), jv(jv_) {
    const int rows = (g.R - hh + 1) >> 1;              // 2 k + hh < R  <=>  k < rows
    klim = t1 < rows ? t1 : rows;
    if (SEG) { const int r0 = 2 * t0 + hh; seg = r0 / seg_rows; off = r0 - seg * seg_rows; }
  }
  // the next batch's 32 loads, nothing else: no wait, no branch (SEG: its carry loop)
  __device__ __forceinline__ void request(float (&a)[GT_DEPTH], float (&b)[GT_DEPTH]) {
#pragma unroll
    for (int q = 0; q < GT_DEPTH; ++q) {
      const bool rv = kn + q < klim;
      if (SEG) {
        ob = (long long)seg * seg_stride + (long long)off * ldb;
        off += 2;
        while (off >= seg_rows) { off -= seg_rows; ++seg; }
      }
      a[q] = ap[rv ? oa : 0];
      b[q] = bp[rv ? ob : 0];
      oa += sa;
      if (!SEG) ob += sb;
      // (the offsets stay CARRIED: through the empty asm hipcc cannot rewrite them as row * ld, which it otherwise
      //  forms for all 64 loads of a trip round the loop below in front of it -- 128 registers and 64 64-bit multiplies)
      asm volatile("" : "+v"(oa), "+v"(ob));
      __builtin_amdgcn_sched_barrier(0);
    }
    kn += GT_DEPTH;
  }
  // the batch that starts at pair kb: sixteen MFMAs in the order of the pairs
  __device__ __forceinline__ void run(const float (&a)[GT_DEPTH], const float (&b)[GT_DEPTH], int kb, f32x16& acc,
                                      float& asum) const {
#pragma unroll
    for (int q = 0; q < GT_DEPTH; ++q) {
      const bool rv = kb + q < klim;
      const float x = (rv && iv) ? a[q] : 0.f, y = (rv && jv) ? b[q] : 0.f;
      asum += x;
      acc = mfma32(x, y, acc);
    }
  }
};

// The schedule of a wave (sched_barrier(0) holds it where hipcc would sink a batch's last loads below its MFMAs):
//   both first batches are requested, then whatever `tail` asks for (the update's m / v / p: consumed last, requested
//   last), then batch 0's MFMAs run -- ONE wait for memory while a wave has at most 2 GT_DEPTH pairs (R <= 256).  Past
//   that a set is requested again right behind its MFMAs and waited for one batch later.  A wave with a single batch
//   (or none) requests only that one.
template <bool SEG, class Tail>
__device__ __forceinline__ void gemm_tn_rows(const GemmTN& g, const float* ap, const float* bp, bool iv, bool jv, int hh,
                                             int t0, int t1, f32x16& acc, float& asum, Tail&& tail) {
  GemmTNWalk<SEG> w(g, ap, bp, iv, jv, hh, t0, t1);
  float a0[GT_DEPTH], b0[GT_DEPTH], a1[GT_DEPTH], b1[GT_DEPTH];
  if (t0 + GT_DEPTH >= t1) {                           // (wave-uniform, as every branch here)
    if (t0 < t1) w.request(a0, b0);
    tail();
    __builtin_amdgcn_sched_barrier(0);
    if (t0 < t1) w.run(a0, b0, t0, acc, asum);
    return;
  }
  w.request(a0, b0);
  w.request(a1, b1);
  tail();
  __builtin_amdgcn_sched_barrier(0);
  int tb = t0;
  while (tb + 2 * GT_DEPTH < t1) {                     // a batch behind the two in flight: both sets go round
    asm volatile("" : "+v"(w.klim));                   // (or hipcc keeps klim - q, q = 1 .. 31, in registers across the loop)
    w.run(a0, b0, tb, acc, asum);
    __builtin_amdgcn_sched_barrier(0);
    w.request(a0, b0);
    __builtin_amdgcn_sched_barrier(0);
    w.run(a1, b1, tb + GT_DEPTH, acc, asum);
    __builtin_amdgcn_sched_barrier(0);
    w.request(a1, b1);                                 // (no branch: if no such batch exists, 32 loads of row 0 nobody waits for)
    __builtin_amdgcn_sched_barrier(0);
    tb += 2 * GT_DEPTH;
  }
  w.run(a0, b0, tb, acc, asum);
  if (tb + GT_DEPTH < t1) w.run(a1, b1, tb + GT_DEPTH, acc, asum);
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
  // What the epilogue reads is asked for behind the operand loads of the first two batches and in front of their MFMAs
  // (consumed last, requested last): it adds no round trip of its own.  What the gfx950 ISA shows of the waits (UPD,
  // unsegmented; profiles/gemm_tile_ab.txt): the MFMAs behind the loop share their code with the loop's exit, where
  // only the 64 operand loads are outstanding, so hipcc counts the operand waits without these 13 - 17 loads --
  // vmcnt(62) .. 32 for batch 0, 31 .. 0 for batch 1.  That over-waits and is safe: batch 0's last MFMAs wait some 17
  // loads into batch 1, and batch 1's last MFMA waits for m / v / p as well, which the epilogue needs right behind it.
  // A vmcnt(62) also stands in front of these loads (64 operand loads are as many as a wave can have outstanding
  // anyway): m / v / p go out when the first operands have landed and return under the MFMAs.
  float um[4], uv[4], up[4], bm = 0.f, bv2 = 0.f, bpar = 0.f, bg = 0.f, bin = 0.f;
  long long uoff = 0, boff = 0;
  bool bias_upd = false;
  auto tail = [&]() {
    if (g.bias_in != nullptr && (UPD || wave == 0)) bin = g.bias_in[(long long)bz * g.bias_in_bstride + (jv ? j : 0)];
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
  };
  if (g.b_seg_rows > 0) gemm_tn_rows<true>(g, ap, bp, iv, jv, hh, t0, t1, acc, asum, tail);      // (block-uniform)
  else gemm_tn_rows<false>(g, ap, bp, iv, jv, hh, t0, t1, acc, asum, tail);
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
        if (g.bias_in != nullptr) v += bin;
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
        if (g.bias_in != nullptr) v += bin;
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
