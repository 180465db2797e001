// The loss block of the cross-pseudo-supervision baseline (reference trian_CPS.py:234-258) in ONE launch:
//   labelled row   : cls = CE(z, Y);  dz = (softmax(z) - onehot(Y)) / bt                               (:234-235)
//   unlabelled row : t_s = argmax z_w, t_w = argmax z_s (torch.max: first maximum, a NaN is the maximum and the first
//                    NaN wins, :238-239);  con_s = mean CE(z_s, t_s), con_w = mean CE(z_w, t_w)         (:241-244)
//                    dz_s = w (softmax(z_s) - onehot(t_s)) / btu, dz_w likewise                         (:245,248)
//   acc            : share of labelled rows network 1 (Base1) gets right                               (:258)
// No memory bank, no threshold, no contrastive term, no gradient into the embedding.
//
// One wavefront per batch row, lanes = classes (K <= 64), both networks' rows in the same lanes (two independent
// latency chains), four rows per workgroup -- the shape of loss_rows_kernel.  The per-row losses go to a small table;
// the workgroup that arrives LAST (an integer ticket: exact, whatever the arrival order) folds the table in a fixed
// order -- thread t takes rows t, t + 256, ...; lanes, then waves 0..3 -- so the logged scalars are the same bytes on
// every run and under graph replay.  No float atomics.  The ticket word is zeroed by a 4-byte memset in front of the
// launch (launch_cps_loss; a memset node of a captured step).
#include "common.hpp"
#include "kernels.hpp"

namespace cmlpl {

namespace {

enum { CPS_CLS_S = 0, CPS_CLS_W, CPS_ACC, CPS_CON_S, CPS_CON_W, CPS_AGREE, CPS_ROWS };

__device__ __forceinline__ int cps_label(const long long* labels, RowSel sel, int r) {
  return (int)labels[rowsel_index(sel, true, r)];
}

// torch.max(z, 1)[1] of the row held one class per lane: first index of the maximum; a NaN counts as the maximum and
// the first NaN wins (mx = wave_max over the valid lanes, which skips NaN)
__device__ __forceinline__ int cps_argmax(float z, float mx, bool kv) {
  const unsigned long long nanb = __ballot(kv && z != z);
  const unsigned long long bal = nanb ? nanb : __ballot(kv && z == mx);
  return __ffsll((long long)bal) - 1;
}

__global__ __launch_bounds__(256) void cps_loss_kernel(CpsArgs a) {
  __shared__ float red[4 * CPS_ROWS];
  __shared__ int slast;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int bt = a.bt, btu = a.btu, K = a.K, n = bt + btu;
  const int RL = bt > btu ? bt : btu;
  const int idx = blockIdx.x * 4 + wave;
  const bool kv = lane < K;
  const float NEG = -3.0e38f;
  if (idx < n) {
    const float zs = kv ? a.logits[(long long)idx * K + lane] : NEG;               // net 0 = Base  ("s")
    const float zw = kv ? a.logits[((long long)n + idx) * K + lane] : NEG;         // net 1 = Base1 ("w")
    const float mxs = wave_max(zs), mxw = wave_max(zw);
    const float es = kv ? expf(zs - mxs) : 0.f, ew = kv ? expf(zw - mxw) : 0.f;
    const float ses = wave_sum(es), sew = wave_sum(ew);
    const float lses = mxs + logf(ses), lsew = mxw + logf(sew);
    const int ams = cps_argmax(zs, mxs, kv), amw = cps_argmax(zw, mxw, kv);
    if (idx < bt) {
      const int yl = cps_label(a.labels, a.sel, idx);
      const float zys = __shfl(zs, yl, 64), zyw = __shfl(zw, yl, 64);
      if (kv) {
        const float oh = (lane == yl) ? 1.f : 0.f;
        a.dlogits[(long long)idx * K + lane] = (es / ses - oh) / (float)bt;
        a.dlogits[((long long)n + idx) * K + lane] = (ew / sew - oh) / (float)bt;
      }
      if (lane == 0) {
        a.rowloss[CPS_CLS_S * RL + idx] = lses - zys;
        a.rowloss[CPS_CLS_W * RL + idx] = lsew - zyw;
        a.rowloss[CPS_ACC * RL + idx] = (amw == yl) ? 1.f : 0.f;
      }
    } else {
      const int i = idx - bt;
      const int ts = amw, tw = ams;              // each network learns the OTHER network's hard label (:238-242)
      const float zts = __shfl(zs, ts, 64), ztw = __shfl(zw, tw, 64);
      if (kv) {
        const float scale = a.w / (float)btu;
        a.dlogits[(long long)idx * K + lane] = scale * (es / ses - (lane == ts ? 1.f : 0.f));
        a.dlogits[((long long)n + idx) * K + lane] = scale * (ew / sew - (lane == tw ? 1.f : 0.f));
      }
      if (lane == 0) {
        a.pseudo[i] = ts;
        a.pseudo[(long long)btu + i] = tw;
        a.rowloss[CPS_CON_S * RL + i] = lses - zts;
        a.rowloss[CPS_CON_W * RL + i] = lsew - ztw;
        a.rowloss[CPS_AGREE * RL + i] = (ts == tw) ? 1.f : 0.f;
      }
    }
  }
  // publish this workgroup's rows (release at agent scope, the explicit wait keeps the ticket behind the write-back:
  // the pattern of us_apply_kernel, memobank.hip), take a ticket; the last arriver folds the table
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const int t = atomicAdd(a.ticket, 1);
    slast = (t == (int)gridDim.x - 1) ? 1 : 0;
  }
  __syncthreads();
  if (!slast) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  float v[CPS_ROWS];
#pragma unroll
  for (int q = 0; q < CPS_ROWS; ++q) {
    const int cnt = (q <= CPS_ACC) ? bt : btu;
    float s = 0.f;
    for (int i = tid; i < cnt; i += 256) s += __builtin_nontemporal_load(a.rowloss + q * RL + i);
    v[q] = wave_sum(s);
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < CPS_ROWS; ++q) red[wave * CPS_ROWS + q] = v[q];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int q = 0; q < CPS_ROWS; ++q)
      v[q] = red[q] + red[CPS_ROWS + q] + red[2 * CPS_ROWS + q] + red[3 * CPS_ROWS + q];
    const float cls_s = v[CPS_CLS_S] / bt, cls_w = v[CPS_CLS_W] / bt, acc = v[CPS_ACC] / bt;
    const float con_s = v[CPS_CON_S] / btu, con_w = v[CPS_CON_W] / btu;
    int hrow = 0;
    const cmlpl_dyn* dynr = dyn_row(a.sel.dyn);
    if (dynr != nullptr) hrow = dynr->hist_row;
    float* o = a.scalars + 16 * hrow;           // the slots of cmlpl_loss_fwd_bwd
    o[0] = 0.f;                                  // no contrastive term
    o[1] = cls_s + a.w * con_s;                  // total_loss   (trian_CPS.py:245)
    o[2] = cls_s; o[3] = con_s; o[4] = acc;
    o[5] = cls_w + a.w * con_w;                  // total_loss1  (:248)
    o[6] = cls_w; o[7] = con_w; o[8] = 0.f;
    o[9] = (float)btu; o[10] = (float)btu;       // every unlabelled row carries a loss
    o[11] = 0.f; o[12] = 0.f;
    o[13] = v[CPS_AGREE];                        // rows on which the two pseudo-labels agree
    o[14] = 0.f; o[15] = 0.f;
  }
}

}  // namespace

size_t cps_loss_ws_floats(int bt, int btu) { return (size_t)CPS_ROWS * (bt > btu ? bt : btu) + 16; }

hipError_t launch_cps_loss(const CpsArgs& a_in, float* ws, hipStream_t st) {
  CpsArgs a = a_in;
  const int RL = a.bt > a.btu ? a.bt : a.btu;
  a.rowloss = ws;
  a.ticket = (int*)(ws + (size_t)CPS_ROWS * RL);
  hipError_t e = hipMemsetAsync(a.ticket, 0, sizeof(int), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cps_loss_kernel, dim3((a.bt + a.btu + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace cmlpl
