// C-ABI entry points of the auxiliary losses (include/cmlpl.h): NT-Xent, the entropy-filtered unsupervised loss and the
// class-wise memory bank.  Argument checking and launches only, as in api.hip.
#include "api_common.hpp"

using namespace cmlpl;

extern "C" {

size_t cmlpl_ntxent_workspace_bytes(int B, int D) { return (B < 1 || D < 1) ? 0 : ntxent_ws_floats(B, D) * 4; }

int cmlpl_ntxent_fwd_bwd(const float* d_emb_i, const float* d_emb_j, int B, int D, float temperature, float* d_loss,
                         float* d_grad_i, float* d_grad_j, void* d_workspace, size_t workspace_bytes, void* stream) {
  if (!d_emb_i || !d_emb_j || !d_loss || !d_grad_i || !d_grad_j || !d_workspace || B < 1 || D < 1 ||
      !(temperature > 0.f))
    return CMLPL_E_ARG;
  NtxPlan plan;              // (a batch no route holds is refused here: nothing is launched, every output keeps its bytes)
  const bool aligned = D % 4 == 0 && (((uintptr_t)d_emb_i | (uintptr_t)d_emb_j) & 15) == 0;
  if (!plan_ntxent(B, D, aligned, &plan)) return CMLPL_E_ARG;
  if (ntxent_ws_floats(B, D) * 4 > workspace_bytes) return CMLPL_E_WORKSPACE;
  return chk(launch_ntxent(d_emb_i, d_emb_j, B, D, temperature, d_loss, d_grad_i, d_grad_j, (float*)d_workspace,
                           (hipStream_t)stream));
}

// ---- loss_helper.py
size_t cmlpl_unsup_workspace_bytes(int B) { return B < 1 ? 0 : unsup_ws_bytes(B); }

int cmlpl_unsup_loss(const float* d_predict, int64_t* d_target, const float* d_pred_teacher, int B, int K,
                     double percent, float* d_loss, float* d_dpredict, void* d_workspace, size_t workspace_bytes,
                     void* stream) {
  if (!d_predict || !d_target || !d_pred_teacher || !d_loss || !d_dpredict || !d_workspace || B < 1 || K < 1 ||
      !(percent >= 0.0 && percent <= 100.0))
    return CMLPL_E_ARG;
  if (unsup_ws_bytes(B) > workspace_bytes) return CMLPL_E_WORKSPACE;
  return chk(launch_unsup(d_predict, (long long*)d_target, d_pred_teacher, B, K, percent, d_loss, d_dpredict,
                          d_workspace, (hipStream_t)stream));
}

int cmlpl_memobank_select(const float* d_prob, const float* d_label, const float* d_low_mask, const float* d_high_mask,
                          int N, int n_labeled, int K, int32_t* d_lists, int32_t* d_counts, void* stream) {
  if (!d_prob || !d_label || !d_low_mask || !d_high_mask || !d_lists || !d_counts || N < 1 || n_labeled < 0 ||
      n_labeled > N || K < 1 || K > 1024)
    return CMLPL_E_ARG;
  return chk(launch_mb_select(d_prob, d_label, d_low_mask, d_high_mask, N, n_labeled, K, d_lists, d_counts,
                              (hipStream_t)stream));
}

int cmlpl_memobank_proto(const float* d_rep_teacher, int N, int D, int K, const int32_t* d_lists,
                         const int32_t* d_counts, float* d_proto, void* stream) {
  if (!d_rep_teacher || !d_lists || !d_counts || !d_proto || N < 1 || D < 1 || K < 1) return CMLPL_E_ARG;
  return chk(launch_mb_proto(d_rep_teacher, D, d_lists, d_counts, N, K, d_proto, (hipStream_t)stream));
}

int cmlpl_memobank_enqueue(const float* d_rep_teacher, int N, int D, int K, const int32_t* d_lists,
                           const int32_t* d_counts, float* d_bank, int32_t* d_state, const int32_t* d_capacity,
                           int capacity_stride, void* stream) {
  if (!d_rep_teacher || !d_lists || !d_counts || !d_bank || !d_state || !d_capacity || N < 1 || D < 1 || K < 1 ||
      capacity_stride < 1)
    return CMLPL_E_ARG;
  return chk(launch_mb_enqueue(d_rep_teacher, D, d_lists, d_counts, N, K, d_bank, d_state, d_capacity,
                               capacity_stride, (hipStream_t)stream));
}

int cmlpl_memobank_push(const float* d_keys, int m, int D, float* d_bank_c, int32_t* d_state_c, int capacity,
                        void* stream) {
  if ((m > 0 && !d_keys) || !d_bank_c || !d_state_c || m < 0 || D < 1 || capacity < 1) return CMLPL_E_ARG;
  return chk(launch_mb_push(d_keys, m, D, d_bank_c, d_state_c, capacity, (hipStream_t)stream));
}

int cmlpl_memobank_infonce(const float* d_rep, int N, int D, const int32_t* d_pool, int pool_rows,
                           const int64_t* d_anchor_draw, const float* d_pos, int64_t pos_qstride,
                           const float* d_bank_c, int capacity, int bank_rows, int head, const int64_t* d_neg_draw,
                           int queries, int negatives, float temperature, float scale, float* d_lossq,
                           float* d_ganchor, float* d_drep, void* stream) {
  if (!d_rep || !d_pool || !d_anchor_draw || !d_pos || !d_bank_c || !d_neg_draw || !d_lossq || !d_ganchor ||
      N < 1 || D < 1 || pool_rows < 1 || pool_rows > N || capacity < 1 || bank_rows < 1 || bank_rows > capacity ||
      head < 0 || head >= capacity || queries < 1 || negatives < 1 || negatives > 127 || !(temperature > 0.f))
    return CMLPL_E_ARG;
  return chk(launch_mb_infonce(d_rep, D, d_pool, (const long long*)d_anchor_draw, d_pos, pos_qstride, d_bank_c,
                               capacity, head, (const long long*)d_neg_draw, queries, negatives, temperature, scale,
                               d_lossq, d_ganchor, d_drep, (hipStream_t)stream));
}

int cmlpl_memobank_loss(const cmlpl_memobank_call* c, void* stream) {
  if (!c || !c->d_rep || !c->d_rep_teacher || !c->d_prob_l || !c->d_prob_u || !c->d_label_l || !c->d_label_u ||
      !c->d_low_mask || !c->d_high_mask || !c->d_bank || !c->d_state || !c->d_capacity || !c->d_lists || !c->d_counts ||
      !c->d_proto || !c->d_lossq || !c->d_ganchor || !c->d_arow || !c->d_drep || !c->d_total)
    return CMLPL_E_ARG;
  if (c->N < 1 || c->n_labeled < 0 || c->n_labeled > c->N || c->K < 1 || c->K > 1024 || c->D < 1 || c->queries < 1 ||
      c->negatives < 1 || c->negatives > 127 || c->capacity_stride < 1 || !(c->temperature > 0.f))
    return CMLPL_E_ARG;
  if ((c->d_anchor_draw == nullptr) != (c->d_neg_draw == nullptr)) return CMLPL_E_ARG;
  if (c->d_momentum && (!c->d_momentum_on || !c->d_prototype)) return CMLPL_E_ARG;
  MbPlan plan;                          // every refusal before the first launch: a refused call has touched nothing
  if (!plan_mb_onepass(c->D, c->K, c->queries, c->negatives, &plan)) return CMLPL_E_ARG;
  MbPrep p;
  p.prob_l = c->d_prob_l; p.prob_u = c->d_prob_u; p.label_l = c->d_label_l; p.label_u = c->d_label_u;
  p.low_mask = c->d_low_mask; p.high_mask = c->d_high_mask; p.rep_t = c->d_rep_teacher;
  p.N = c->N; p.Nl = c->n_labeled; p.K = c->K; p.D = c->D;
  p.lists = c->d_lists; p.counts = c->d_counts; p.proto = c->d_proto;
  p.bank = c->d_bank; p.state = c->d_state; p.caps = c->d_capacity; p.cap_stride = c->capacity_stride;
  p.keys_log = c->d_keys_log;
  MbLoss l;
  l.rep = c->d_rep; l.N = c->N; l.D = c->D; l.K = c->K; l.Q = c->queries; l.NN = c->negatives;
  l.lists = c->d_lists; l.counts = c->d_counts; l.state = c->d_state; l.proto = c->d_proto;
  l.bank = c->d_bank; l.caps = c->d_capacity; l.cap_stride = c->capacity_stride;
  l.anchor_draw = (const long long*)c->d_anchor_draw; l.neg_draw = (const long long*)c->d_neg_draw;
  l.seed = c->seed; l.call = c->call;
  l.momentum = c->d_momentum; l.momentum_on = c->d_momentum_on; l.ema = c->ema; l.prototype = c->d_prototype;
  l.temp = c->temperature;
  l.lossq = c->d_lossq; l.ganchor = c->d_ganchor; l.arow = c->d_arow; l.drep = c->d_drep; l.total = c->d_total;
  return chk(launch_mb_onepass(p, l, (hipStream_t)stream));
}

int cmlpl_memobank_sum(const float* d_v, int n, float* d_out, void* stream) {
  if (!d_v || !d_out || n < 1) return CMLPL_E_ARG;
  return chk(launch_mb_sum(d_v, n, d_out, (hipStream_t)stream));
}

}  // extern "C"
