// C-ABI entry points (include/cmlpl.h): argument checking, workspace carving and the launch
// sequence of one training step.  No allocation, no synchronisation, graph-capturable.
// (prediction: api_infer.hip; the auxiliary losses: api_aux.hip.)  Helpers first, in one namespace; the entry points after.
#include <vector>

#include "api_common.hpp"

using namespace cmlpl;

namespace {

inline int64_t up4(int64_t v) { return (v + 3) & ~(int64_t)3; }

void fill_layout(const Dims& d, cmlpl_layout_t* out) {
  const int64_t numel[CMLPL_NUM_TENSORS] = {
      64LL * d.C, 64, 36864, 64, 36864, 64, 1024LL * d.bands, 1024, (int64_t)d.K * d.F, d.K,
      256LL * 1024, 256, 64LL * 1024, 64, 64LL * 256, 64};
  int64_t off = 0;
  for (int i = 0; i < CMLPL_NUM_TENSORS; ++i) {
    out->param_off[i] = off;
    out->param_numel[i] = numel[i];
    off = up4(off + numel[i]);
    if (i == CMLPL_NUM_LIVE - 1) out->param_live = off;
  }
  out->param_total = off;
  out->packed_total = pack_total(d.C, d.bands);
  out->cls_in = d.F;
  out->reserved = 0;
}

// workspace of the network forward/backward (all sizes in bytes, 256-B aligned regions)
struct NetWs {
  float *a0, *p1, *p2, *y, *ynorm, *catd, *dropgen, *dy, *dp2, *dp1, *da0, *part1, *part2, *part0;
  uint8_t *m1, *m2;
  uint32_t* hstat;      // [4 kinds][2 networks][n] per-sample maxima the fused kernels leave for the two-piece weight gradient
  Wgrad3Plan w1, w2;    // the plans part1 / part2 are sized by: the reduce launch folds that many partials
  size_t bytes;
};

// which kernels a call on `nets` networks x n rows runs (kernels.hpp): computed once per entry point, read by everything below
bool make_route(const Dims& d, int nets, int n, NetRoute* r) { return route_net(d.H, d.W, d.C, d.K, nets * n, r); }

// per-net conv0 weight-gradient partials: one per sample when the fused data-gradient kernel produces them
int conv0_partials(const Dims& d, const NetRoute& r, int n) {
  return r.conv0_partials_per_sample() ? n : plan_conv0_wgrad_G(n, d.C, d.HW);
}

bool carve_net(const Dims& d, const NetRoute& r, int nets, int n, char* base, NetWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += up256(bytes); return p; };
  const size_t N = (size_t)nets * n;
  bool wpair = false;
  if (!plan_wgrad3_both(nets, n, d.H, d.W, d.H2, d.W2, true, &w->w1, &w->w2, &wpair)) return false;
  const int G0 = conv0_partials(d, r, n);
  w->a0 = (float*)take(N * d.HW * 64 * 4);
  w->p1 = (float*)take(N * d.P2 * 64 * 4);
  w->m1 = (uint8_t*)take(N * d.P2 * 64);
  w->p2 = (float*)take(N * d.P4 * 64 * 4);
  w->m2 = (uint8_t*)take(N * d.P4 * 64);
  w->y = (float*)take(N * 1024 * 4);
  w->ynorm = (float*)take(N * 4);
  w->catd = (float*)take(N * d.F * 4);
  w->dropgen = (float*)take(N * d.F * 4);
  w->dy = (float*)take(N * 1024 * 4);
  w->dp2 = (float*)take(N * d.P4 * 64 * 4);
  w->dp1 = (float*)take(N * d.P2 * 64 * 4);
  w->da0 = (float*)take(N * d.HW * 64 * 4);
  w->part1 = (float*)take((size_t)nets * w->w1.G * PART3 * 4);
  w->part2 = (float*)take((size_t)nets * w->w2.G * PART3 * 4);
  w->part0 = (float*)take((size_t)nets * G0 * (size_t)conv0_partial_size(d.C) * 4);
  w->hstat = (uint32_t*)take((size_t)4 * 2 * n * 4);
  w->bytes = off;
  return true;
}

// extra regions used only by cmlpl_train_step / cmlpl_loss_fwd_bwd
struct StepWs {
  float *xn, *sn, *dlogits, *dfeat, *probs, *loss;
  size_t bytes;
};

// (the loss region is last: no other offset depends on the banks' rows)
void carve_step(const Dims& d, int n, size_t loss_bytes, char* base, StepWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) { char* p = base ? base + off : nullptr; off += up256(bytes); return p; };
  w->xn = (float*)take((size_t)2 * n * d.C * d.HW * 4);
  w->sn = (float*)take((size_t)2 * n * d.bands * 4);
  w->dlogits = (float*)take((size_t)2 * n * d.K * 4);
  w->dfeat = (float*)take((size_t)2 * n * 1024 * 4);
  w->probs = (float*)take((size_t)4 * n * d.K * 4);
  w->loss = (float*)take(loss_bytes);
  w->bytes = off;
}

// The step context: what the shape and the row count of a call decide.  An entry point opens it once -- ctx_shape in front
// of its argument checks, ctx_carve behind them (both refusals are CMLPL_E_SHAPE) -- and everything below it reads it.
struct StepCtx {
  Dims d; cmlpl_layout_t L;
  int nets, n; NetRoute r; NetWs nw;
  StepWs sw;              // behind the networks' regions (a call on the networks alone reads none of it)
  size_t loss_bytes;      // of sw.loss: the loss block of n rows against banks of bank_rows rows (at least n)
};
bool ctx_shape(const cmlpl_shape* shape, StepCtx* c) {
  if (!make_dims(shape, &c->d)) return false;
  fill_layout(c->d, &c->L);
  return true;
}
bool ctx_carve(StepCtx* c, int nets, int n, int bank_rows, void* base) {
  c->nets = nets; c->n = n;
  if (!make_route(c->d, nets, n, &c->r) || !carve_net(c->d, c->r, nets, n, (char*)base, &c->nw)) return false;
  c->loss_bytes = loss_ws_floats(n, n, n, c->d.K, bank_rows > n ? bank_rows : n) * 4;
  carve_step(c->d, n, c->loss_bytes, base ? (char*)base + c->nw.bytes : nullptr, &c->sw);
  return true;
}

PackInfo make_pack_info(const Dims& d, const cmlpl_layout_t& L) {
  PackInfo pi;
  pi.stride = L.packed_total; pi.off_w0 = L.param_off[0]; pi.off_w1 = L.param_off[2]; pi.off_w2 = L.param_off[4];
  pi.off_ws = L.param_off[6]; pi.C = d.C; pi.bands = d.bands;
  return pi;
}

// ---- optional per-kernel timing (cmlpl_timing_begin/_end): hipEvent pairs recorded on the launch stream
// around the selected launches.  Off by default; the only process-global state of the library.
struct Timing {
  bool on = false;
  uint32_t mask = 0;
  std::vector<hipEvent_t> ev;
  std::vector<int> ids;
  size_t used = 0;
} g_timing;

template <class F>
int timed(int id, hipStream_t st, F f) {
  Timing& t = g_timing;
  if (t.on && ((t.mask >> id) & 1u) && t.used + 2 <= t.ev.size()) {
    (void)hipEventRecord(t.ev[t.used], st);
    const int rc = f();
    (void)hipEventRecord(t.ev[t.used + 1], st);
    t.ids.push_back(id);
    t.used += 2;
    return rc;
  }
  return f();
}
#define TIMED(id, expr) timed((id), st, [&]() -> int { return (expr); })

// the keys of a call's rows in the noise and dropout streams: a shard's global ones, or those of a batch of bt labelled rows
struct RowKeys { int lab0, unl_base; };
RowKeys row_keys(const cmlpl_shard* sh, int bt) { return {sh ? sh->lab0 : 0, sh ? sh->bt_g + sh->unl0 : bt}; }

// patch rows that are already augmented: [nets][n][C*HW]
XSrc xsrc_plain(const float* d_xn, int nets, int n, long long per, uint64_t seed, uint64_t step,
                const cmlpl_shard* sh, DynRef dyn = DynRef()) {
  XSrc x = XSrc();
  x.sel.dyn = dyn;
  const int nlab = sh ? sh->nlab : n;
  for (int i = 0; i < 2; ++i) {
    x.lab[i] = d_xn + (long long)(i < nets ? i : 0) * n * per;
    x.unl[i] = x.lab[i] + (long long)nlab * per;
  }
  x.nlab = nlab; x.sigma = 0.f;
  const RowKeys k = row_keys(sh, n);                              // keys of the dropout stream
  x.lab0 = k.lab0; x.unl_base = k.unl_base;
  x.seed = seed; x.step = step;
  return x;
}
// raw labelled / unlabelled rows + noise formed in the kernels
RowSel batch_sel(const cmlpl_batch* b, DynRef dyn) {
  RowSel s = RowSel();
  s.lab_idx = (const long long*)b->d_lab_idx; s.unl_idx = (const long long*)b->d_unl_idx; s.dyn = dyn;
  return s;
}
XSrc xsrc_raw(const cmlpl_batch* b, float sigma, uint64_t seed, uint64_t step, const cmlpl_shard* sh,
              DynRef dyn = DynRef()) {
  XSrc x = XSrc();
  x.sel = batch_sel(b, dyn);
  for (int i = 0; i < 2; ++i) {
    x.lab[i] = b->d_xpl; x.unl[i] = b->d_xpu;
    x.nz_lab[i] = b->noise8 ? b->noise8[2 * i] : nullptr;          // reference draw order, see cmlpl_augment
    x.nz_unl[i] = b->noise8 ? b->noise8[4 + 2 * i] : nullptr;
  }
  x.sigma = sigma; x.nlab = b->bt; x.philox = b->noise8 == nullptr;
  const RowKeys k = row_keys(sh, b->bt);
  x.lab0 = k.lab0; x.unl_base = k.unl_base;
  x.seed = seed; x.step = step;
  return x;
}

// What fwd_core runs on.  Call sites value-initialise the record and fill it by name: a field left out is null / zero.
struct FwdCall {
  const float *params, *packed; int64_t param_stride;   // canonical weights [nets][param_stride], packed sets [nets][L.packed_total]
  XSrc xs; const float *xn, *sn;       // the patch rows; pre-augmented rows, for the unfused conv0 / spectral kernels
  const XSrc* xspec; float* sn_out; const long long* labels; float* labels_f;   // raw spectra for the fused spectral kernel + what it also writes; or null
  const float* dropmask; float dropout_p; int train; uint64_t seed, step; const cmlpl_shard* shard;
  float *logits, *feat, *xn_save;      // outputs; xn_save: where the fused kernels leave the rows they saw, or null
  // parts: bit 0 = the spectral branch (feat_spe + ReLU; with early_feat also the L2 normalisation -> feat, ynorm),
  //        bit 1 = the convolution stack + head (-> logits; feat / ynorm too unless early_feat)
  int parts = 3; bool early_feat;
};
int fwd_core(const StepCtx& c, hipStream_t st, const FwdCall& f) {
  const Dims& d = c.d;
  const NetRoute& r = c.r;
  const cmlpl_layout_t& L = c.L;
  const NetWs& w = c.nw;
  const int nets = c.nets, n = c.n;
  int rc;
  const long long pk_ns = L.packed_total;
  float* d_feat = f.feat;
  if (f.parts & 1) {  // spectral branch (feat_spe + ReLU)
    if (f.xspec != nullptr) {
      // raw spectra: augmentation + GEMM + bias + ReLU in one launch (also writes the augmented rows for the
      // weight gradient)
      if ((rc = TIMED(CMLPL_K_SPE_FWD, chk(launch_spe_fused(nets, n, d.bands, *f.xspec, f.params + L.param_off[6],
                                   f.params + L.param_off[7], f.param_stride, w.y, f.sn_out, f.labels, f.labels_f,
                                   f.xspec->nlab, st))))) return rc;
    } else {
      // pre-augmented spectra (the nn.Module path): y = relu(sn . W^T + b) from the canonical weight
      if ((rc = TIMED(CMLPL_K_SPE_FWD, chk(launch_spe_fwd(nets, n, d.bands, f.sn, f.params + L.param_off[6],
                                   f.params + L.param_off[7], f.param_stride, w.y, st))))) return rc;
    }
    // the embeddings right here (they depend on nothing the convolutions compute, tools/models.py:142-146)
    // (timed with the spectral branch it belongs to)
    if (f.early_feat && (rc = TIMED(CMLPL_K_SPE_FWD, chk(launch_feat_norm(nets, n, w.y, w.ynorm, d_feat, (long long)n * 1024, st)))))
      return rc;
  }
  if (!(f.parts & 2)) return 0;
  if (f.early_feat) d_feat = nullptr;           // the head skips its own normalisation
  if (f.shard && f.shard->nlab + f.shard->nunl != n) return CMLPL_E_ARG;
  if (r.fwd == ROUTE_A) {
    // the whole spatial forward + head of a sample in one workgroup: conv0 + conv1 + pool + conv2 + pool + flatten /
    // concat / dropout / classifier / L2-norm.  Needs the spectral branch output (launched above, same stream).
    FwdTail t;
    t.w2f = f.packed + pack_off_b3(d.C, d.bands, 2); t.w2f_ns = pk_ns; t.b2 = f.params + L.param_off[5];
    t.wc = f.params + L.param_off[8]; t.bc = f.params + L.param_off[9]; t.p_ns = f.param_stride;
    t.y = w.y; t.dropmask = f.dropmask; t.dropgen = w.dropgen; t.catd = w.catd; t.ynorm = w.ynorm;
    t.logits = f.logits; t.feat = d_feat; t.p2 = w.p2; t.m2 = w.m2; t.dropout_p = f.dropout_p; t.train = f.train; t.K = d.K;
    t.w1h = f.packed + pack_off_h2(d.C, d.bands, 0); t.w1h_ns = pk_ns; t.h2flag = (const uint32_t*)(f.packed + pack_off_h2flag(d.C, d.bands));
    // every sample's largest |a0| / |p1| (this launch) and gradient operands (the backward's), for the two-piece
    // weight-gradient launch of the same step
    if (r.stats) t.hstat = w.hstat;
    return TIMED(CMLPL_K_CONV1_FWD, chk(launch_conv3_fused(r, nets, n, d.C, d.H, d.W, f.xs, f.packed + pack_off_w0b3(d.C, d.bands),
                               pk_ns, f.params + L.param_off[1], f.param_stride, w.a0, f.packed + pack_off_b3(d.C, d.bands, 0), pk_ns,
                               f.params + L.param_off[3], f.param_stride, w.p1, w.m1, &t, st, f.xn_save)));
  }
  // the general 3x3 launches on two fp16 pieces where their plans allow; when all four of a step do, each leaves its
  // samples' image maxima for the two-piece weight gradient (NetRoute::stats)
  const uint32_t* h2flag = (const uint32_t*)(f.packed + pack_off_h2flag(d.C, d.bands));
  uint32_t* const hstat = r.stats ? w.hstat : nullptr;
  if (r.fwd == ROUTE_B) {
    // conv0 + conv1 in one launch, input rows taken where they lie and augmented in LDS: neither an augmented
    // copy of the input nor a0's round trip between the two convolutions touches HBM (a0 is still written once,
    // for the backward pass)
    if ((rc = TIMED(CMLPL_K_CONV1_FWD, chk(launch_conv3_fused(r, nets, n, d.C, d.H, d.W, f.xs, f.packed + pack_off_w0b3(d.C, d.bands),
                               pk_ns, f.params + L.param_off[1], f.param_stride, w.a0, f.packed + pack_off_b3(d.C, d.bands, 0), pk_ns,
                               f.params + L.param_off[3], f.param_stride, w.p1, w.m1, nullptr, st, f.xn_save))))) return rc;
  } else {
    if (conv0a_ok(d.C, d.HW) && (f.xn == nullptr || f.xs.sigma == 0.f)) {
      // the general path: augmentation + conv0 in ONE launch on the split-bf16 MFMA, from the rows `xs` names (raw rows
      // with their noise -> the augmented rows also go to xn_save for the backward; or a caller's pre-augmented tensor)
      if ((rc = TIMED(CMLPL_K_CONV0_FWD, chk(launch_conv0a_fwd(nets, n, d.C, d.HW, f.xs, f.packed + pack_off_w0b3(d.C, d.bands), pk_ns,
                                     f.params + L.param_off[1], f.param_stride, w.a0, f.xn_save, st))))) return rc;
    } else {
      if (!f.xn) return CMLPL_E_ARG;
      if ((rc = TIMED(CMLPL_K_CONV0_FWD, chk(launch_conv0_fwd(nets, n, d.C, d.HW, f.xn, f.packed + pack_off_w0t(), pk_ns,
                                     f.params + L.param_off[1], f.param_stride, w.a0, st))))) return rc;
    }
    const Conv3H2 h1 = {f.packed + pack_off_h2(d.C, d.bands, 0), pk_ns, h2flag, hstat, 0};
    if ((rc = TIMED(CMLPL_K_CONV1_FWD, chk(launch_conv3(r.plan[0], 0, nets, n, d.H, d.W, w.a0, nullptr, f.packed + pack_off_b3(d.C, d.bands, 0),
                               pk_ns, f.params + L.param_off[3], f.param_stride, w.p1, w.m1, st, h1))))) return rc;
  }
  const Conv3H2 h2 = {f.packed + pack_off_h2(d.C, d.bands, 2), pk_ns, h2flag, hstat, 1};
  if ((rc = TIMED(CMLPL_K_CONV2_FWD, chk(launch_conv3(r.plan[2], 0, nets, n, d.H2, d.W2, w.p1, nullptr, f.packed + pack_off_b3(d.C, d.bands, 2),
                             pk_ns, f.params + L.param_off[5], f.param_stride, w.p2, w.m2, st, h2))))) return rc;
  const RowKeys k = row_keys(f.shard, n);
  return TIMED(CMLPL_K_HEAD_FWD, chk(launch_head_fwd(nets, n, d.P4, d.K, w.p2, w.y, f.dropmask, w.dropgen, f.dropout_p,
                             f.train, f.seed, f.step, f.shard ? f.shard->nlab : n, k.lab0, k.unl_base, f.params + L.param_off[8],
                             f.params + L.param_off[9], f.param_stride, w.catd, w.ynorm, f.logits, d_feat, st,
                             f.xs.sel.dyn)));
}

// What bwd_core runs on; filled like FwdCall.
struct BwdCall {
  const float *params, *packed; int64_t param_stride;
  XSrc xs; const float *xn, *sn;       // the rows the forward saw: for the fused data gradient / for the unfused conv0 and feat_spe weight gradients
  const float* dropmask; float dropout_p; int train;
  const float *dlogits, *dfeat; float* grads; int64_t grad_stride;   // grads: output [nets][grad_stride]
  int* dyn_cursor; cmlpl_dyn* dyn_table;   // graph replay: the reduce launch advances the cursor of dyn_table; or both null
  // parts: bit 0 = the data-gradient chain + the 3x3 weight-gradient partials (needs dlogits; dfeat only when parts == 3),
  //        bit 1 = partial reduction + classifier / feat_spe weight gradients (parts == 2: dy first takes its dfeat part)
  int parts = 3; const AdamFuse* fuse;     // fuse: the Adam step rides in the reduce launch (parts == 3, no cursor)
};
int bwd_core(const StepCtx& c, hipStream_t st, const BwdCall& b) {
  const Dims& d = c.d;
  const NetRoute& r = c.r;
  const cmlpl_layout_t& L = c.L;
  const NetWs& w = c.nw;
  const int nets = c.nets, n = c.n;
  const float* mask = (!b.train || b.dropout_p <= 0.f) ? nullptr : (b.dropmask ? b.dropmask : w.dropgen);
  int rc;
  uint32_t* const hstat = r.stats ? w.hstat : nullptr;
  const uint32_t* h2flag = (const uint32_t*)(b.packed + pack_off_h2flag(d.C, d.bands));
  // in two parts the head runs WITHOUT the feature gradients (dy is linear in them; launch_dy_fixup adds their share
  // in front of the feat_spe weight-gradient GEMM, bit-identically)
  const float* d_dfeat_head = (b.parts == 3) ? b.dfeat : nullptr;
  GemmTN gw_cls, gw_spe;
  {
    GemmTN& g = gw_cls;
    g.bias_in = nullptr; g.bias_in_bstride = 0; g.relu = 0;
    // dW_cls[k][f] = sum_n dlogits[n][k] * catd[n][f] ; db_cls[k] = sum_n dlogits[n][k]
    g.A = b.dlogits; g.a_bstride = (long long)n * d.K; g.lda = d.K; g.M = d.K;
    g.B = w.catd; g.b_bstride = (long long)n * d.F; g.ldb = d.F; g.N = d.F;
    g.C = b.grads + L.param_off[8]; g.c_bstride = b.grad_stride; g.ldc = d.F;
    g.bias = b.grads + L.param_off[9]; g.bias_bstride = b.grad_stride;
    g.R = n; g.batches = nets; g.scale = 1.f;
    // dW_spe[o][b] = sum_n dy[n][o] * sn[n][b] ; db_spe[o] = sum_n dy[n][o]   (same launch)
    GemmTN& h = gw_spe;
    h = g;
    h.A = w.dy; h.a_bstride = (long long)n * 1024; h.lda = 1024; h.M = 1024;
    h.B = b.sn; h.b_bstride = (long long)n * d.bands; h.ldb = d.bands; h.N = d.bands;
    h.C = b.grads + L.param_off[6]; h.ldc = d.bands;
    h.bias = b.grads + L.param_off[7];
  }
  if (b.parts & 1) {
    if (r.bwd == ROUTE_A) {
      // ONE per-sample launch for the whole data-gradient chain: head backward -> conv2 data gradient -> conv1 data
      // gradient -> conv0 weight-gradient partial.  dp2 / dp1 / dy still go to HBM for the weight-gradient kernels
      // that follow; da0 and the pooled-gradient hand-offs stay on chip.
      BwdHead hd;
      hd.dlogits = b.dlogits; hd.dfeat = d_dfeat_head; hd.mask = mask; hd.wc = b.params + L.param_off[8]; hd.p_ns = b.param_stride;
      hd.y = w.y; hd.ynorm = w.ynorm; hd.m2 = w.m2; hd.w2d = b.packed + pack_off_b3(d.C, d.bands, 3); hd.w2d_ns = L.packed_total;
      hd.dy = w.dy; hd.dp2 = w.dp2; hd.dp1 = w.dp1; hd.K = d.K;
      hd.w1h = b.packed + pack_off_h2(d.C, d.bands, 1); hd.w1h_ns = L.packed_total;
      hd.h2flag = h2flag; hd.hstat = hstat;
      if ((rc = TIMED(CMLPL_K_CONV1_DGRAD, chk(launch_conv3_fused_bwd(r, nets, n, d.C, d.H, d.W, w.dp1, w.m1,
                                 b.packed + pack_off_b3(d.C, d.bands, 1), L.packed_total, b.xs, w.part0,
                                 (long long)n * conv0_partial_size(d.C), &hd, st))))) return rc;
    } else {
      // General path (windows the per-sample kernels do not take: P 20x20, B5 15x15): one launch per stage.  Round 4:
      // both 3x3 weight gradients in ONE launch here too (the pair kernel, placed behind conv2's data gradient, which
      // produces conv1's pooled gradient), and the classifier / feat_spe weight-gradient GEMMs ride in the reduce launch --
      // 17 launches where there were 19; the forked side streams of round 1 are gone (they never paid: DESIGN.md section 7).
      // feat is re-formed inside head_bwd as y / ||y|| (the forward's own division), so it is not an input here
      if ((rc = TIMED(CMLPL_K_HEAD_BWD, chk(launch_head_bwd(nets, n, d.P4, d.K, b.dlogits, d_dfeat_head, mask,
                                    b.params + L.param_off[8], b.param_stride, w.y, w.ynorm, w.dy, w.dp2, st))))) return rc;
      const Conv3H2 h3 = {b.packed + pack_off_h2(d.C, d.bands, 3), L.packed_total, h2flag, hstat, 3};
      if ((rc = TIMED(CMLPL_K_CONV2_DGRAD, chk(launch_conv3(r.plan[3], 1, nets, n, d.H2, d.W2, w.dp2, w.m2, b.packed + pack_off_b3(d.C, d.bands, 3),
                                 L.packed_total, nullptr, 0, w.dp1, nullptr, st, h3))))) return rc;
      // (round 6: conv1's data gradient in FRONT of the weight-gradient pair launch -- it leaves the maxima of conv1's
      //  gradient operand that the two-piece weight gradient scales by; neither reads what the other writes)
      if (r.bwd == ROUTE_B) {
        // conv1 data gradient + conv0 weight gradient in one launch: da0 never goes to HBM
        if ((rc = TIMED(CMLPL_K_CONV1_DGRAD, chk(launch_conv3_fused_bwd(r, nets, n, d.C, d.H, d.W, w.dp1, w.m1,
                                   b.packed + pack_off_b3(d.C, d.bands, 1), L.packed_total, b.xs, w.part0,
                                   (long long)n * conv0_partial_size(d.C), nullptr, st))))) return rc;
      } else {
        if (!b.xn) return CMLPL_E_ARG;
        const Conv3H2 h1 = {b.packed + pack_off_h2(d.C, d.bands, 1), L.packed_total, h2flag, hstat, 2};
        if ((rc = TIMED(CMLPL_K_CONV1_DGRAD, chk(launch_conv3(r.plan[1], 1, nets, n, d.H, d.W, w.dp1, w.m1, b.packed + pack_off_b3(d.C, d.bands, 1),
                                   L.packed_total, nullptr, 0, w.da0, nullptr, st, h1))))) return rc;
        if ((rc = TIMED(CMLPL_K_CONV0_WGRAD, chk(launch_conv0_wgrad(nets, n, d.C, d.HW, b.xn, w.da0, w.part0, st, hstat, h2flag,
                                                                           L.packed_total)))))
          return rc;
      }
    }
    // conv1's and conv2's weight gradients, on every path: one launch where the pair kernel exists (timed as the conv1
    // kernel; the launcher reports which it was, nothing here depends on it)
    bool merged;
    if ((rc = TIMED(CMLPL_K_CONV1_WGRAD, chk(launch_wgrad3_pair(nets, n, d.H, d.W, w.a0, w.dp1, w.m1, w.part1, d.H2, d.W2,
                                  w.p1, w.dp2, w.m2, w.part2, &merged, st, hstat, h2flag, L.packed_total))))) return rc;
  }
  if (!(b.parts & 2)) return 0;
  if (b.parts == 2) {
    if (!b.dfeat) return CMLPL_E_ARG;
    if ((rc = TIMED(CMLPL_K_HEAD_BWD, chk(launch_dy_fixup(nets, n, w.y, w.ynorm, b.dfeat, w.dy, st))))) return rc;
  }
  // one launch folds the per-workgroup partials of all three convolutions into the flat gradient
  ReduceTable rt;
  rt.count = 0; rt.total_blocks = 0; rt.grad_ns = b.grad_stride; rt.dyn_cursor = b.dyn_cursor; rt.dyn_table = b.dyn_table;
  if (b.fuse != nullptr && (b.parts != 3 || b.dyn_cursor != nullptr || b.fuse->gbase != b.grads)) return CMLPL_E_ARG;
  const bool fused = b.fuse != nullptr;                   // block widths of the fused launch (kernels.hpp: reduce_el)
  reduce_table_add(rt, w.part1, w.w1.G, PART3, 1, 64, b.grads + L.param_off[2], b.grads + L.param_off[3], fused);
  reduce_table_add(rt, w.part2, w.w2.G, PART3, 1, 64, b.grads + L.param_off[4], b.grads + L.param_off[5], fused);
  reduce_table_add(rt, w.part0, conv0_partials(d, r, n), conv0_partial_size(d.C), 0, d.C,
                   b.grads + L.param_off[0], b.grads + L.param_off[1], fused);
  // the classifier / feat_spe weight-gradient GEMMs ride along (independent, short); with `fuse` so does the Adam step
  // of every gradient element this launch forms -- all ten live tensors
  return TIMED(CMLPL_K_CONV1_WRED, chk(launch_reduce_gemm(nets, rt, gw_cls, gw_spe, st, b.fuse)));
}

// 0, or the error of a malformed batch.  Split-fed (d_cube null): the four row buffers.  Cube-fed (ABI 6): the scene, its
// two pixel lists and NO window buffers; a square window no larger than the scene that fits the gather's LDS tile.
int check_batch(const Dims& d, const cmlpl_batch* b) {
  if (!b || b->bt < 1 || b->btu < 1 || !b->d_xl || !b->d_xu) return CMLPL_E_ARG;
  if (b->d_cube == nullptr) return (b->d_xpl && b->d_xpu) ? 0 : CMLPL_E_ARG;
  if (b->d_xpl || b->d_xpu || !b->d_lab_pix || !b->d_unl_pix || b->cube_rows < 1 || b->cube_cols < 1) return CMLPL_E_ARG;
  if (d.H != d.W || b->cube_rows < d.H || b->cube_cols < d.W || cube_feed_lds(d.C, d.W) > LDS_MAX) return CMLPL_E_SHAPE;
  return 0;
}

// One forward or backward pass of the step's two networks over a batch (cmlpl_forward* / cmlpl_backward*, the stages of
// the sharded step, and the two halves of cmlpl_train_step): the arguments those entry points share, then each side's own.
struct PassCall {
  const cmlpl_hparams* hp; const cmlpl_batch* batch; const cmlpl_shard* shard;
  const float *params, *packed, *dropmask; int train; uint64_t seed, step;
  void* workspace; size_t workspace_bytes; DynRef dyn;
  int parts = 3;                                        // as fwd_core's / bwd_core's
  float *logits, *feat, *labels_f; int sym_mode;        // forward: outputs, spatial augmentation of cube-fed rows
  const float *dlogits, *dfeat; float* grads; int64_t grad_stride; int* dyn_cursor; const AdamFuse* fuse;   // backward
};
PassCall pass_call(const cmlpl_hparams* hp, const cmlpl_batch* batch, const cmlpl_shard* shard, const float* d_params,
                   const float* d_packed, const float* d_dropmask, int train, uint64_t seed, uint64_t step,
                   void* d_workspace, size_t workspace_bytes) {
  PassCall p = PassCall();
  p.hp = hp; p.batch = batch; p.shard = shard; p.params = d_params; p.packed = d_packed; p.dropmask = d_dropmask;
  p.train = train; p.seed = seed; p.step = step; p.workspace = d_workspace; p.workspace_bytes = workspace_bytes;
  return p;
}

int check_forward(const Dims& d, const PassCall& p) {
  if (!p.hp || !p.params || !p.workspace || ((p.parts & 2) && (!p.packed || !p.logits)) || ((p.parts & 1) && !p.feat))
    return CMLPL_E_ARG;                // (the spatial part alone writes no embeddings: the spectral part has formed them)
  if (int brc = check_batch(d, p.batch)) return brc;
  if (p.labels_f && !p.batch->d_labels) return CMLPL_E_ARG;
  if (p.hp->dropout_p < 0.f || p.hp->dropout_p >= 1.f) return CMLPL_E_ARG;
  if (p.shard && (p.shard->nlab != p.batch->bt || p.shard->nunl != p.batch->btu)) return CMLPL_E_ARG;
  return 0;
}
int forward_impl(const StepCtx& c, hipStream_t st, const PassCall& p) {
  const Dims& d = c.d;
  const NetRoute& r = c.r;
  const StepWs& sw = c.sw;
  const cmlpl_batch* batch = p.batch;
  const int parts = p.parts;
  // does the step need an augmented copy of the patches in HBM?  (only when a conv0 pass falls back to the unfused kernels)
  const bool copy = r.xn_copy();
  const RowKeys k = row_keys(p.shard, batch->bt);
  int rc;
  // the augmentation launch remains only for what the fused kernels cannot take raw: the patches when a conv0 pass
  // falls back to the unfused kernels, the spectra when the fused spectral kernel does not apply, and the label
  // conversion for the data-parallel exchange buffer
  const bool spe_fused = spe_fused_ok(d.bands);
  // (general path: the augmentation of the patches rides in conv0's launch where conv0a_fwd_kernel takes the window; it
  //  leaves the augmented rows in sw.xn like the fused forward does)
  const bool c0a = r.fwd == ROUTE_C && conv0a_ok(d.C, d.HW);
  // (cube-fed batch: the patches' augmented rows come from the gather launch below, whatever the path)
  const bool cube = batch->d_cube != nullptr;
  const int which = ((parts & 2) && copy && !c0a && !cube ? 1 : 0) | ((parts & 1) && !spe_fused ? 2 : 0);
  float* const d_labels_f = (parts & 1) ? p.labels_f : nullptr;     // (the labels travel with the spectral part)
  const RowSel sel = batch_sel(batch, p.dyn);
  if (which &&
      (rc = TIMED(CMLPL_K_AUGMENT, chk(launch_augment(which, 2, batch->bt, batch->btu, d.C * d.HW, d.bands, k.lab0,
                                k.unl_base, batch->d_xpl, batch->d_xl, batch->d_xpu, batch->d_xu, batch->noise8,
                                p.hp->noise_sigma, p.seed, p.step, sw.xn, sw.sn, nullptr, st,
                                (const long long*)batch->d_labels, d_labels_f, &sel))))) return rc;
  XSrc xspec = xsrc_raw(batch, p.hp->noise_sigma, p.seed, p.step, p.shard, p.dyn);
  for (int i = 0; i < 2; ++i) {       // the spectral rows and their draws (reference order, see cmlpl_augment)
    xspec.lab[i] = batch->d_xl; xspec.unl[i] = batch->d_xu;
    xspec.nz_lab[i] = batch->noise8 ? batch->noise8[2 * i + 1] : nullptr;
    xspec.nz_unl[i] = batch->noise8 ? batch->noise8[4 + 2 * i + 1] : nullptr;
  }
  FwdCall f = FwdCall();
  f.params = p.params; f.param_stride = c.L.param_total; f.packed = p.packed;
  f.xspec = spe_fused ? &xspec : nullptr; f.sn_out = sw.sn; f.labels = (const long long*)batch->d_labels; f.labels_f = d_labels_f;
  f.sn = sw.sn; f.dropmask = p.dropmask; f.dropout_p = p.hp->dropout_p; f.train = p.train; f.seed = p.seed; f.step = p.step;
  f.shard = p.shard; f.logits = p.logits; f.feat = p.feat; f.parts = parts;
  f.early_feat = parts != 3;          // in two parts (the sharded step) the spectral part forms the embeddings itself
  if (cube) {
    // the windows are gathered from the scene and augmented into sw.xn -- the rows the backward reads -- and the forward
    // runs on them as plain rows by batch row (no noise, no index lists: both are spent) without writing them again
    if ((parts & 2) &&
        (rc = TIMED(CMLPL_K_CUBE_FEED, chk(launch_cube_feed(batch->d_cube, batch->cube_rows, batch->cube_cols, d.C, d.W,
                                  (const long long*)batch->d_lab_pix, (const long long*)batch->d_unl_pix, batch->bt,
                                  batch->btu, k.lab0, k.unl_base, batch->noise8, p.hp->noise_sigma, p.seed, p.step, sw.xn, &sel,
                                  st, p.sym_mode))))) return rc;
    f.xs = xsrc_plain(sw.xn, 2, c.n, (long long)d.C * d.HW, p.seed, p.step, p.shard, p.dyn);
    f.xn = sw.xn;
  } else {
    // (fused per-sample kernels: the forward leaves the rows it saw in sw.xn for cmlpl_backward, which lands them by DMA)
    f.xs = xsrc_raw(batch, p.hp->noise_sigma, p.seed, p.step, p.shard, p.dyn);
    f.xn = (copy && !c0a) ? sw.xn : nullptr;
    f.xn_save = (!copy || c0a) ? sw.xn : nullptr;
  }
  return fwd_core(c, st, f);
}

int check_backward(const Dims& d, const PassCall& p) {
  if (!p.hp || !p.params || !p.packed || !p.dlogits || ((p.parts & 2) && !p.grads) || !p.workspace) return CMLPL_E_ARG;
  return check_batch(d, p.batch);
}
int backward_impl(const StepCtx& c, hipStream_t st, const PassCall& p) {
  const StepWs& sw = c.sw;
  BwdCall b = BwdCall();
  b.params = p.params; b.param_stride = c.L.param_total; b.packed = p.packed;
  // the patches as the forward saw them: sw.xn holds them in [nets][n][C*HW] layout either way -- written by the fused
  // forward (augmented, or plain copies when no noise is added) or, when a conv0 pass fell back to the unfused kernels
  // (`xn_copy`), by the augmentation launch.  The fused data gradient reads plain rows by batch row: it knows neither noise
  // nor index lists, so it must never be handed the raw batch (a 9x9 window at 128 + 128 rows plans an unfused forward
  // and a fused backward: with the raw rows conv0's weight gradient came from un-augmented rows 0..n-1 of the split).
  b.xs = xsrc_plain(sw.xn, 2, c.n, (long long)c.d.C * c.d.HW, p.seed, p.step, p.shard, p.dyn);
  b.xn = c.r.xn_copy() ? sw.xn : nullptr; b.sn = sw.sn;
  b.dropmask = p.dropmask; b.dropout_p = p.hp->dropout_p; b.train = p.train;
  b.dlogits = p.dlogits; b.dfeat = p.dfeat; b.grads = p.grads; b.grad_stride = p.grad_stride;
  b.dyn_cursor = p.dyn_cursor; b.dyn_table = p.dyn_cursor ? (cmlpl_dyn*)p.dyn.table : nullptr;
  b.parts = p.parts; b.fuse = p.fuse;
  return bwd_core(c, st, b);
}
// a pass called alone: its own checks, the carving for its batch, and the workspace up to the loss block's inputs (the
// whole step needs all of it)
int pass_alone(StepCtx& c, const PassCall& p, bool backward, void* stream) {
  if (int rc = backward ? check_backward(c.d, p) : check_forward(c.d, p)) return rc;
  if (!ctx_carve(&c, 2, p.batch->bt + p.batch->btu, 0, p.workspace)) return CMLPL_E_SHAPE;
  if (c.nw.bytes + (size_t)((char*)c.sw.dlogits - (char*)c.sw.xn) > p.workspace_bytes) return CMLPL_E_WORKSPACE;
  return backward ? backward_impl(c, (hipStream_t)stream, p) : forward_impl(c, (hipStream_t)stream, p);
}
int pass_entry(const cmlpl_shape* shape, const PassCall& p, bool backward, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  return pass_alone(c, p, backward, stream);
}

int fill_loss_args(const Dims& d, const cmlpl_shard* sh, const float* d_logits, const float* d_feat,
                   const int64_t* d_labels, const cmlpl_banks* banks, int smooth, float adap_mask,
                   const cmlpl_hparams* hp, void* ws, size_t ws_bytes, LossArgs* out,
                   const cmlpl_gathered* gth = nullptr, const RowSel* sel = nullptr) {
  if (!sh || !banks || !hp || !ws) return CMLPL_E_ARG;
  if (gth == nullptr && (!d_logits || !d_feat || !d_labels)) return CMLPL_E_ARG;
  if (gth != nullptr && (!gth->d_recv_feat || !gth->d_logits_local || gth->world < 1 || gth->bt_local < 1 || gth->btu_local < 1 ||
                         gth->world * gth->bt_local != sh->bt_g || gth->world * gth->btu_local != sh->btu_g ||
                         sh->nunl != gth->btu_local || sh->unl0 % gth->btu_local != 0 ||
                         (sh->nlab != 0 && (sh->nlab != gth->bt_local || sh->lab0 % gth->bt_local != 0))))
    return CMLPL_E_ARG;
  if (sh->bt_g < 1 || sh->btu_g < 1 || sh->btu_g > 2048 || sh->nlab < 0 || sh->nunl < 1 || sh->lab0 < 0 ||
      sh->unl0 < 0 || sh->lab0 + sh->nlab > sh->bt_g || sh->unl0 + sh->nunl > sh->btu_g)
    return CMLPL_E_ARG;
  if (banks->Q < sh->bt_g + sh->btu_g || !banks->d_feats[0] || !banks->d_feats[1] || !banks->d_probs[0] ||
      !banks->d_probs[1])
    return CMLPL_E_ARG;
  if (loss_ws_floats(sh->nlab, sh->nunl, sh->btu_g, d.K, banks->Q) * 4 > ws_bytes) return CMLPL_E_WORKSPACE;
  LossArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = d_logits; a.feat = d_feat; a.labels = d_labels;
  if (sel != nullptr) a.sel = *sel;
  if (gth != nullptr) {
    const long long n_l = gth->bt_local + gth->btu_local;
    a.recv_f = gth->d_recv_feat; a.bt_l = gth->bt_local; a.btu_l = gth->btu_local;
    a.pack_f = 2 * n_l * 1024 + gth->bt_local;
    a.logits_loc = gth->d_logits_local;
  }
  for (int i = 0; i < 2; ++i) {
    a.bank_f[i] = banks->d_feats[i]; a.bank_p[i] = banks->d_probs[i];
    a.bank_fw[i] = banks->d_feats[i]; a.bank_pw[i] = banks->d_probs[i];
  }
  a.Q = banks->Q; a.ptr0 = ((banks->ptr[0] % a.Q) + a.Q) % a.Q; a.ptr1 = ((banks->ptr[1] % a.Q) + a.Q) % a.Q;
  a.bt = sh->bt_g; a.btu = sh->btu_g; a.K = d.K; a.smooth = smooth;
  a.lab0 = sh->lab0; a.nlab = sh->nlab; a.unl0 = sh->unl0; a.nunl = sh->nunl;
  a.adap_mask = adap_mask; a.T = hp->temperature; a.alpha = hp->alpha;
  a.w_contrast = hp->w_contrast; a.w_mutual = hp->w_mutual; a.pos_thr = hp->pos_thr; a.neg_thr = hp->neg_thr;
  loss_ws_carve(a, (float*)ws);
  *out = a;
  return 0;
}
// The two phases of the loss block on filled arguments: check the phase's outputs, set them, launch.
int loss_phase1_run(LossArgs& a, float* d_dlogits, float* d_dfeat, float* d_probs_local, hipStream_t st) {
  if (!d_dlogits || !d_dfeat || !d_probs_local) return CMLPL_E_ARG;
  a.dlogits = d_dlogits; a.dfeat = d_dfeat; a.probs_l = d_probs_local;
  return TIMED(CMLPL_K_LOSS, chk(launch_loss_phase1(a, st)));
}
int loss_phase2_run(LossArgs& a, const float* d_probs_global, int probs_shard_rows, float* d_scalars, float* d_dfeat,
                    float* d_dfeat_w_partial, hipStream_t st) {
  if (!d_probs_global || !d_scalars || !d_dfeat || !d_dfeat_w_partial || probs_shard_rows < 1 ||
      a.btu % probs_shard_rows != 0)
    return CMLPL_E_ARG;
  a.probs_g = d_probs_global; a.pshard = probs_shard_rows; a.scalars = d_scalars; a.dfeat = d_dfeat;
  a.dfw_part = d_dfeat_w_partial;
  if (int rc = TIMED(CMLPL_K_LOSS2, chk(launch_loss_graph(a, st)))) return rc;
  // the two feature-gradient GEMMs + the scalar block (the bank write went with phase 1's row kernel)
  return TIMED(CMLPL_K_LOSS_DFEAT, chk(launch_loss_dfeat(a, st)));
}
// the whole loss block on one GPU (both phases back to back); sel: labels by index / device-side step scalars
int loss_both(const Dims& d, int bt, int btu, const float* d_logits, const float* d_feat,
              const int64_t* d_labels, const cmlpl_banks* banks, int smooth, float adap_mask,
              const cmlpl_hparams* hp, float* d_scalars, float* d_dlogits, float* d_dfeat,
              float* d_probs, void* d_workspace, size_t workspace_bytes, hipStream_t st, const RowSel* sel) {
  if (!d_probs || !d_dfeat || !d_dlogits || !d_scalars) return CMLPL_E_ARG;
  const cmlpl_shard sh = {bt, btu, 0, bt, 0, btu};
  LossArgs a;
  int rc = fill_loss_args(d, &sh, d_logits, d_feat, d_labels, banks, smooth, adap_mask, hp, d_workspace,
                          workspace_bytes, &a, nullptr, sel);
  if (rc) return rc;
  // one GPU: the probabilities are already global, and the column-side gradient goes straight to dfeat[1]
  // (phase 1's launches carry phase 2's fields as well: one argument block serves the whole loss)
  float* const dfw = d_dfeat + ((size_t)(bt + btu) + bt) * 1024;
  a.probs_g = d_probs; a.pshard = btu; a.scalars = d_scalars; a.dfw_part = dfw;
  if ((rc = loss_phase1_run(a, d_dlogits, d_dfeat, d_probs, st))) return rc;
  return loss_phase2_run(a, d_probs, btu, d_scalars, d_dfeat, dfw, st);
}

// the CPS loss block (cps_loss.hip); sel: labels by index / device-side logging row
int cps_loss_impl(const Dims& d, int bt, int btu, const float* d_logits, const int64_t* d_labels,
                  const cmlpl_hparams* hp, float* d_scalars, float* d_dlogits, int64_t* d_pseudo, void* d_workspace,
                  size_t workspace_bytes, hipStream_t st, const RowSel* sel) {
  if (bt < 1 || btu < 1 || !d_logits || !d_labels || !hp || !d_scalars || !d_dlogits || !d_pseudo || !d_workspace)
    return CMLPL_E_ARG;
  if (cps_loss_ws_floats(bt, btu) * 4 > workspace_bytes) return CMLPL_E_WORKSPACE;
  CpsArgs a;
  memset(&a, 0, sizeof(a));
  a.logits = d_logits; a.labels = (const long long*)d_labels;
  if (sel != nullptr) a.sel = *sel;
  a.bt = bt; a.btu = btu; a.K = d.K; a.w = hp->w_mutual;
  a.dlogits = d_dlogits; a.scalars = d_scalars; a.pseudo = (long long*)d_pseudo;
  return TIMED(CMLPL_K_CPS_LOSS, chk(launch_cps_loss(a, (float*)d_workspace, st)));
}

// the options of a step: 0, or CMLPL_E_ARG (include/cmlpl.h, cmlpl_optim)
bool optim_norm_wanted(const cmlpl_optim* opt) { return opt->max_norm > 0.f || opt->d_norms != nullptr; }
int check_optim(const cmlpl_optim* opt) {
  if (!(opt->max_norm >= 0.f && opt->max_norm <= 3.0e38f) || !(opt->weight_decay >= 0.f && opt->weight_decay <= 3.0e38f))
    return CMLPL_E_ARG;                                                   // (a NaN fails both comparisons)
  if (((uintptr_t)opt->d_norms & 3) || ((uintptr_t)opt->d_partials & 7)) return CMLPL_E_ARG;
  if (optim_norm_wanted(opt) && opt->d_partials == nullptr) return CMLPL_E_ARG;
  return 0;
}
int grad_norm_launch(const cmlpl_layout_t& L, int nets, const float* d_grads, int64_t grad_stride, void* d_partials,
                     hipStream_t st) {
  long long off[CMLPL_NUM_LIVE], numel[CMLPL_NUM_LIVE];
  for (int t = 0; t < CMLPL_NUM_LIVE; ++t) { off[t] = L.param_off[t]; numel[t] = L.param_numel[t]; }
  return chk(launch_grad_norm(nets, d_grads, grad_stride, off, numel, (double*)d_partials, st));
}
int adam_impl(const Dims& d, const cmlpl_layout_t& L, int nets, float* d_params, int64_t param_stride,
              const float* d_grads, int64_t grad_stride, float* d_m, float* d_v, int64_t t,
              const cmlpl_hparams* hp, float* d_packed, hipStream_t st, DynRef dyn, const cmlpl_optim* opt = nullptr) {
  int rc;
  if (nets < 1 || nets > 2 || !d_params || !d_grads || !d_m || !d_v || !hp || t < 1) return CMLPL_E_ARG;
  if (opt == nullptr)
    return TIMED(CMLPL_K_ADAM, chk(launch_adam(nets, d_params, param_stride, d_grads, grad_stride, d_m, d_v,
                              L.param_live, t, hp->lr, hp->beta1, hp->beta2, hp->eps, d_packed,
                              make_pack_info(d, L), st, dyn)));
  if ((rc = check_optim(opt))) return rc;
  AdamOpt o;
  o.partials = nullptr; o.norms = opt->d_norms; o.max_norm = opt->max_norm; o.keep = adam_keep(hp->lr, opt->weight_decay);
  if (o.keep == 0.f) return CMLPL_E_ARG;                      // (its bits would read "no decay" in a table row)
  const bool wanted = optim_norm_wanted(opt);
  if (wanted) o.partials = (const double*)opt->d_partials;
  if (grad_stride < L.param_total) return CMLPL_E_ARG;
  auto both = [&]() -> int {                                  // the partials, then the update that folds them
    if (wanted)
      if (int r = grad_norm_launch(L, nets, d_grads, grad_stride, opt->d_partials, st)) return r;
    return chk(launch_adam(nets, d_params, param_stride, d_grads, grad_stride, d_m, d_v, L.param_live, t, hp->lr,
                           hp->beta1, hp->beta2, hp->eps, d_packed, make_pack_info(d, L), st, dyn, &o));
  };
  return TIMED(CMLPL_K_ADAM, both());
}
// the norms row without an update: the partials, then their fold
int grad_norm_impl(const cmlpl_layout_t& L, int nets, const float* d_grads, int64_t grad_stride, float max_norm,
                   void* d_partials, float* d_norms, hipStream_t st, DynRef dyn) {
  if (nets < 1 || nets > 2 || !d_grads || !d_partials || !d_norms || grad_stride < L.param_total ||
      !(max_norm >= 0.f && max_norm <= 3.0e38f) || ((uintptr_t)d_partials & 7) || ((uintptr_t)d_norms & 3))
    return CMLPL_E_ARG;
  if (int rc = grad_norm_launch(L, nets, d_grads, grad_stride, d_partials, st)) return rc;
  return chk(launch_grad_norm_fin(nets, (const double*)d_partials, max_norm, d_norms, st, dyn));
}

// one stage of the sharded step, every per-step scalar from the device table (see cmlpl_dist_io)
int dist_stage_run(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_dist_io* io, int stage, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  const DynRef dyn = {io->d_dyn_table, io->d_dyn_cursor};
  PassCall p = pass_call(hp, &io->batch, &io->shard, io->d_params, io->d_packed, nullptr, 1, io->seed, 0, io->d_workspace,
                         io->workspace_bytes);
  p.dyn = dyn;
  LossArgs a;
  auto fill_loss = [&]() -> int {
    RowSel sel = RowSel();
    sel.dyn = dyn;
    return fill_loss_args(c.d, &io->shard, nullptr, nullptr, nullptr, &io->banks, 1, 0.f, hp, io->d_loss_workspace,
                          io->loss_workspace_bytes, &a, &io->gathered, &sel);
  };
  switch (stage) {
    case CMLPL_STAGE_SPECTRAL:
      p.feat = io->d_feat_l; p.labels_f = io->d_labels_f; p.parts = 1;
      return pass_alone(c, p, false, stream);
    case CMLPL_STAGE_SPATIAL:
      p.logits = io->d_logits_l; p.parts = 2;
      return pass_alone(c, p, false, stream);
    case CMLPL_STAGE_PHASE1:
      if (int rc = fill_loss()) return rc;
      return loss_phase1_run(a, io->d_dlogits, io->d_dfeat, io->d_probs_l, st);
    case CMLPL_STAGE_PHASE2:
      if (int rc = fill_loss()) return rc;
      return loss_phase2_run(a, io->d_probs_g, io->probs_shard_rows, io->d_scalars, io->d_dfeat, io->d_dfeat_w_partial, st);
    case CMLPL_STAGE_BACKWARD_DATA:
      p.dlogits = io->d_dlogits; p.parts = 1;
      return pass_alone(c, p, true, stream);
    case CMLPL_STAGE_BACKWARD_WEIGHTS:      // (the reduce launch of this part advances the table's cursor)
      p.dlogits = io->d_dlogits; p.dfeat = io->d_dfeat; p.grads = io->d_grads; p.grad_stride = io->grad_stride;
      p.dyn_cursor = io->d_dyn_cursor; p.parts = 2;
      return pass_alone(c, p, true, stream);
    case CMLPL_STAGE_UPDATE:
      return adam_impl(c.d, c.L, 2, io->d_params, c.L.param_total, io->d_grads, io->grad_stride, io->d_m, io->d_v, 1, hp,
                       io->d_packed, st, dyn);
    default:
      return CMLPL_E_ARG;
  }
}

// ---- a launch sequence as a replayable hipGraph: what `enqueue` puts on the stream, captured and instantiated
struct StepGraph { hipGraph_t graph; hipGraphExec_t exec; };

template <class F>
int capture_graph(hipStream_t st, F enqueue, void** graph_out) {
  if (g_timing.on) return CMLPL_E_ARG;                     // (event pairs are not part of the product's graph)
  hipError_t e = loss_prepare_capture();
  if (e != hipSuccess) return (int)e;
  e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return (int)e;
  const int rc = enqueue();
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(st, &g);                          // always end the capture, also after a failed launch
  if (rc != 0) { if (g) (void)hipGraphDestroy(g); return rc; }   // (the sequence's own error before the capture's)
  if (e != hipSuccess) return (int)e;
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  if (e != hipSuccess) { (void)hipGraphDestroy(g); return (int)e; }
  *graph_out = new StepGraph{g, ex};
  return 0;
}

}  // namespace

extern "C" {

int cmlpl_abi_version(void) { return CMLPL_ABI_VERSION; }

// hash of the kernel sources + C header this binary was built from (cmlpl_amd/build_ext.py passes it; the marker lets
// the build script read it from the file without loading the library): the Python binding refuses a stale binary
#ifndef CMLPL_SOURCE_HASH
#define CMLPL_SOURCE_HASH "unknown"
#endif
const char* cmlpl_source_hash(void) {
  static const char marked[] = "CMLPL_SOURCE_HASH=" CMLPL_SOURCE_HASH;
  return marked + sizeof("CMLPL_SOURCE_HASH=") - 1;
}

int cmlpl_layout(const cmlpl_shape* shape, cmlpl_layout_t* out) {
  Dims d;
  if (!out) return CMLPL_E_ARG;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  fill_layout(d, out);
  return 0;
}

int cmlpl_packed_flag_offset(const cmlpl_shape* shape, int64_t* off_floats) {
  Dims d;
  if (!off_floats) return CMLPL_E_ARG;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  *off_floats = pack_off_h2flag(d.C, d.bands);
  return 0;
}

size_t cmlpl_workspace_bytes(const cmlpl_shape* shape, int nets, int n, int bank_rows) {
  StepCtx c;
  if (!ctx_shape(shape, &c) || nets < 1 || nets > 2 || n < 1 || !ctx_carve(&c, nets, n, bank_rows, nullptr)) return 0;
  return c.nw.bytes + c.sw.bytes + 256;
}

int cmlpl_pack_weights(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                       float* d_packed, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  if (!d_params || !d_packed || nets < 1 || nets > 2) return CMLPL_E_ARG;
  return chk(launch_pack_weights(nets, d_params, param_stride, make_pack_info(c.d, c.L), d_packed, (hipStream_t)stream));
}

int cmlpl_augment(const cmlpl_shape* shape, int nets, int bt, int btu, const float* d_xpl, const float* d_xl,
                  const float* d_xpu, const float* d_xu, const float* const* noise8, float sigma, uint64_t seed,
                  uint64_t step, const cmlpl_shard* shard, float* d_xn, float* d_sn, float* d_snT, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || bt < 0 || btu < 0 || bt + btu < 1 || !d_xn || !d_sn) return CMLPL_E_ARG;
  if ((bt > 0 && (!d_xpl || !d_xl)) || (btu > 0 && (!d_xpu || !d_xu))) return CMLPL_E_ARG;
  if (shard && (shard->nlab != bt || shard->nunl != btu)) return CMLPL_E_ARG;
  const RowKeys k = row_keys(shard, bt);
  hipStream_t st = (hipStream_t)stream;
  return TIMED(CMLPL_K_AUGMENT, chk(launch_augment(3, nets, bt, btu, d.C * d.HW, d.bands, k.lab0, k.unl_base, d_xpl, d_xl,
                            d_xpu, d_xu, noise8, sigma, seed, step, d_xn, d_sn, d_snT, st)));
}

int cmlpl_basenet2_fwd(const cmlpl_shape* shape, int nets, int n, const float* d_params, int64_t param_stride,
                       const float* d_packed, const float* d_xn, const float* d_sn, const float* d_snT,
                       const float* d_dropmask, float dropout_p, int train, uint64_t seed, uint64_t step,
                       const cmlpl_shard* shard,
                       float* d_logits, float* d_feat, void* d_workspace, size_t workspace_bytes, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || !d_params || !d_packed || !d_xn || !d_sn || !d_logits || !d_feat ||
      !d_workspace)
    return CMLPL_E_ARG;
  if (dropout_p < 0.f || dropout_p >= 1.f) return CMLPL_E_ARG;
  if (!ctx_carve(&c, nets, n, 0, d_workspace)) return CMLPL_E_SHAPE;
  if (c.nw.bytes > workspace_bytes) return CMLPL_E_WORKSPACE;
  FwdCall f = FwdCall();
  f.params = d_params; f.param_stride = param_stride; f.packed = d_packed;
  f.xs = xsrc_plain(d_xn, nets, n, (long long)c.d.C * c.d.HW, seed, step, shard);
  f.xn = d_xn; f.sn = d_sn;
  f.dropmask = d_dropmask; f.dropout_p = dropout_p; f.train = train; f.seed = seed; f.step = step; f.shard = shard;
  f.logits = d_logits; f.feat = d_feat;
  return fwd_core(c, (hipStream_t)stream, f);
}

int cmlpl_basenet2_bwd(const cmlpl_shape* shape, int nets, int n, const float* d_params, int64_t param_stride,
                       const float* d_packed, const float* d_xn, const float* d_sn, const float* d_dropmask,
                       float dropout_p, int train, const float* d_dlogits, const float* d_dfeat, float* d_grads,
                       int64_t grad_stride, void* d_workspace, size_t workspace_bytes, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || !d_params || !d_packed || !d_xn || !d_sn || !d_dlogits || !d_grads ||
      !d_workspace)
    return CMLPL_E_ARG;
  if (!ctx_carve(&c, nets, n, 0, d_workspace)) return CMLPL_E_SHAPE;
  if (c.nw.bytes > workspace_bytes) return CMLPL_E_WORKSPACE;
  BwdCall b = BwdCall();
  b.params = d_params; b.param_stride = param_stride; b.packed = d_packed;
  b.xs = xsrc_plain(d_xn, nets, n, (long long)c.d.C * c.d.HW, 0, 0, nullptr);
  b.xn = d_xn; b.sn = d_sn;
  b.dropmask = d_dropmask; b.dropout_p = dropout_p; b.train = train;
  b.dlogits = d_dlogits; b.dfeat = d_dfeat; b.grads = d_grads; b.grad_stride = grad_stride;
  return bwd_core(c, (hipStream_t)stream, b);
}

int cmlpl_forward_spectral(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                           const cmlpl_shard* shard, const float* d_params, uint64_t seed, uint64_t step, float* d_feat,
                           float* d_labels_f, void* d_workspace, size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, nullptr, nullptr, 1, seed, step, d_workspace, workspace_bytes);
  p.feat = d_feat; p.labels_f = d_labels_f; p.parts = 1;
  return pass_entry(shape, p, false, stream);
}
int cmlpl_forward_spatial(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                          const cmlpl_shard* shard, const float* d_params, const float* d_packed, const float* d_dropmask,
                          int train, uint64_t seed, uint64_t step, float* d_logits, void* d_workspace,
                          size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, d_packed, d_dropmask, train, seed, step, d_workspace, workspace_bytes);
  p.logits = d_logits; p.parts = 2;
  return pass_entry(shape, p, false, stream);
}
int cmlpl_forward(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch, const cmlpl_shard* shard,
                  const float* d_params, const float* d_packed, const float* d_dropmask, int train, uint64_t seed,
                  uint64_t step, float* d_logits, float* d_feat, float* d_labels_f, void* d_workspace,
                  size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, d_packed, d_dropmask, train, seed, step, d_workspace, workspace_bytes);
  p.logits = d_logits; p.feat = d_feat; p.labels_f = d_labels_f;
  return pass_entry(shape, p, false, stream);
}

int cmlpl_backward_data(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch, const cmlpl_shard* shard,
                        const float* d_params, const float* d_packed, const float* d_dropmask, int train, uint64_t seed,
                        uint64_t step, const float* d_dlogits, void* d_workspace, size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, d_packed, d_dropmask, train, seed, step, d_workspace, workspace_bytes);
  p.dlogits = d_dlogits; p.parts = 1;
  return pass_entry(shape, p, true, stream);
}
int cmlpl_backward_weights(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                           const cmlpl_shard* shard, const float* d_params, const float* d_packed, const float* d_dropmask,
                           int train, uint64_t seed, uint64_t step, const float* d_dlogits, const float* d_dfeat,
                           float* d_grads, int64_t grad_stride, void* d_workspace, size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, d_packed, d_dropmask, train, seed, step, d_workspace, workspace_bytes);
  p.dlogits = d_dlogits; p.dfeat = d_dfeat; p.grads = d_grads; p.grad_stride = grad_stride; p.parts = 2;
  return pass_entry(shape, p, true, stream);
}
int cmlpl_backward(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch, const cmlpl_shard* shard,
                   const float* d_params, const float* d_packed, const float* d_dropmask, int train, uint64_t seed,
                   uint64_t step, const float* d_dlogits, const float* d_dfeat, float* d_grads, int64_t grad_stride,
                   void* d_workspace, size_t workspace_bytes, void* stream) {
  PassCall p = pass_call(hp, batch, shard, d_params, d_packed, d_dropmask, train, seed, step, d_workspace, workspace_bytes);
  p.dlogits = d_dlogits; p.dfeat = d_dfeat; p.grads = d_grads; p.grad_stride = grad_stride;
  return pass_entry(shape, p, true, stream);
}

size_t cmlpl_loss_workspace_bytes(const cmlpl_shape* shape, const cmlpl_shard* shard, int bank_rows) {
  Dims d;
  if (!make_dims(shape, &d) || !shard || shard->nunl < 1 || shard->btu_g < 1 || bank_rows < 1) return 0;
  return loss_ws_floats(shard->nlab, shard->nunl, shard->btu_g, d.K, bank_rows) * 4;
}

int cmlpl_loss_phase1(const cmlpl_shape* shape, const cmlpl_shard* shard, const float* d_logits, const float* d_feat,
                      const int64_t* d_labels, const cmlpl_banks* banks, int smooth, float adap_mask,
                      const cmlpl_hparams* hp, float* d_dlogits, float* d_dfeat, float* d_probs_local,
                      void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  LossArgs a;
  if (int rc = fill_loss_args(d, shard, d_logits, d_feat, d_labels, banks, smooth, adap_mask, hp, d_workspace,
                              workspace_bytes, &a)) return rc;
  return loss_phase1_run(a, d_dlogits, d_dfeat, d_probs_local, (hipStream_t)stream);
}

int cmlpl_loss_phase2(const cmlpl_shape* shape, const cmlpl_shard* shard, const float* d_logits, const float* d_feat,
                      const int64_t* d_labels, const cmlpl_banks* banks, int smooth, float adap_mask,
                      const cmlpl_hparams* hp, const float* d_probs_global, int probs_shard_rows, float* d_scalars,
                      float* d_dfeat, float* d_dfeat_w_partial, void* d_workspace, size_t workspace_bytes,
                      void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  LossArgs a;
  if (int rc = fill_loss_args(d, shard, d_logits, d_feat, d_labels, banks, smooth, adap_mask, hp, d_workspace,
                              workspace_bytes, &a)) return rc;
  return loss_phase2_run(a, d_probs_global, probs_shard_rows, d_scalars, d_dfeat, d_dfeat_w_partial, (hipStream_t)stream);
}

int cmlpl_loss_phase1_g(const cmlpl_shape* shape, const cmlpl_shard* shard, const cmlpl_gathered* gathered,
                        const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                        float* d_dlogits, float* d_dfeat, float* d_probs_local, void* d_workspace,
                        size_t workspace_bytes, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (!gathered) return CMLPL_E_ARG;
  LossArgs a;
  if (int rc = fill_loss_args(d, shard, nullptr, nullptr, nullptr, banks, smooth, adap_mask, hp, d_workspace,
                              workspace_bytes, &a, gathered)) return rc;
  return loss_phase1_run(a, d_dlogits, d_dfeat, d_probs_local, (hipStream_t)stream);
}

int cmlpl_loss_phase2_g(const cmlpl_shape* shape, const cmlpl_shard* shard, const cmlpl_gathered* gathered,
                        const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                        const float* d_probs_global, int probs_shard_rows, float* d_scalars, float* d_dfeat,
                        float* d_dfeat_w_partial, void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (!gathered) return CMLPL_E_ARG;
  LossArgs a;
  if (int rc = fill_loss_args(d, shard, nullptr, nullptr, nullptr, banks, smooth, adap_mask, hp, d_workspace,
                              workspace_bytes, &a, gathered)) return rc;
  return loss_phase2_run(a, d_probs_global, probs_shard_rows, d_scalars, d_dfeat, d_dfeat_w_partial, (hipStream_t)stream);
}

int cmlpl_loss_fwd_bwd(const cmlpl_shape* shape, int bt, int btu, const float* d_logits, const float* d_feat,
                       const int64_t* d_labels, const cmlpl_banks* banks, int smooth, float adap_mask,
                       const cmlpl_hparams* hp, float* d_scalars, float* d_dlogits, float* d_dfeat,
                       float* d_probs, void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  return loss_both(d, bt, btu, d_logits, d_feat, d_labels, banks, smooth, adap_mask, hp, d_scalars, d_dlogits,
                   d_dfeat, d_probs, d_workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

size_t cmlpl_cps_loss_workspace_bytes(const cmlpl_shape* shape, int bt, int btu) {
  Dims d;
  if (!make_dims(shape, &d) || bt < 1 || btu < 1) return 0;
  return cps_loss_ws_floats(bt, btu) * 4;
}
int cmlpl_cps_loss_fwd_bwd(const cmlpl_shape* shape, int bt, int btu, const float* d_logits, const int64_t* d_labels,
                           const cmlpl_hparams* hp, float* d_scalars, float* d_dlogits, int64_t* d_pseudo,
                           void* d_workspace, size_t workspace_bytes, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  return cps_loss_impl(d, bt, btu, d_logits, d_labels, hp, d_scalars, d_dlogits, d_pseudo, d_workspace,
                       workspace_bytes, (hipStream_t)stream, nullptr);
}

int cmlpl_dist_unpack(const cmlpl_shape* shape, int world, int bt_local, int btu_local, const float* d_gathered_feat,
                      const float* d_gathered_logits, float* d_logits_g, float* d_feat_g, int64_t* d_labels_g, void* stream) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (world < 1 || bt_local < 1 || btu_local < 1 || !d_gathered_feat || !d_gathered_logits || !d_logits_g || !d_feat_g ||
      !d_labels_g)
    return CMLPL_E_ARG;
  return chk(launch_dist_unpack(d_gathered_feat, d_gathered_logits, world, bt_local, btu_local, d.K, d_logits_g, d_feat_g,
                                (long long*)d_labels_g, (hipStream_t)stream));
}

int cmlpl_dyn_adam(const cmlpl_hparams* hp, int64_t adam_t, float* step_size, float* bc2_sqrt) {
  if (!hp || adam_t < 1 || !step_size || !bc2_sqrt) return CMLPL_E_ARG;
  adam_bias_scalars(hp->lr, hp->beta1, hp->beta2, adam_t, step_size, bc2_sqrt);
  return 0;
}

int cmlpl_adam_step_opt(const cmlpl_shape* shape, int nets, float* d_params, int64_t param_stride,
                        const float* d_grads, int64_t grad_stride, float* d_m, float* d_v, int64_t t,
                        const cmlpl_hparams* hp, float* d_packed, const cmlpl_optim* opt, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  return adam_impl(c.d, c.L, nets, d_params, param_stride, d_grads, grad_stride, d_m, d_v, t, hp, d_packed, (hipStream_t)stream,
                   DynRef(), opt);
}
int cmlpl_adam_step(const cmlpl_shape* shape, int nets, float* d_params, int64_t param_stride,
                    const float* d_grads, int64_t grad_stride, float* d_m, float* d_v, int64_t t,
                    const cmlpl_hparams* hp, float* d_packed, void* stream) {
  return cmlpl_adam_step_opt(shape, nets, d_params, param_stride, d_grads, grad_stride, d_m, d_v, t, hp, d_packed, nullptr, stream);
}
size_t cmlpl_grad_norm_partials_bytes(void) { return grad_norm_partials_bytes(); }
int cmlpl_grad_norm(const cmlpl_shape* shape, int nets, const float* d_grads, int64_t grad_stride, float max_norm,
                    void* d_partials, float* d_norms, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  return grad_norm_impl(c.L, nets, d_grads, grad_stride, max_norm, d_partials, d_norms, (hipStream_t)stream, DynRef());
}
int cmlpl_dyn_adam_opt(const cmlpl_hparams* hp, int64_t adam_t, float weight_decay, float* step_size, float* bc2_sqrt,
                       float* keep) {
  if (!keep || !(weight_decay >= 0.f && weight_decay <= 3.0e38f)) return CMLPL_E_ARG;
  if (int rc = cmlpl_dyn_adam(hp, adam_t, step_size, bc2_sqrt)) return rc;
  *keep = adam_keep(hp->lr, weight_decay);
  return *keep == 0.f ? CMLPL_E_ARG : 0;
}

int cmlpl_train_step_opt(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io,
                         const cmlpl_optim* opt, void* stream) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  if (!hp || !io || io->bt < 1 || io->btu < 1 || !io->d_workspace || !io->d_params || !io->d_grads ||
      !io->d_packed || !io->d_logits || !io->d_feat || !io->d_scalars || !io->d_labels)
    return CMLPL_E_ARG;
  if (io->apply_update && (!io->d_m || !io->d_v)) return CMLPL_E_ARG;
  if (opt != nullptr) {
    if (int orc = check_optim(opt)) return orc;
    if (io->apply_update && adam_keep(hp->lr, opt->weight_decay) == 0.f) return CMLPL_E_ARG;
  }
  // reserved: bits 0..7 the method, bits 8..9 the spatial augmentation of the cube-fed rows (CMLPL_SYM_*), no other bit
  const int method = io->reserved & 0xff, sym_mode = (io->reserved >> 8) & 3;
  if ((io->reserved & ~0x3ff) != 0 || sym_mode > CMLPL_SYM_D4 ||
      (method != CMLPL_METHOD_CMLPL && method != CMLPL_METHOD_CPS))
    return CMLPL_E_ARG;
  if (sym_mode != CMLPL_SYM_NONE && io->d_cube == nullptr) return CMLPL_E_ARG;
  const bool cps = method == CMLPL_METHOD_CPS;
  // one context for the whole step: forward, loss block, backward and update read the same dims, route and carving
  if (!ctx_carve(&c, 2, io->bt + io->btu, io->banks.Q, io->d_workspace)) return CMLPL_E_SHAPE;
  if (c.nw.bytes + c.sw.bytes > io->workspace_bytes) return CMLPL_E_WORKSPACE;
  const cmlpl_layout_t& L = c.L;
  const StepWs& sw = c.sw;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((io->d_dyn_table == nullptr) != (io->d_dyn_cursor == nullptr)) return CMLPL_E_ARG;
  const DynRef dyn = {io->d_dyn_table, io->d_dyn_cursor};
  const cmlpl_shard sh = {io->bt, io->btu, 0, io->bt, 0, io->btu};
  const cmlpl_batch batch = {io->d_xpl, io->d_xl, io->d_xpu, io->d_xu, io->d_labels, io->noise8, io->bt, io->btu,
                             io->d_lab_idx, io->d_unl_idx, io->d_cube, io->cube_rows, io->cube_cols, io->d_lab_pix,
                             io->d_unl_pix};
  PassCall p = pass_call(hp, &batch, &sh, io->d_params, io->d_packed, io->d_dropmask, 1, io->seed, io->step, io->d_workspace,
                         io->workspace_bytes);
  p.dyn = dyn; p.logits = io->d_logits; p.feat = io->d_feat; p.sym_mode = sym_mode;
  if ((rc = check_forward(c.d, p)) || (rc = forward_impl(c, st, p))) return rc;
  const RowSel sel = batch_sel(&batch, dyn);
  if (cps) {
    // the CPS loss block: one launch; its pseudo-labels take the front of the (otherwise unused) probability region,
    // its row table the loss workspace; no embedding gradient exists, so the backward runs with d_dfeat = null
    if ((rc = cps_loss_impl(c.d, io->bt, io->btu, io->d_logits, io->d_labels, hp, io->d_scalars, sw.dlogits,
                            (int64_t*)sw.probs, sw.loss, c.loss_bytes, st, &sel)))
      return rc;
  } else if ((rc = loss_both(c.d, io->bt, io->btu, io->d_logits, io->d_feat, io->d_labels, &io->banks,
                      io->smooth, io->adap_mask, hp, io->d_scalars, sw.dlogits, sw.dfeat, sw.probs, sw.loss,
                      c.loss_bytes, st, &sel)))
    return rc;
  // The eager step without clipping and without a norms row: the reduce launch applies the update itself (every live
  // gradient comes from it and Adam is elementwise), and no optimizer launch follows.  A captured step keeps two nodes:
  // its reduce launch advances the device cursor while Adam reads the row behind it.  CMLPL_FUSE_ADAM=0: two launches.
  AdamFuse fuse;
  const bool fused = io->apply_update && io->adam_t >= 1 && dyn.table == nullptr && switches().fuse_adam != 0 &&
                     (opt == nullptr || !optim_norm_wanted(opt));
  if (fused) {
    fuse.params = io->d_params; fuse.m = io->d_m; fuse.v = io->d_v; fuse.pstride = L.param_total; fuse.gbase = io->d_grads;
    adam_fuse_scalars(fuse, hp->lr, hp->beta1, hp->beta2, hp->eps, io->adam_t);
    fuse.keep = opt != nullptr ? adam_keep(hp->lr, opt->weight_decay) : 1.f;
    fuse.packed = io->d_packed; fuse.pi = make_pack_info(c.d, L);
  }
  // (the backward's own checks are among those already made: it reads what the forward was given and sw.dlogits)
  p.dlogits = sw.dlogits; p.dfeat = cps ? nullptr : sw.dfeat; p.grads = io->d_grads; p.grad_stride = L.param_total;
  p.dyn_cursor = io->d_dyn_cursor; p.fuse = fused ? &fuse : nullptr;
  if ((rc = backward_impl(c, st, p))) return rc;
  if (fused) return 0;
  if (io->apply_update)   // (device-side scalars: the by-value step count is not used, any valid one will do)
    return adam_impl(c.d, L, 2, io->d_params, L.param_total, io->d_grads, L.param_total, io->d_m, io->d_v,
                     (dyn.table != nullptr && io->adam_t < 1) ? 1 : io->adam_t, hp, io->d_packed, st, dyn, opt);
  if (opt != nullptr && opt->d_norms != nullptr)     // no update: the norms of these gradients all the same
    return grad_norm_impl(L, 2, io->d_grads, L.param_total, opt->max_norm, opt->d_partials, opt->d_norms, st, dyn);
  return 0;
}
int cmlpl_train_step(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io, void* stream) {
  return cmlpl_train_step_opt(shape, hp, io, nullptr, stream);
}

// ---- the step as a replayable hipGraph
int cmlpl_step_graph_create_opt(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io,
                                const cmlpl_optim* opt, void* stream, void** graph_out) {
  if (!io || !graph_out || !io->d_dyn_table || !io->d_dyn_cursor) return CMLPL_E_ARG;
  return capture_graph((hipStream_t)stream, [&]() { return cmlpl_train_step_opt(shape, hp, io, opt, stream); }, graph_out);
}
int cmlpl_step_graph_create(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io, void* stream,
                            void** graph_out) {
  return cmlpl_step_graph_create_opt(shape, hp, io, nullptr, stream, graph_out);
}

int cmlpl_dist_stage_graph_create(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_dist_io* io, int stage,
                                  void* stream, void** graph_out) {
  if (!shape || !hp || !io || !graph_out || !io->d_dyn_table || !io->d_dyn_cursor || !io->batch.d_lab_idx ||
      !io->batch.d_unl_idx || io->batch.noise8 != nullptr)
    return CMLPL_E_ARG;
  return capture_graph((hipStream_t)stream, [&]() { return dist_stage_run(shape, hp, io, stage, stream); }, graph_out);
}

int cmlpl_step_graph_launch(void* graph, void* stream) {
  if (!graph) return CMLPL_E_ARG;
  return chk(hipGraphLaunch(((StepGraph*)graph)->exec, (hipStream_t)stream));
}

int cmlpl_step_graph_destroy(void* graph) {
  if (!graph) return CMLPL_E_ARG;
  StepGraph* sg = (StepGraph*)graph;
  (void)hipGraphExecDestroy(sg->exec);
  (void)hipGraphDestroy(sg->graph);
  delete sg;
  return 0;
}

int cmlpl_timing_begin(uint32_t kernel_mask, int max_launches) {
  Timing& t = g_timing;
  if (t.on || max_launches < 1) return CMLPL_E_ARG;
  t.ev.resize((size_t)max_launches * 2);
  for (auto& e : t.ev) {
    hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) return (int)rc;
  }
  t.ids.clear(); t.used = 0; t.mask = kernel_mask; t.on = true;
  return 0;
}

int cmlpl_timing_end(double* ms_sum, int64_t* launches) {
  Timing& t = g_timing;
  if (!t.on || !ms_sum || !launches) return CMLPL_E_ARG;
  t.on = false;
  for (int i = 0; i < CMLPL_K_COUNT; ++i) { ms_sum[i] = 0.0; launches[i] = 0; }
  int rc = 0;
  for (size_t i = 0; i < t.ids.size(); ++i) {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(t.ev[2 * i + 1]);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, t.ev[2 * i], t.ev[2 * i + 1]);
    if (e != hipSuccess) { rc = (int)e; break; }
    ms_sum[t.ids[i]] += ms; launches[t.ids[i]] += 1;
  }
  for (auto& e : t.ev) (void)hipEventDestroy(e);
  t.ev.clear(); t.ids.clear(); t.used = 0;
  return rc;
}

int cmlpl_debug_region(const cmlpl_shape* shape, int nets, int n, const char* name, size_t* byte_offset,
                       size_t* bytes) {
  StepCtx c;
  if (!ctx_shape(shape, &c)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || !name || !byte_offset || !bytes) return CMLPL_E_ARG;
  char* base = (char*)(uintptr_t)4096;   // fake base: only offsets are used
  if (!ctx_carve(&c, nets, n, 0, base)) return CMLPL_E_SHAPE;
  const Dims& d = c.d;
  const NetWs& w = c.nw;
  const size_t N = (size_t)nets * n;
  struct { const char* nm; const void* p; size_t b; } tab[] = {
      {"a0", w.a0, N * d.HW * 256}, {"p1", w.p1, N * d.P2 * 256}, {"m1", w.m1, N * d.P2 * 64},
      {"p2", w.p2, N * d.P4 * 256}, {"m2", w.m2, N * d.P4 * 64}, {"y", w.y, N * 4096},
      {"ynorm", w.ynorm, N * 4}, {"catd", w.catd, N * d.F * 4}, {"dropgen", w.dropgen, N * d.F * 4},
      {"dy", w.dy, N * 4096}, {"dp2", w.dp2, N * d.P4 * 256}, {"dp1", w.dp1, N * d.P2 * 256},
      {"da0", w.da0, N * d.HW * 256}};
  for (auto& t : tab)
    if (!strcmp(t.nm, name)) { *byte_offset = (size_t)((const char*)t.p - base); *bytes = t.b; return 0; }
  if (nets != 2) return CMLPL_E_ARG;          // (the step's regions: two networks)
  if (!strcmp(name, "xn")) {   // the step's augmented patch rows [2][n][C*H*W] (cmlpl_forward keeps them for cmlpl_backward)
    *byte_offset = w.bytes; *bytes = (size_t)2 * n * d.C * d.HW * 4;
    return 0;
  }
  // a CPS step's pseudo-labels: int64 [2][btu]; a CMLPL step's probabilities: p_w, p_s, p_w0, p_s0 as [4][btu][K] -- both
  // at the start of the same region (n covers them)
  const bool pseudo = !strcmp(name, "cps_pseudo");
  if (pseudo || !strcmp(name, "probs")) {
    *byte_offset = (size_t)((const char*)c.sw.probs - base);
    *bytes = pseudo ? (size_t)2 * n * 8 : (size_t)4 * n * d.K * 4;
    return 0;
  }
  return CMLPL_E_ARG;
}

int cmlpl_debug_reload_switches(void) {
  switches_table() = read_switches();
  return 0;
}

int cmlpl_debug_two_piece(const cmlpl_shape* shape, int nets, int n) {
  Dims d;
  if (!make_dims(shape, &d) || nets < 1 || nets > 2 || n < 1) return CMLPL_E_SHAPE;
  NetRoute r;
  make_route(d, nets, n, &r);           // (a map without a plan has no two-piece launch: nothing to refuse here)
  const int f = switches().f16x2;
  if (r.fwd == ROUTE_A && r.bwd == ROUTE_A)     // the per-sample kernels
    return r.stats ? 1 | 2 | 4 : f == 2 ? 1 : f == 3 ? 2 : 0;    // (the switch's forward-only / backward-only modes: weight gradients on three pieces)
  if (r.fwd != ROUTE_C || r.bwd != ROUTE_C) return 0;   // (mixed paths: switch-forced variants)
  return (r.plan[0].h2x ? 1 : 0) | (r.plan[1].h2x ? 2 : 0) | (r.stats ? 4 : 0) | (r.plan[2].h2x && r.plan[3].h2x ? 8 : 0);
}

int cmlpl_debug_conv3_plan(const cmlpl_shape* shape, int nets, int n, int map, int mode, int* out3) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || map < 0 || map > 1 || mode < 0 || mode > 1 || !out3) return CMLPL_E_ARG;
  NetRoute r;
  make_route(d, nets, n, &r);
  const Conv3Variant& pl = r.plan[2 * map + mode];
  if (pl.S < 1) return CMLPL_E_SHAPE;
  out3[0] = pl.S; out3[1] = pl.MTW; out3[2] = pl.nw;
  return 0;
}

int cmlpl_debug_route(const cmlpl_shape* shape, int nets, int n, int* out) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || !out) return CMLPL_E_ARG;
  NetRoute r;
  if (!make_route(d, nets, n, &r)) return CMLPL_E_SHAPE;
  int* o = out;
  *o++ = r.fwd; *o++ = r.bwd; *o++ = (r.fwd_ps.big || r.bwd_ps.big) ? 1 : 0;
  for (const Conv3Variant* v : {&r.fwd_ps, &r.bwd_ps}) { *o++ = v->nw; *o++ = v->tpw; *o++ = v->h2x ? 1 : 0; }
  for (const Conv3Variant& p : r.plan) { *o++ = p.S; *o++ = p.MTW; *o++ = p.nw; *o++ = p.ks ? 1 : 0; *o++ = p.h2x ? 1 : 0; }
  *o++ = r.stats ? 1 : 0;
  return 0;
}

int cmlpl_debug_wgrad3_plan(const cmlpl_shape* shape, int nets, int n, int* out) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  if (nets < 1 || nets > 2 || n < 1 || !out) return CMLPL_E_ARG;
  NetRoute r;
  if (!make_route(d, nets, n, &r)) return CMLPL_E_SHAPE;
  Wgrad3Plan p1, p2;
  bool pair = false;
  if (!plan_wgrad3_both(nets, n, d.H, d.W, d.H2, d.W2, true, &p1, &p2, &pair)) return CMLPL_E_SHAPE;
  // (the list exists in the pair launch only, and only in a step whose launches leave the maxima table)
  const size_t lbytes = pair ? wgrad3_pair_list_bytes(p1, p2, n, d.H, d.H2, r.stats) : 0;
  int* o = out;
  for (const Wgrad3Plan* p : {&p1, &p2}) {
    *o++ = p->rsplit; *o++ = p->b3; *o++ = p->U; *o++ = p->UPG; *o++ = p->G; *o++ = (int)(p->lds + lbytes); *o++ = p->cspl;
  }
  *o++ = pair ? 1 : 0; *o++ = lbytes > 0 ? 1 : 0; *o++ = device_cus();
  return 0;
}

int cmlpl_debug_loss_plan(const cmlpl_shape* shape, const cmlpl_shard* shard, int bank_rows, int smooth, int* out) {
  Dims d;
  if (!make_dims(shape, &d)) return CMLPL_E_SHAPE;
  const cmlpl_shard* sh = shard;
  if (!sh || !out) return CMLPL_E_ARG;
  if (sh->bt_g < 1 || sh->btu_g < 1 || sh->btu_g > 2048 || sh->nlab < 0 || sh->nunl < 1 || sh->lab0 < 0 ||
      sh->unl0 < 0 || sh->lab0 + sh->nlab > sh->bt_g || sh->unl0 + sh->nunl > sh->btu_g ||
      bank_rows < sh->bt_g + sh->btu_g)
    return CMLPL_E_ARG;                 // (what fill_loss_args refuses)
  LossArgs a;
  memset(&a, 0, sizeof(a));
  a.Q = bank_rows; a.bt = sh->bt_g; a.btu = sh->btu_g; a.K = d.K; a.smooth = smooth;
  a.lab0 = sh->lab0; a.nlab = sh->nlab; a.unl0 = sh->unl0; a.nunl = sh->nunl;
  LossPlan p;
  plan_loss_phase1(a, &p);
  int* o = out;
  *o++ = p.kernel; *o++ = p.MB; *o++ = p.NBW; *o++ = p.gx; *o++ = p.gy; *o++ = p.ctiles;
  *o++ = loss_dfeat_lds_shape(a) ? 1 : 0; *o++ = plan_loss_dfeat_lds(a) ? 1 : 0; *o++ = device_cus();
  return 0;
}

int cmlpl_debug_unsup_plan(int B, int K, int* out) {
  UnsupPlan p;
  if (!out || !plan_unsup(B, K, &p)) return CMLPL_E_ARG;
  out[0] = p.route; out[1] = p.regrows;
  return 0;
}

int cmlpl_debug_memobank_plan(int D, int K, int queries, int negatives, int* out) {
  MbPlan p;
  if (!out || !plan_mb_onepass(D, K, queries, negatives, &p)) return CMLPL_E_ARG;
  out[0] = p.kernel; out[1] = (int)p.lds_infonce; out[2] = (int)p.lds_scatter;
  return 0;
}

int cmlpl_debug_ntxent_plan(int B, int D, int aligned, int* out) {
  NtxPlan p;
  if (!out || !plan_ntxent(B, D, aligned != 0 && D % 4 == 0, &p)) return CMLPL_E_ARG;
  int* o = out;
  *o++ = p.route; *o++ = p.ncw; *o++ = p.kc; *o++ = p.waves; *o++ = p.sim_gx; *o++ = p.sim_gy; *o++ = p.grad_gx;
  *o++ = p.grad_gy; *o++ = (int)p.lds; *o++ = p.ct;
  return 0;
}

}  // extern "C"
