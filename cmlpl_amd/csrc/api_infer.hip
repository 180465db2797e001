// C-ABI entry points of prediction (include/cmlpl.h): window cuts, inference straight from the scene cube, the spectral
// embedding and the views of test-time augmentation.  Argument checking and launches only, as in api.hip.
#include "api_common.hpp"

using namespace cmlpl;

extern "C" {

// which cuts take w x w windows of C channels (include/cmlpl.h): the launchers' own LDS sizes against their own limit
int cmlpl_patches_fit(int C, int w) {
  if (C < 1 || w < 1 || w > 4096 || C > 65536) return 0;          // (far past any fit; w * C below stays inside int)
  return (extract_lds(C, w) <= LDS_MAX ? 1 : 0) | (tta_patches_lds(C, w) <= LDS_MAX ? 2 : 0);
}

int cmlpl_extract_patches(const float* d_cube, int rows, int cols, int C, int w, const int64_t* d_pixel_idx, int n,
                          float* d_out, void* stream) {
  if (!d_cube || !d_pixel_idx || !d_out || rows < 1 || cols < 1 || C < 1 || w < 1 || n < 1) return CMLPL_E_ARG;
  if (w / 2 > rows || w / 2 > cols || !(cmlpl_patches_fit(C, w) & 1)) return CMLPL_E_SHAPE;
  return chk(launch_extract_patches(d_cube, rows, cols, C, w, (const long long*)d_pixel_idx, n, d_out,
                                    (hipStream_t)stream));
}

// ---- inference straight from the scene cube: ONE core under the four entry points.  `nets` networks score n pixels -- a
// LIST (d_pix, with d_spec_row) or the RANGE from pixel0 on -- clean (view == nullptr) or on a view of test-time
// augmentation (include/cmlpl.h, "THE DEFINITION OF A VIEW"; sigma == 0: exactly the clean call's launches and writes).
// Workspace: y = relu(feat_spe(spectrum)) [nets][n][1024], then -- a view call -- the view's spectra rows [n][bands].
static bool view_args_ok(float sigma) { return sigma >= 0.f && sigma <= 3.0e38f; }   // (a NaN fails both)
// the spatial element of a view ("THE DEFINITION OF A SPATIAL ELEMENT"): 0, or the error of one a h x w window does not take
static int view_sym_check(uint32_t sym, int h, int w) {
  if (sym > 7u) return CMLPL_E_ARG;
  return ((sym & 4u) && h != w) ? CMLPL_E_SHAPE : 0;
}

static size_t infer_y_bytes(int nets, int n) { return up256((size_t)nets * n * 1024 * 4); }

static size_t infer_workspace(const cmlpl_shape* shape, int nets, int n, bool view) {
  Dims d;
  Conv3Variant v;
  if (!make_dims(shape, &d) || n < 1 || nets < 1 || nets > 2 || !route_infer(d.H, d.W, d.C, d.K, &v)) return 0;   // 0: not a shape the fused forward takes
  return infer_y_bytes(nets, n) + (view ? up256((size_t)n * shape->bands * 4) : 0);
}

static int infer_impl(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride, const float* d_packed,
                      int64_t packed_stride, const float* d_cube, int rows, int cols, const float* d_spectra, bool listed,
                      const int64_t* d_spec_row, const int64_t* d_pix, int64_t pixel0, int n, int64_t* d_labels,
                      float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream, const ViewKey* view) {
  Dims d;
  cmlpl_layout_t L;
  if (view && view->sym > 7u) return CMLPL_E_ARG;
  if (!make_dims(shape, &d) || cmlpl_layout(shape, &L)) return CMLPL_E_SHAPE;
  if (!d_params || !d_packed || !d_cube || !d_spectra || !d_labels || !d_workspace || rows < 1 || cols < 1 || n < 1 ||
      (view && !view_args_ok(view->sigma)))
    return CMLPL_E_ARG;
  if (view) if (int src = view_sym_check(view->sym, d.H, d.W)) return src;
  if (rows < d.H / 2 || cols < d.W / 2) return CMLPL_E_ARG;      // (one mirror fold: what the launcher refuses, either feed)
  if (listed ? (!d_pix || nets < 1 || nets > 2 ||
                (nets == 2 && (param_stride < L.param_total || packed_stride < L.packed_total)))
             : (pixel0 < 0 || pixel0 + n > (int64_t)rows * cols))
    return CMLPL_E_ARG;
  Conv3Variant v;
  if (!route_infer(d.H, d.W, d.C, d.K, &v)) return CMLPL_E_SHAPE;
  const bool big = (int64_t)rows * cols * d.C >= (1LL << 31);                  // (the gather's 32-bit offsets)
  if (listed && big) return CMLPL_E_ARG;
  if (infer_workspace(shape, nets, n, view != nullptr) > workspace_bytes) return CMLPL_E_WORKSPACE;
  if (view && view->sigma == 0.f && view->sym == 0u) view = nullptr;      // the clean forward, its launches and its bytes
  if (view && !listed && big) return CMLPL_E_ARG;                         // (what the launcher refuses)
  hipStream_t st = (hipStream_t)stream;
  float* y = (float*)d_workspace;
  const float* sn = listed ? d_spectra : d_spectra + (long long)pixel0 * d.bands;
  const long long* spec_row = (const long long*)d_spec_row;
  int rc;
  if (view) {          // every network scores the same view: one set of rows, read by all (network stride 0)
    float* vrows = (float*)((char*)d_workspace + infer_y_bytes(nets, n));
    if ((rc = chk(launch_tta_spectra(sn, spec_row, (const long long*)d_pix, pixel0, (long long)rows * cols, n, d.bands, vrows,
                                     *view, st)))) return rc;
    sn = vrows;
    spec_row = nullptr;
  }
  // spectral branch of the pixels (canonical weights); the range-fed call is one network on plain rows
  if ((rc = chk(launch_spe_fwd(nets, n, d.bands, sn, d_params + L.param_off[6], d_params + L.param_off[7],
                               listed ? (long long)param_stride : L.param_total, y, st, spec_row, listed ? 0 : -1)))) return rc;
  FwdTail t;
  memset(&t, 0, sizeof(t));
  t.w2f = d_packed + pack_off_b3(d.C, d.bands, 2); t.b2 = d_params + L.param_off[5];
  t.wc = d_params + L.param_off[8]; t.bc = d_params + L.param_off[9];
  t.y = y; t.logits = d_logits; t.K = d.K;
  const InferNets nn = {nets, (long long)param_stride, (long long)packed_stride, (const long long*)d_pix};
  return chk(launch_conv3_infer(v, n, d.C, d.H, d.W, d_cube, rows, cols, pixel0, d_packed + pack_off_w0b3(d.C, d.bands),
                                d_params + L.param_off[1], d_packed + pack_off_b3(d.C, d.bands, 0),
                                d_params + L.param_off[3], t, (long long*)d_labels, st, listed ? &nn : nullptr, view));
}

size_t cmlpl_infer_workspace_bytes(const cmlpl_shape* shape, int n) { return infer_workspace(shape, 1, n, false); }
size_t cmlpl_eval_workspace_bytes(const cmlpl_shape* shape, int nets, int n) { return infer_workspace(shape, nets, n, false); }
size_t cmlpl_infer_tta_workspace_bytes(const cmlpl_shape* shape, int n) { return infer_workspace(shape, 1, n, true); }
size_t cmlpl_eval_tta_workspace_bytes(const cmlpl_shape* shape, int nets, int n) { return infer_workspace(shape, nets, n, true); }

int cmlpl_infer_cube(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                     int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                     float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream) {
  return infer_impl(shape, 1, d_params, 0, d_packed, 0, d_cube, rows, cols, d_spectra, false, nullptr, nullptr, pixel0, n,
                    d_labels, d_logits, d_workspace, workspace_bytes, stream, nullptr);
}

int cmlpl_infer_pixels(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                       const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                       const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                       int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream) {
  return infer_impl(shape, nets, d_params, param_stride, d_packed, packed_stride, d_cube, rows, cols, d_spectra, true,
                    d_spec_row, d_pix, 0, n, d_labels, d_logits, d_workspace, workspace_bytes, stream, nullptr);
}

// The embedding of listed spectra rows (include/cmlpl.h): the spectral launch of infer_impl straight into d_feat, then the
// normalisation in place (feat_norm_kernel reads its own float4 before it stores it).
int cmlpl_embed(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride, const float* d_spectra,
                const int64_t* d_spec_row, int n, float* d_feat, float* d_norm, void* stream) {
  Dims d;
  cmlpl_layout_t L;
  if (!make_dims(shape, &d) || cmlpl_layout(shape, &L)) return CMLPL_E_SHAPE;
  if (!d_params || !d_spectra || !d_feat || !d_norm || n < 1 || nets < 1 || nets > 2 ||
      (nets == 2 && param_stride < L.param_total) || (reinterpret_cast<uintptr_t>(d_feat) & 15))
    return CMLPL_E_ARG;
  hipStream_t st = (hipStream_t)stream;
  int rc;
  if ((rc = chk(launch_spe_fwd(nets, n, d.bands, d_spectra, d_params + L.param_off[6], d_params + L.param_off[7],
                               (long long)param_stride, d_feat, st, (const long long*)d_spec_row, 0)))) return rc;
  return chk(launch_feat_norm(nets, n, d_feat, d_norm, d_feat, (long long)n * 1024, st));
}

int cmlpl_infer_cube_tta_sym(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                             int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                             float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream, float sigma,
                             uint64_t seed, uint32_t view, uint32_t sym) {
  const ViewKey key = {sigma, seed, view, sym};
  return infer_impl(shape, 1, d_params, 0, d_packed, 0, d_cube, rows, cols, d_spectra, false, nullptr, nullptr, pixel0, n,
                    d_labels, d_logits, d_workspace, workspace_bytes, stream, &key);
}

int cmlpl_infer_cube_tta(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                         int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                         float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream, float sigma,
                         uint64_t seed, uint32_t view) {
  return cmlpl_infer_cube_tta_sym(shape, d_params, d_packed, d_cube, rows, cols, d_spectra, pixel0, n, d_labels, d_logits,
                                  d_workspace, workspace_bytes, stream, sigma, seed, view, 0);
}

int cmlpl_infer_pixels_tta_sym(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                               const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                               const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                               int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes,
                               void* stream, float sigma, uint64_t seed, uint32_t view, uint32_t sym) {
  const ViewKey key = {sigma, seed, view, sym};
  return infer_impl(shape, nets, d_params, param_stride, d_packed, packed_stride, d_cube, rows, cols, d_spectra, true,
                    d_spec_row, d_pix, 0, n, d_labels, d_logits, d_workspace, workspace_bytes, stream, &key);
}

int cmlpl_infer_pixels_tta(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                           const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                           const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                           int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream,
                           float sigma, uint64_t seed, uint32_t view) {
  return cmlpl_infer_pixels_tta_sym(shape, nets, d_params, param_stride, d_packed, packed_stride, d_cube, rows, cols,
                                    d_spectra, d_spec_row, d_pix, n, d_labels, d_logits, d_workspace, workspace_bytes, stream,
                                    sigma, seed, view, 0);
}

int cmlpl_tta_patches(const float* d_cube, int rows, int cols, int C, int w, const int64_t* d_pixel_idx, int n,
                      float* d_out, const float* d_spectra, const int64_t* d_spec_row, int bands, float* d_spectra_out,
                      float sigma, uint64_t seed, uint32_t view, void* stream) {
  return cmlpl_tta_patches_sym(d_cube, rows, cols, C, w, d_pixel_idx, n, d_out, d_spectra, d_spec_row, bands, d_spectra_out,
                               sigma, seed, view, stream, 0);
}

int cmlpl_tta_patches_sym(const float* d_cube, int rows, int cols, int C, int w, const int64_t* d_pixel_idx, int n,
                          float* d_out, const float* d_spectra, const int64_t* d_spec_row, int bands, float* d_spectra_out,
                          float sigma, uint64_t seed, uint32_t view, void* stream, uint32_t sym) {
  if (sym > 7u) return CMLPL_E_ARG;      // (the windows are square: every element applies)
  if (!d_pixel_idx || (!d_out && !d_spectra_out) || rows < 1 || cols < 1 || n < 1 || !view_args_ok(sigma)) return CMLPL_E_ARG;
  if (d_out && (!d_cube || C < 1 || w < 1)) return CMLPL_E_ARG;
  if (d_spectra_out && (!d_spectra || bands < 1)) return CMLPL_E_ARG;
  if (d_out && (w / 2 > rows || w / 2 > cols || !(cmlpl_patches_fit(C, w) & 2))) return CMLPL_E_SHAPE;
  const ViewKey key = {sigma, seed, view, sym};
  int rc;
  if (d_out && (rc = chk(launch_tta_patches(d_cube, rows, cols, C, w, (const long long*)d_pixel_idx, n, d_out, key,
                                            (hipStream_t)stream)))) return rc;
  if (d_spectra_out && (rc = chk(launch_tta_spectra(d_spectra, (const long long*)d_spec_row, (const long long*)d_pixel_idx, 0,
                                                    (long long)rows * cols, n, bands, d_spectra_out, key,
                                                    (hipStream_t)stream)))) return rc;
  return 0;
}

}  // extern "C"
