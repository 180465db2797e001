/* cmlpl.h -- C ABI of the MI355X-native CMLPL training hot path (libcmlpl_hip.so).
 *
 * The reference (liuli33/CMLPL) has no FFI/plugin interface: its hot path is inline
 * PyTorch in train.py:150-279 and tools/models.py:97-152.  This header is therefore
 * the boundary the reference's Python would bind via ctypes; each
 * entry point names the reference lines it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; every pointer named d_* is DEVICE memory
 *     owned by the caller (no ownership transfer, no hidden allocation);
 *   - every call takes a hipStream_t as `void* stream`, is asynchronous and re-entrant
 *     across streams (no implicit synchronisation, graph-capturable);
 *   - return 0 = ok, negative = argument error (CMLPL_E_*), positive = hipError_t;
 *   - every tensor is fp32 and every result is fp32-grade; labels are int64 (torch.long).  The 3x3 / 1x1 convolutions
 *     (forward, data and weight gradients) form each fp32 product from three exact bf16 pieces per operand, six of
 *     the nine piece products (the dropped ones are below 2^-21 |a b| in the worst case, 0.7 * 2^-24 on average),
 *     fp32 accumulation: measured against fp64 at the level of an fp32 fma chain.  An infinite
 *     operand of such a product becomes NaN (a finite fp32 path would keep the infinity); NaN stays NaN.
 *   - the library expects ONE calling thread per process at a time (one process per GPU is the deployment
 *     model); the lazily-set kernel attributes are tracked per device, so engines on several devices of one
 *     process work, but cmlpl_timing_begin/_end state is process-global and not thread-safe.
 *   - `nets` is 1 or 2: kernels are batched over the two networks Base/Base1
 *     (train.py:118-125) through a grid dimension; per-network buffers are
 *     laid out [net][...] with the strides returned by cmlpl_layout().
 */
#ifndef CMLPL_H
#define CMLPL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMLPL_ABI_VERSION 6
#define CMLPL_FEAT_DIM 1024 /* tools/models.py:119 */
#define CMLPL_CONV_CH 64    /* tools/models.py:102-107 */

enum {
  CMLPL_E_ARG = -1,      /* null pointer / bad size */
  CMLPL_E_SHAPE = -2,    /* unsupported shape (e.g. K > 64, window too large for LDS) */
  CMLPL_E_WORKSPACE = -3,/* workspace too small */
  CMLPL_E_COMM = -4      /* cmlpl_dist_step: a collective failed (RCCL's ncclResult_t r > 0 comes back as -4 - r) */
};

/* Shape of one BaseNet2 (tools/models.py:98-128, generalised per SURVEY.md section 0). */
typedef struct cmlpl_shape {
  int32_t C;     /* conv0 input channels (reference literal 60, models.py:102) */
  int32_t H, W;  /* window size (reference: 20x20)                            */
  int32_t bands; /* num_features (models.py:121)                              */
  int32_t K;     /* num_classes  (models.py:127), 1..64                       */
} cmlpl_shape;

/* Hyper-parameters consumed inside the step (train.py:356-379 flags + literals). */
typedef struct cmlpl_hparams {
  float lr, beta1, beta2, eps;      /* torch.optim.Adam defaults, train.py:131-132        */
  float temperature, alpha;         /* train.py:374,371                                    */
  float noise_sigma, dropout_p;     /* train.py:378,377                                    */
  float w_contrast, w_mutual;       /* literals 0.5 / 4, train.py:266,270                  */
  float pos_thr, neg_thr;           /* literals 0.8 / 0.3, train.py:251,254                */
} cmlpl_hparams;

/* Flat parameter buffer of ONE network: the 16 state_dict tensors of BaseNet2 in
 * canonical PyTorch layouts, LIVE tensors first:
 *   0 conv0.weight[64,C,1,1] 1 conv0.bias 2 conv1.weight[64,64,3,3] 3 conv1.bias
 *   4 conv2.weight 5 conv2.bias 6 feat_spe.weight[1024,bands] 7 feat_spe.bias
 *   8 classifier.weight[K,cls_in] 9 classifier.bias | 10..15 feat_ss*, dead (models.py:122-126)
 * Each tensor's offset is a multiple of 4 floats. */
#define CMLPL_NUM_TENSORS 16
#define CMLPL_NUM_LIVE 10
typedef struct cmlpl_layout_t {
  int64_t param_off[CMLPL_NUM_TENSORS];   /* element offsets in the per-net flat buffer  */
  int64_t param_numel[CMLPL_NUM_TENSORS];
  int64_t param_total;                    /* floats per net (all 16 tensors)             */
  int64_t param_live;                     /* floats per net covered by Adam (tensors 0-9) */
  int64_t packed_total;                   /* floats per net of kernel-side re-packed weights (3x3 and conv0 weights as
                                             split-bf16 MFMA fragments, k-major copies of conv0 / feat_spe); opaque to
                                             the caller; written by cmlpl_pack_weights and by cmlpl_adam_step */
  int32_t cls_in;                         /* 64*(H/2/2)*(W/2/2) + 1024                    */
  int32_t reserved;
} cmlpl_layout_t;

int cmlpl_abi_version(void);
/* 16-hex-digit hash of the kernel sources and this header the binary was built from ("unknown" for a build outside
 * cmlpl_amd/build_ext.py).  The Python binding compares it with the hash of the sources next to it and refuses a
 * stale binary (cmlpl_amd/_lib.py); the reference has no counterpart (it has no native code). */
const char* cmlpl_source_hash(void);
int cmlpl_layout(const cmlpl_shape* shape, cmlpl_layout_t* out);

/* Bytes of device workspace needed by the calls below for up to `n` rows per network
 * (n = labelled + unlabelled), `nets` networks and a bank of `bank_rows` rows. */
size_t cmlpl_workspace_bytes(const cmlpl_shape* shape, int nets, int n, int bank_rows);

/* Re-pack the weights of `nets` networks into the kernel-side layouts (every entry of d_packed, pad rows included).
 * Call it once after parameters are set or loaded; cmlpl_adam_step then keeps every non-pad entry current itself
 * (it never touches the zero pad rows this call writes, so a packed buffer must have been through this call once). */
int cmlpl_pack_weights(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                       float* d_packed, void* stream);

/* Row shard of a data-parallel step: the global batch has bt_g labelled and
 * btu_g unlabelled rows; this rank owns labelled rows [lab0, lab0+nlab) and unlabelled rows
 * [unl0, unl0+nunl).  One GPU: {bt, btu, 0, bt, 0, btu} (or NULL where allowed).  In-kernel random
 * streams are keyed by the GLOBAL sample index, so noise/dropout do not depend on the sharding. */
typedef struct cmlpl_shard {
  int32_t bt_g, btu_g;
  int32_t lab0, nlab;
  int32_t unl0, nunl;
} cmlpl_shard;

/* Input augmentation + batch concat: train.py:157-158,163-164,170-171,173-174,181-184.
 *   xn[net] = cat(XPl, XPu) + sigma * N(0,1),  sn[net] = cat(Xl, Xu) + sigma * N(0,1)
 * d_noise: NULL (in-kernel counter-based draws -- PCG4D hash + Box-Muller, keyed by seed/step/stream/global sample) or 8 device pointers in the
 * reference's draw order [XPl/0, Xl/0, XPl/1, Xl/1, XPu/0, Xu/0, XPu/1, Xu/1].
 * With bt == 0 or sigma == 0 it is a plain (concatenating) copy. */
int cmlpl_augment(const cmlpl_shape* shape, int nets, int bt, int btu,
                  const float* d_xpl, const float* d_xl, const float* d_xpu, const float* d_xu,
                  const float* const* noise8, float sigma, uint64_t seed, uint64_t step,
                  const cmlpl_shard* shard /* NULL = one GPU */, float* d_xn, float* d_sn,
                  float* d_snT /* optional [nets][bands][n] copy of sn, k-major for feat_spe */, void* stream);

/* BaseNet2.forward (tools/models.py:130-152) for `nets` networks on rows [n].
 *   d_xn [nets][n][C][H*W], d_sn [nets][n][bands]  (already augmented)
 *   d_dropmask: [nets][n][cls_in] multiplier (0 or 1/(1-p)); NULL with dropout_p == 0 or
 *               train == 0 -> no dropout; NULL with train != 0 and p > 0 -> Philox mask
 *   outputs: d_logits [nets][n][K], d_feat [nets][n][1024]; activations needed by
 *   cmlpl_basenet2_bwd are kept in d_workspace. */
int cmlpl_basenet2_fwd(const cmlpl_shape* shape, int nets, int n,
                       const float* d_params, int64_t param_stride, const float* d_packed,
                       const float* d_xn, const float* d_sn,
                       const float* d_snT /* optional: sn transposed [nets][bands][n] (from cmlpl_augment) */,
                       const float* d_dropmask,
                       float dropout_p, int train, uint64_t seed, uint64_t step,
                       const cmlpl_shard* shard /* NULL = rows are global samples 0..n-1 */,
                       float* d_logits, float* d_feat, void* d_workspace, size_t workspace_bytes,
                       void* stream);

/* Backward of the above w.r.t. the 10 live tensors (autograd of train.py:267,271).
 *   d_dlogits [nets][n][K], d_dfeat [nets][n][1024] (may be NULL = zero)
 *   d_grads   [nets][grad_stride] flat, same offsets as the parameters (tensors 0-9 written). */
int cmlpl_basenet2_bwd(const cmlpl_shape* shape, int nets, int n,
                       const float* d_params, int64_t param_stride, const float* d_packed,
                       const float* d_xn, const float* d_sn,
                       const float* d_dropmask, float dropout_p, int train, /* as given to _fwd */
                       const float* d_dlogits, const float* d_dfeat,
                       float* d_grads, int64_t grad_stride,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* One training batch as the reference holds it (train.py:155-171): labelled and unlabelled rows in their own
 * buffers (the concat of train.py:173-174,183-184 is an index computation in the kernels, not a copy) and the
 * augmentation noise either drawn in-kernel (PCG4D hash + Box-Muller, noise8 == NULL) or given as the 8 tensors of the
 * reference's draw order (see cmlpl_augment). */
typedef struct cmlpl_batch {
  const float* d_xpl; const float* d_xl;   /* [bt][C][H][W], [bt][bands]   */
  const float* d_xpu; const float* d_xu;   /* [btu][C][H][W], [btu][bands] */
  const int64_t* d_labels;                 /* [bt] (may be NULL where no entry point reads it) */
  const float* const* noise8;
  int32_t bt, btu;
  /* ABI 3 -- batches BY INDEX (hsi_loader.py:109-133 hands out rows of XP.npy / X.npy / Y.npy by index; the reference's
   * DataLoader then copies them into a batch tensor): when given, labelled row s of the batch is row d_lab_idx[s] of
   * d_xpl / d_xl / d_labels and unlabelled row s is row d_unl_idx[s] of d_xpu / d_xu -- the kernels read the rows where
   * the resident split lies, no gathered copy of the batch exists.  NULL = rows 0 .. bt-1 / 0 .. btu-1 as before.
   * (The explicit noise tensors and dropout masks of parity mode stay indexed by batch row.) */
  const int64_t* d_lab_idx; const int64_t* d_unl_idx;
  /* ABI 6 -- the CUBE-FED batch: no window tensor exists.  d_cube [cube_rows][cube_cols][C] f32 is the resident scene
   * (band-last, what cmlpl_scene_project / cmlpl_extract_patches / cmlpl_infer_cube read); the patch row of labelled
   * batch row s is the H x W window (H == W), through the mirror index of MirrowCut / ExtractPatches
   * (tools/hyper_tools.py:35-55, :226-243), of scene pixel d_lab_pix[r], r = d_lab_idx[s] (or s when d_lab_idx is NULL)
   * -- the SAME split row r that d_xl / d_labels are read at; unlabelled rows likewise through d_unl_pix.  One gather
   * launch in front of the forward forms the augmented rows of both networks from the cube (same noise counters: a
   * cube-fed step is bit-identical to the step on cmlpl_extract_patches' windows).
   *   d_cube == NULL: the batch is read from d_xpl / d_xpu as before (the three fields below are ignored).
   *   d_cube != NULL: d_xpl and d_xpu must be NULL, d_lab_pix / d_unl_pix are required (row-major pixel indices in
   *   [0, cube_rows * cube_cols): the kernels follow them without a bounds check), cube_rows, cube_cols >= the window.
   * Otherwise CMLPL_E_ARG / CMLPL_E_SHAPE (H != W, scene smaller than the window, window too large for LDS). */
  const float* d_cube; int32_t cube_rows, cube_cols;
  const int64_t* d_lab_pix; const int64_t* d_unl_pix;
} cmlpl_batch;

/* One step's scalars in DEVICE memory (ABI 3): what changes from step to step, for a step captured ONCE in a hipGraph
 * and replayed (SURVEY.md section 7 stage 6; the reference's loop passes them as Python scalars, train.py:146-150,
 * 212,221,234-237).  The caller fills a table of rows ahead of time (e.g. one epoch) and passes it with a device
 * cursor: a launch of cmlpl_train_step with d_dyn_table != NULL takes these values from the table instead of from
 * cmlpl_step_io, and advances the cursor itself (in its weight-gradient reduce launch), so that replaying the captured
 * launch sequence walks the table with no host work per step.
 * Table layout: row 0 is the WORKING COPY of the current step's row (the kernels read it there: one dependent load
 * instead of cursor -> row); the rows of steps 1, 2, .. follow at indices 1, 2, ..  To start (or restart) a run of
 * steps the caller writes its rows at 1 .. k, copies row 1 into row 0 as well and sets *d_dyn_cursor = 1; every step
 * then moves the cursor on and copies the next row into row 0 (so the table needs one row beyond the last step's:
 * k + 2 rows for k steps; the extra row's contents do not matter). */
typedef struct cmlpl_dyn {
  uint64_t step;            /* counter of the in-kernel random streams (cmlpl_step_io.step)            */
  int64_t adam_t;           /* 1-based Adam step                                                       */
  int64_t lab_off, unl_off; /* offsets added to the row number before d_lab_idx / d_unl_idx are read   */
  int32_t ptr[2];           /* bank write pointers BEFORE the step (train.py:234,237)                  */
  int32_t smooth;           /* train.py:212 gate                                                       */
  float adap_mask;          /* train.py:221                                                            */
  int32_t hist_row;         /* the step's scalars go to d_scalars + 16 * hist_row                      */
  float adam_step_size;     /* lr / (1 - beta1^adam_t)   } torch.optim.Adam's bias corrections, formed in double  */
  float adam_bc2_sqrt;      /* sqrt(1 - beta2^adam_t)    } on the host: cmlpl_dyn_adam() fills both               */
  int32_t reserved;         /* 0, or the bit pattern of the step's decay factor ("A CLIPPED, DECAYED ADAM STEP")       */
} cmlpl_dyn;
/* the two Adam scalars of a table row, exactly as cmlpl_adam_step forms them from (hp, t) */
int cmlpl_dyn_adam(const cmlpl_hparams* hp, int64_t adam_t, float* step_size, float* bc2_sqrt);

/* Both networks' forward on one batch (train.py:157-189): augmentation + BaseNet2.forward for Base and Base1.
 * Where the window fits the per-sample kernels (H*W <= 128) the patches are augmented inside the fused forward, which
 * also stores the augmented rows in the workspace (2 * n * C * H * W floats written per step); cmlpl_backward lands
 * them for conv0's weight gradient.  It must therefore be given the same batch / seed / step / shard and the SAME
 * workspace (sized by cmlpl_workspace_bytes(shape, 2, bt + btu, bank_rows)), which holds the saved activations and
 * those rows in between -- and NO other cmlpl_forward may run on that workspace between the two (an evaluation or
 * teacher pass in between needs a workspace of its own: it would overwrite the rows the weight gradient reads).
 *   hp: noise_sigma and dropout_p are used.  Outputs as cmlpl_basenet2_fwd / _bwd with nets = 2. */
int cmlpl_forward(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                  const cmlpl_shard* shard /* NULL = one GPU */,
                  const float* d_params /* [2][param_total] */, const float* d_packed /* [2][packed_total] */,
                  const float* d_dropmask, int train, uint64_t seed, uint64_t step,
                  float* d_logits, float* d_feat,
                  float* d_labels_f /* optional [bt]: the labels as float, written for the packed exchange buffer */,
                  void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_backward(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                   const cmlpl_shard* shard,
                   const float* d_params, const float* d_packed,
                   const float* d_dropmask, int train, uint64_t seed, uint64_t step,
                   const float* d_dlogits, const float* d_dfeat, float* d_grads, int64_t grad_stride,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* ABI 4: cmlpl_forward / cmlpl_backward in two parts each, for a step that exchanges data between them (the sharded step
 * of cmlpl_amd/distributed.py).  The split follows what depends on what in tools/models.py:130-152:
 *   cmlpl_forward_spectral : augmented spectra -> feat_spe + ReLU -> L2 normalisation (:142-146) -> d_feat [2][n][1024]
 *                            (+ d_labels_f).  The embeddings depend on NOTHING the convolutions compute: a sharded step
 *                            starts their all-gather here and lets it run under the spatial part.
 *   cmlpl_forward_spatial  : conv0 .. conv2, pooling, concat / dropout / classifier (:132-141,144,147-150) -> d_logits.
 *                            Same workspace, after the spectral part (it reads the spectral ReLU output there).
 *   cmlpl_backward_data    : the data-gradient chain (classifier, conv2, conv1, conv0 partials) and the 3x3 weight-gradient
 *                            partials -- needs d_dlogits ONLY (:144-150): the column-side feature gradient can still be
 *                            in its reduce-scatter.
 *   cmlpl_backward_weights : dy takes its feature-gradient share (through the normalisation's backward; bit-identical to
 *                            the one-part head), partials are reduced, classifier / feat_spe weight gradients -> d_grads.
 * Both halves of a pair take the same batch / seed / step / shard / workspace as the whole call would. */
int cmlpl_forward_spectral(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                           const cmlpl_shard* shard, const float* d_params, uint64_t seed, uint64_t step,
                           float* d_feat, float* d_labels_f /* optional [bt] */,
                           void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_forward_spatial(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                          const cmlpl_shard* shard, const float* d_params, const float* d_packed,
                          const float* d_dropmask, int train, uint64_t seed, uint64_t step, float* d_logits,
                          void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_backward_data(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                        const cmlpl_shard* shard, const float* d_params, const float* d_packed,
                        const float* d_dropmask, int train, uint64_t seed, uint64_t step, const float* d_dlogits,
                        void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_backward_weights(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_batch* batch,
                           const cmlpl_shard* shard, const float* d_params, const float* d_packed,
                           const float* d_dropmask, int train, uint64_t seed, uint64_t step, const float* d_dlogits,
                           const float* d_dfeat, float* d_grads, int64_t grad_stride,
                           void* d_workspace, size_t workspace_bytes, void* stream);

/* State of the two memory banks (train.py:138-145). */
typedef struct cmlpl_banks {
  float* d_feats[2];  /* [Q][1024] queue_feats, queue_feats1 */
  float* d_probs[2];  /* [Q][K]    queue_probs, queue_probs1 */
  int32_t Q;          /* rows, 5*labeled_batch_size*2 (train.py:138) */
  int32_t ptr[2];     /* write pointers BEFORE this step (host keeps train.py:234,237) */
} cmlpl_banks;

/* The loss block, train.py:191-266, forward + analytic backward, plus the bank write
 * (train.py:223-237; rows are written modulo Q).
 *   d_logits [2][n][K], d_feat [2][n][1024]: net 0 = Base ("s"), net 1 = Base1 ("w");
 *   rows [0,bt) labelled, [bt,n) unlabelled; d_labels int64 [bt]
 *   smooth    : train.py:212 gate (epoch > 0 or batch_index > queue_batch)
 *   adap_mask : thr * exp(-0.5*(epoch/num_epochs)^2), train.py:147-148,221
 *   outputs   : d_scalars[16] = {ctr_s,total_s,cls_s,con_s,acc, total_w,cls_w,con_w,ctr_w,
 *                                n_mask_w,n_mask_s,n_pos,n_neg,0,0,0}   (train.py:274-278)
 *               d_dlogits [2][n][K], d_dfeat [2][n][1024]
 *               d_probs [4][btu][K] = {p_w, p_s smoothed, p_w0, p_s0}  (required scratch/output). */
int cmlpl_loss_fwd_bwd(const cmlpl_shape* shape, int bt, int btu,
                       const float* d_logits, const float* d_feat, const int64_t* d_labels,
                       const cmlpl_banks* banks, int smooth, float adap_mask,
                       const cmlpl_hparams* hp,
                       float* d_scalars, float* d_dlogits, float* d_dfeat, float* d_probs,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* The same loss block split at the one point where a data-parallel step must exchange data.
 * Inputs are the GLOBAL logits/feats/labels (rows ordered [labelled of all ranks ; unlabelled of all
 * ranks]); outputs cover this rank's rows only.
 *   phase 1: similarity tiles (local rows x banks / all keys), per-row softmax, CE, smoothing, masks,
 *            mutual loss; writes d_dlogits [2][nlab+nunl][K] and d_probs_local [4][nunl][K]
 *   -- caller all-gathers d_probs_local into d_probs_global (rank-major [W][4][nunl][K]) --
 *   phase 2: pseudo-label graph + contrastive loss for the local rows, bank write of the global batch,
 *            this rank's additive share of d_scalars[16], d_dfeat [2][nlab+nunl][1024] (net-0 rows final;
 *            net-1 rows are to be overwritten by the caller with its reduce-scattered slice of)
 *            d_dfeat_w_partial [btu_g][1024] = this rank's partial of the column-side gradient. */
size_t cmlpl_loss_workspace_bytes(const cmlpl_shape* shape, const cmlpl_shard* shard, int bank_rows);
int cmlpl_loss_phase1(const cmlpl_shape* shape, const cmlpl_shard* shard,
                      const float* d_logits, const float* d_feat, const int64_t* d_labels,
                      const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                      float* d_dlogits, float* d_dfeat /* labelled rows are zeroed here */, float* d_probs_local,
                      void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_loss_phase2(const cmlpl_shape* shape, const cmlpl_shard* shard,
                      const float* d_logits, const float* d_feat, const int64_t* d_labels,
                      const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                      const float* d_probs_global, int probs_shard_rows,
                      float* d_scalars, float* d_dfeat, float* d_dfeat_w_partial,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* The loss phases of the SHARDED step (ABI 4).  What crosses ranks is read WHERE THE ALL-GATHER LEFT IT (no re-ordering
 * copy): d_recv_feat holds `world` rank-major blocks [ 2*n_l*1024 feat | bt_l labels as float ] (n_l = bt_local +
 * btu_local, per-rank rows [labelled ; unlabelled]) -- the buffer cmlpl_forward_spectral's d_feat and d_labels_f are laid
 * out for, gathered while the convolutions run.  The LOGITS are never gathered: d_logits_local [2][n_l][K] are this
 * rank's rows (cmlpl_forward_spatial's output), the only ones phase 1 reads; the bank write needs the other ranks'
 * un-smoothed probabilities and takes them from the gathered probabilities, so it rides with phase 2.
 * Otherwise identical to cmlpl_loss_phase1 / _phase2. */
typedef struct cmlpl_gathered {
  const float* d_recv_feat;
  const float* d_logits_local;
  int32_t world, bt_local, btu_local;
} cmlpl_gathered;
int cmlpl_loss_phase1_g(const cmlpl_shape* shape, const cmlpl_shard* shard, const cmlpl_gathered* gathered,
                        const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                        float* d_dlogits, float* d_dfeat, float* d_probs_local,
                        void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_loss_phase2_g(const cmlpl_shape* shape, const cmlpl_shard* shard, const cmlpl_gathered* gathered,
                        const cmlpl_banks* banks, int smooth, float adap_mask, const cmlpl_hparams* hp,
                        const float* d_probs_global, int probs_shard_rows,
                        float* d_scalars, float* d_dfeat, float* d_dfeat_w_partial,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* Inspection aid: re-order gathered blocks into the global row order [labelled of all ranks ; unlabelled of all ranks]:
 * d_gathered_feat = [world][ 2*n_l*1024 feat | bt_l labels as float ] (the step's exchange buffer), d_gathered_logits =
 * [world][2*n_l*K] (the step does not gather logits: a caller that wants the global logits gathers them for this call). */
int cmlpl_dist_unpack(const cmlpl_shape* shape, int world, int bt_local, int btu_local,
                      const float* d_gathered_feat, const float* d_gathered_logits,
                      float* d_logits_g, float* d_feat_g, int64_t* d_labels_g, void* stream);

/* torch.optim.Adam.step for `nets` flat buffers (train.py:268,272); `t` is the 1-based
 * step count.  Also refreshes the packed conv weights when d_packed != NULL. */
int cmlpl_adam_step(const cmlpl_shape* shape, int nets, float* d_params, int64_t param_stride,
                    const float* d_grads, int64_t grad_stride, float* d_m, float* d_v,
                    int64_t t, const cmlpl_hparams* hp, float* d_packed, void* stream);

/* One whole training step, train.py:150-278: augment -> 2x forward -> loss block ->
 * bank write -> 2x backward -> 2x Adam.  d_state buffers persist across steps. */
typedef struct cmlpl_step_io {
  const float* d_xpl; const float* d_xl; const int64_t* d_labels;  /* labelled batch  */
  const float* d_xpu; const float* d_xu;                           /* unlabelled batch */
  const float* const* noise8;   /* NULL = in-kernel draws (PCG4D hash + Box-Muller)     */
  const float* d_dropmask;      /* NULL = Philox4x32-10 mask; else [2][n][cls_in]       */
  float* d_params; float* d_m; float* d_v; float* d_grads; float* d_packed;  /* [2][param_total] (packed: [2][packed_total]) */
  cmlpl_banks banks;
  float* d_scalars;             /* [16] as in cmlpl_loss_fwd_bwd                        */
  float* d_logits; float* d_feat; /* [2][n][K], [2][n][1024] (outputs)                  */
  void* d_workspace; size_t workspace_bytes;
  int32_t bt, btu;
  int32_t smooth; float adap_mask;
  int64_t adam_t;               /* 1-based                                               */
  uint64_t seed, step;          /* key / counter of the in-kernel random streams         */
  int32_t apply_update;         /* 0 = stop after the gradients                          */
  int32_t reserved;             /* the training METHOD (named after ABI 6, no bump: every earlier caller passes 0):
                                   CMLPL_METHOD_CMLPL = 0, CMLPL_METHOD_CPS = 1 -- see cmlpl_cps_loss_fwd_bwd --
                                   in bits 0..7; bits 8..9: the spatial augmentation of a cube-fed step's rows,
                                   CMLPL_SYM_NONE / _FLIPS / _D4 ("THE DEFINITION OF A SPATIAL ELEMENT"); no other bit */
  /* ABI 3 */
  const int64_t* d_lab_idx; const int64_t* d_unl_idx;   /* as in cmlpl_batch; NULL = consecutive rows */
  const cmlpl_dyn* d_dyn_table; int32_t* d_dyn_cursor;   /* NULL = the by-value fields above are used  */
  /* ABI 6 */
  const float* d_cube; int32_t cube_rows, cube_cols;     /* as in cmlpl_batch; d_cube NULL = d_xpl / d_xpu are read */
  const int64_t* d_lab_pix; const int64_t* d_unl_pix;
} cmlpl_step_io;

int cmlpl_train_step(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io,
                     void* stream);

/* The step as a replayable hipGraph (SURVEY.md section 7 stage 6): _create captures ONE cmlpl_train_step(io) on
 * `stream` (io->d_dyn_table / d_dyn_cursor must be set: everything that changes between steps then lives in device
 * memory) and instantiates it; _launch enqueues one replay = one training step, no other host work.  Run one eager
 * step first (lazily-set kernel attributes cannot be set while capturing).  The handle owns the graph; _destroy frees it. */
int cmlpl_step_graph_create(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io, void* stream,
                            void** graph_out);
int cmlpl_step_graph_launch(void* graph, void* stream);
int cmlpl_step_graph_destroy(void* graph);

/* The seven stages of the SHARDED step (spectral | spatial | loss phase 1 | loss phase 2 | backward data | backward
 * weights | update; the collectives run between them, in the caller's hands: cmlpl_amd/distributed.py) as replayable
 * hipGraphs: what cmlpl_forward_spectral, cmlpl_forward_spatial, cmlpl_loss_phase1_g, cmlpl_loss_phase2_g,
 * cmlpl_backward_data, cmlpl_backward_weights and cmlpl_adam_step launch, captured once per stage with every per-step
 * scalar read from the cmlpl_dyn table (as a captured cmlpl_train_step does).  The backward-weights stage advances the
 * cursor (its reduce launch), the update stage reads the finished step's row.  Batches by index only (d_lab_idx /
 * d_unl_idx: this rank's slice starts at the row's lab_off / unl_off); in-kernel random streams only.  Launch / destroy a
 * stage's graph with cmlpl_step_graph_launch / cmlpl_step_graph_destroy. */
typedef struct cmlpl_dist_io {
  cmlpl_batch batch;            /* this rank's rows (bt, btu PER RANK), by index (ABI 6: split-fed or cube-fed)     */
  cmlpl_shard shard;            /* this rank's place in the global batch                                           */
  cmlpl_gathered gathered;      /* the gathered embeddings / labels and this rank's logits                          */
  cmlpl_banks banks;            /* (ptr[] unused: the table carries the pointers)                                  */
  float* d_params; float* d_m; float* d_v; float* d_packed;   /* [2][param_total] / [2][packed_total]              */
  float* d_grads; int64_t grad_stride;                         /* the gradient bucket, [2][grad_stride]             */
  float* d_logits_l; float* d_feat_l; float* d_labels_f;       /* this rank's logits; its block of the exchange buffer */
  float* d_dlogits; float* d_dfeat;                            /* [2][n_l][K], [2][n_l][1024]                        */
  float* d_probs_l; const float* d_probs_g; int32_t probs_shard_rows; int32_t reserved;
  float* d_scalars;             /* ring base [hist_rows][16]: the row comes from the table                          */
  float* d_dfeat_w_partial;     /* [btu_g][1024]                                                                    */
  void* d_workspace; size_t workspace_bytes;                   /* cmlpl_workspace_bytes(shape, 2, n_l, Q)           */
  void* d_loss_workspace; size_t loss_workspace_bytes;         /* cmlpl_loss_workspace_bytes                        */
  uint64_t seed;
  cmlpl_dyn* d_dyn_table; int32_t* d_dyn_cursor;
} cmlpl_dist_io;
enum { CMLPL_STAGE_SPECTRAL = 0, CMLPL_STAGE_SPATIAL = 1, CMLPL_STAGE_PHASE1 = 2, CMLPL_STAGE_PHASE2 = 3,
       CMLPL_STAGE_BACKWARD_DATA = 4, CMLPL_STAGE_BACKWARD_WEIGHTS = 5, CMLPL_STAGE_UPDATE = 6 };
int cmlpl_dist_stage_graph_create(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_dist_io* io, int stage,
                                  void* stream, void** graph_out);

/* The SHARDED step as ONE call: the seven stages above, eagerly, with the four collectives issued between them from
 * inside (train.py:150-278 for a rank's shard; the staging of cmlpl_amd/distributed.py's drive_step: embedding
 * all-gather asynchronously behind the spectral stage and waited for in front of phase 1, probability all-gather,
 * reduce-scatter of d_dfeat_w_partial into net 1's unlabelled rows of d_dfeat asynchronously behind phase 2 and waited
 * for in front of the backward-weights stage, all-reduce of the gradient bucket).  A rank's step driven stage by stage
 * from Python is bound by the host (profiles/r06_dist_trace_b2_64.txt); this entry point is ~25 enqueues back to back.
 *   io    : as for the stage graphs, with d_dyn_table = d_dyn_cursor = NULL (scalars by value: `args`); batch by rows
 *           or by index, noise8 / banks.ptr[] as in the eager stage calls; d_labels_f must follow d_feat_l directly (the
 *           rank's block of the exchange buffer [2*n_l*1024 feat | bt_l labels] is sent as one piece), gathered.
 *           d_logits_local == d_logits_l, probs_shard_rows == btu_local; d_scalars = ring base, row args->scalars_row.
 *   coll  : the rank's communicator as three C functions over float32 buffers (sum), the side stream the two
 *           asynchronous exchanges run on and four hipEvent_t created with hipEventDisableTiming (side_stream NULL:
 *           all four collectives in order on `stream`, no events).  Each function
 *           enqueues on `stream` and returns 0 or an error code.  cmlpl_rccl_bind fills one from an initialised
 *           ncclComm_t and the path of the librccl.so the process uses (dlopen: this library does not link RCCL; it
 *           also creates the side stream and the events); _unbind frees what _bind made (not the ncclComm_t).
 *           NULL = one rank whose exchange buffers alias its own blocks (d_recv_feat == d_feat_l, d_probs_g ==
 *           d_probs_l, d_dfeat_w_partial == d_dfeat + (n_l + bt_l) * 1024): no collective is issued. */
typedef struct cmlpl_collectives {
  void* ctx;
  int (*all_gather)(void* ctx, const float* send, float* recv, size_t send_count, void* stream);
  int (*reduce_scatter)(void* ctx, const float* send, float* recv, size_t recv_count, void* stream);
  int (*all_reduce)(void* ctx, float* buf, size_t count, void* stream);
  void* side_stream;            /* hipStream_t */
  void* events[4];              /* hipEvent_t  */
} cmlpl_collectives;
typedef struct cmlpl_dist_step_args {
  uint64_t step;                /* counter of the in-kernel random streams                                          */
  int64_t adam_t;               /* 1-based                                                                          */
  const float* d_dropmask;      /* NULL = Philox mask; else this rank's [2][n_l][cls_in]                            */
  int32_t smooth; float adap_mask;
  int32_t apply_update;         /* 0 = stop after the gradient all-reduce                                           */
  int32_t scalars_row;
} cmlpl_dist_step_args;
int cmlpl_rccl_bind(const char* librccl_path, void* nccl_comm, cmlpl_collectives* out);
int cmlpl_rccl_unbind(cmlpl_collectives* coll);
int cmlpl_dist_step(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_dist_io* io,
                    const cmlpl_dist_step_args* args, const cmlpl_collectives* coll, void* stream);

/* Caller-side row N3: w x w patch windows gathered on device from the z-scored / PCA'd
 * scene cube instead of materialising XP.npy (tools/hyper_tools.py:35-55 MirrowCut, :226-243
 * ExtractPatches; for PaviaU that tensor is 19.9 GB).  d_cube [rows][cols][C] f32, d_pixel_idx int64 [n]
 * row-major pixel indices, d_out [n][C][w][w].  Exact (pure gather).  Even w reproduces the reference;
 * odd w (which the reference cannot run) is the centred generalisation. */
int cmlpl_extract_patches(const float* d_cube, int rows, int cols, int C, int w,
                          const int64_t* d_pixel_idx, int n, float* d_out, void* stream);

/* Caller-side rows N1 x N3 joined: whole-image inference straight from the scene cube
 * (tools/hyper_tools.py:416-437 test_whole over the patches of :226-243 ExtractPatches; train.py:291-294).  One network,
 * eval mode (no dropout): pixels pixel0 .. pixel0 + n - 1 (row-major) of d_cube [rows][cols][C] f32 (band-last, the
 * z-scored / PCA'd scene) with window shape->H == shape->W, their spectra d_spectra [rows * cols][bands] (row pixel0 + i
 * is read for pixel i).  The fused forward gathers each window through the mirror index while it stages its slab: no
 * patch tensor exists in HBM.  d_labels [n] int64 = argmax of the logits (first maximum, NaN first: torch.max);
 * d_logits [n][K] optional (null: not written).  d_params / d_packed: ONE network's flat parameters and packed weights
 * (cmlpl_layout / cmlpl_pack_weights with nets = 1).  Workspace: cmlpl_infer_workspace_bytes(shape, n) -- which is 0 for
 * a shape this entry point does not take.
 * Returns CMLPL_E_SHAPE for windows the per-sample forward does not take (more than 256 window pixels, final pooled
 * maps of more than 12 pixels: extract patches and use cmlpl_basenet2_fwd there), CMLPL_E_ARG for a scene with fewer
 * rows or columns than half a window (the mirror index folds once) -- as every error here, before any launch. */
size_t cmlpl_infer_workspace_bytes(const cmlpl_shape* shape, int n);
int cmlpl_infer_cube(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                     int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                     float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream);

/* Validation on a pixel list -- ADDED AFTER ABI 6 WITHOUT A VERSION BUMP: the three entry points below are pure
 * additions (no struct changes size, no existing prototype changes, a binding finds them by symbol), and the version
 * number is what callers built against ABI 6 compare; a binding that needs them checks that the symbols resolve (as
 * cmlpl_amd/_lib.py does: a library without them is refused whole, not half-used).
 *
 * cmlpl_infer_pixels: cmlpl_infer_cube for a LIST of scene pixels and for both networks in one launch chain (the
 * reference's per-epoch test_acc, tools/hyper_tools.py:372-413, needs the labelled test pixels only: 42,776 of PaviaU's
 * 207,400).  Item i is scene pixel d_pix[i] (row-major index into d_cube [rows][cols][C]; any order, repeats allowed); its
 * spectrum is row d_spec_row[i] of d_spectra [.][bands], or row i when d_spec_row is NULL (a split's compact rows).
 * d_spec_row == d_pix with the whole scene's spectra reproduces cmlpl_infer_cube's addressing.  Networks: `nets` (1 or 2)
 * flat parameter / packed-weight blocks param_stride / packed_stride floats apart (cmlpl_layout / cmlpl_pack_weights);
 * d_labels [nets][n] int64, d_logits [nets][n][K] or NULL.  Each item is one workgroup's arithmetic on its own window and
 * row: the results equal cmlpl_infer_cube's at the same pixels bit for bit, whatever the order of the list.
 * The indices are DATA ON THE DEVICE: this call cannot check them without a synchronisation.  The caller checks their
 * range once, where a list is set up (cmlpl_amd.evaluate.Evaluator does); the window gather clamps d_pix[i] into the
 * scene, d_spec_row is used as it is.
 * Workspace: cmlpl_eval_workspace_bytes(shape, nets, n), 0 for a shape this entry point does not take.
 * Returns CMLPL_E_ARG (null pointer, n < 1, nets outside 1..2, rows / cols smaller than half a window, a stride shorter
 * than a network), CMLPL_E_SHAPE (as cmlpl_infer_cube: more than 256 window pixels -- cmlpl_extract_patches takes the same
 * list, cmlpl_basenet2_fwd the patches), CMLPL_E_WORKSPACE -- all before any launch.
 *
 * cmlpl_confusion: d_cm [nets][K][K] int64 += counts of (row = d_truth[i], column = d_pred[net][i]) over i < n; K <= 64.
 * It ACCUMULATES (chunks of a list, the shares of several ranks): hipMemsetAsync starts a fresh matrix.  Items whose
 * truth is outside 0 .. K - 1 are counted in d_ignored[0] (optional, accumulated too) and nowhere else.  Integer atomics:
 * exact, and the same bytes on every run.
 * Neither call synchronises or allocates: both can be captured in a graph. */
size_t cmlpl_eval_workspace_bytes(const cmlpl_shape* shape, int nets, int n);
int cmlpl_infer_pixels(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                       const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                       const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                       int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_confusion(const int64_t* d_pred, int nets, const int64_t* d_truth, int n, int K, int64_t* d_cm,
                    int64_t* d_ignored, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- where the two-piece RANGE FLAG words of one network lie inside
 * its packed block: *off_floats = their offset in floats from the block's start; they run to packed_total (16 floats =
 * 64 bytes, word 0 carries the flag).  A full pack (cmlpl_pack_weights) zeroes them and raises them anew from the
 * current weights; the Adam step's incremental re-pack only ever raises them.  A checkpoint therefore saves these
 * words and ORs them back in behind the full pack that follows a load (cmlpl_amd/checkpoint.py), or a resumed run
 * could take other convolution loops than the run it continues.  Host arithmetic only; CMLPL_E_ARG / CMLPL_E_SHAPE. */
int cmlpl_packed_flag_offset(const cmlpl_shape* shape, int64_t* off_floats);

/* Added after ABI 6, no bump (nothing existing moves) -- the CROSS-PSEUDO-SUPERVISION baseline (reference trian_CPS.py:
 * the same two BaseNet2, augmentation, dropout and Adam; only the loss block differs, :234-250).
 *
 * cmlpl_cps_loss_fwd_bwd: that loss block alone, forward + analytic backward, ONE kernel launch (behind a 4-byte memset).
 *   d_logits [2][n][K]: net 0 = Base ("s"), net 1 = Base1 ("w"); rows [0,bt) labelled, [bt,n) unlabelled; d_labels [bt]
 *   labelled row   : cls = CE(z, Y), dz = (softmax(z) - onehot(Y)) / bt                                    (:234-235)
 *   unlabelled row : t_s = argmax z_w, t_w = argmax z_s -- torch.max's rule as in cmlpl_infer_cube: first maximum, a NaN
 *                    counts as the maximum and the first NaN wins (:238-239); con_s = mean CE(z_s, t_s), con_w = mean
 *                    CE(z_w, t_w); dz_s = w (softmax(z_s) - onehot(t_s)) / btu, dz_w likewise, w = hp->w_mutual (the
 *                    reference's literal is 0.1, :245,248: cmlpl_amd.TrainEngine(method="cps") sets it)
 *   outputs        : d_dlogits [2][n][K]; d_pseudo int64 [2][btu] = {t_s, t_w};
 *                    d_scalars[16] in the slots of cmlpl_loss_fwd_bwd = {0, total_s, cls_s, con_s, acc, total_w, cls_w,
 *                    con_w, 0, btu, btu, 0, 0, AGREE, 0, 0}: total = cls + w con, acc = share of labelled rows net 1
 *                    gets right (:258), AGREE = number of unlabelled rows with t_s == t_w.
 *   No memory bank, no threshold, no contrastive term and NO gradient into the embedding: the backward of a CPS step
 *   takes d_dfeat = NULL (cmlpl_backward's "may be NULL = zero").  The scalar sums are folded in a fixed order (no float
 *   atomics): the same bytes on every run and under graph replay.
 * The whole step (cmlpl_train_step / cmlpl_step_graph_create with cmlpl_step_io.reserved = CMLPL_METHOD_CPS): forward ->
 *   this loss -> backward (d_dfeat NULL) -> Adam.  io->banks are neither read nor written (only banks.Q sizes the
 *   workspace as before), smooth / adap_mask are ignored, d_feat is still written by the forward; under replay the
 *   logging row and the Adam scalars come from the cmlpl_dyn table as for CMLPL.  The step's pseudo-labels lie in the
 *   workspace: cmlpl_debug_region(shape, 2, n, "cps_pseudo").  Another value of `reserved`: CMLPL_E_ARG. */
enum { CMLPL_METHOD_CMLPL = 0, CMLPL_METHOD_CPS = 1 };
size_t cmlpl_cps_loss_workspace_bytes(const cmlpl_shape* shape, int bt, int btu);
int cmlpl_cps_loss_fwd_bwd(const cmlpl_shape* shape, int bt, int btu, const float* d_logits, const int64_t* d_labels,
                           const cmlpl_hparams* hp, float* d_scalars, float* d_dlogits, int64_t* d_pseudo,
                           void* d_workspace, size_t workspace_bytes, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- the EXPONENTIAL MOVING AVERAGE of the weights, the "teacher"
 * (reference tools/models.py:155-164 WeightEMA_BN: Ensemble = Base * (1 - alpha) + Ensemble * alpha).
 *
 * cmlpl_ema_update: d_ema[i] = fl( fl(d_src[i] * oma) + fl(d_ema[i] * a) ) for i < count, a = (float)alpha,
 *   oma = (float)(1.0 - alpha): three separately rounded fp32 operations, never an FMA -- what the reference's two tensor
 *   products and their sum round to, bit for bit.  `alpha` is a DOUBLE because the reference forms 1 - alpha in double
 *   before the product rounds it to fp32: (float)(1.0 - 0.95) and 1.0f - (float)0.95 are three ulps apart, and with the
 *   second the result differs from the reference's in nearly every other element.
 *   One contiguous range, any count, any 4-byte aligned pointers (16-byte accesses where both are aligned alike, single
 *   floats otherwise); d_src == d_ema is allowed (each element is read before it is written); NaN and infinity propagate
 *   as the arithmetic says.  One kernel launch, no atomics, no workspace, no synchronisation, no other host call: it can
 *   be captured in a graph.  count == 0 returns 0 without a launch.  CMLPL_E_ARG: count < 0, alpha outside [0, 1] or not
 *   finite, a null or misaligned pointer with count > 0.
 * cmlpl_amd.TrainEngine(teacher_alpha=) enqueues it over both networks' whole parameter block behind every step that
 * applies its update (and behind every graph replay); cmlpl_amd.models.WeightEMA_BN calls it once per tensor. */
int cmlpl_ema_update(const float* d_src, float* d_ema, int64_t count, double alpha, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- the ENSEMBLE of 1..4 networks' logits: averaged class
 * probabilities, the label they give, its confidence, the entropy and the members' disagreement (the reference has no
 * counterpart: it reports each network alone).
 *
 * cmlpl_ensemble: d_logits holds `members` (1..4) blocks [n][K] f32, member_stride floats apart (>= n K when members > 1;
 *   ignored for one member).  Per pixel i < n:
 *     p_m      = softmax(z_m[i]) in fp32, the maximum subtracted first -- torch.softmax's semantics: a member row that holds
 *                a NaN or a +inf is NaN everywhere, -inf logits give probability 0
 *     p        = sum_m w_m p_m, m ascending; w_m = weights[m] / sum(weights), formed in double and rounded to fp32 on the
 *                host.  `weights` is a HOST array [members], read during the call; NULL = equal weights
 *     label    = the FIRST maximum of p; a NaN counts as the maximum and the first NaN wins (torch.max's rule, as in
 *                cmlpl_infer_cube)                                                        -> d_labels [n] int64
 *     conf     = p[label]                                                                 -> d_conf [n] or NULL
 *     entropy  = -sum_c p_c logf(p_c) with 0 log 0 = 0, NaN when p is NaN                 -> d_entropy [n] or NULL
 *     disagree = the number of members whose own label (the same rule on p_m) is not label -> d_disagree [n] int32 or NULL
 *     p itself                                                                            -> d_probs [n][K] or NULL
 *   One launch: a group of G lanes per pixel (G = the smallest power of two >= K), shuffle butterflies of width G, no LDS,
 *   no atomics, no workspace, no synchronisation, no other host call (it can be captured in a graph); the same bytes on
 *   every run.  CMLPL_E_ARG before any launch: members outside 1..4, K outside 1..64, n < 1, a weight that is negative or
 *   not finite, weights whose sum is not positive, a member_stride below n K with members > 1, a null d_logits / d_labels,
 *   a misaligned pointer. */
int cmlpl_ensemble(const float* d_logits, int members, int64_t member_stride, const float* weights, int n, int K,
                   int64_t* d_labels, float* d_probs, float* d_conf, float* d_entropy, int32_t* d_disagree, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- TEST-TIME AUGMENTATION: prediction from several noisy VIEWS of
 * each pixel, x + sigma N(0,1), the kind of input the networks were trained on (train.py's --m, which the reference parses
 * and never uses).
 *
 * THE DEFINITION OF A VIEW.  View t (0-based) of scene pixel P (row-major index into the cube) under (seed, sigma), in
 * the terms of the generator of csrc/common.hpp (noise_hash / noise_normal4 / noise_normal4p / noise_normal8 / noise_ctr):
 *   window element (window pixel p = i W + j, band b):
 *     x_view = fmaf(z, sigma, x),  z = component (b & 3) of
 *              noise_normal4p(seed, step = t, CMLPL_STREAM_TTA_XP, gsample = P, G),  G = p QP + (b >> 2),
 *              QP = 4 ceil(C / 16)
 *     (bands 8c .. 8c + 7 of one window pixel are ONE hash call -- noise_normal8 with pair G >> 1: the unit of a gather
 *      from the band-last cube.  The training streams key the [C][H][W] element order instead, where eight consecutive
 *      elements are eight pixels of one band.)  G < 2^24 for every window up to 20 x 20 and C up to 256.
 *   spectrum element k:
 *     x_view = fmaf(z, sigma, x),  z = component (k & 3) of
 *              noise_normal4(seed, t, CMLPL_STREAM_TTA_X, noise_ctr(P, k >> 2))
 *   The streams 0x400 / 0x500 are disjoint from the training streams (0x100, 0x200, 0x300, each + net).
 *   A view is a property of (seed, t, P) ALONE: every network scores the same views, and neither the position of P in a
 *   list or chunk nor the kind of launch (pixel range, pixel list, by patches) changes a bit of it.  For a pixel list P is
 *   d_pix[i] clamped into the scene -- also when the spectra are a split's compact rows (d_spec_row == NULL).
 *   sigma == 0 is legal everywhere below and gives the clean window / spectrum, the clean forward's bytes.
 *
 * cmlpl_infer_cube_tta / cmlpl_infer_pixels_tta: cmlpl_infer_cube / cmlpl_infer_pixels on view `view` of every pixel --
 *   the same arguments, results, shapes and errors, plus (sigma, seed, view).  The fused forward adds the view's noise
 *   while it stages its slab from the cube (kernels of their own: the clean launches are untouched); the spectra
 *   get theirs in a small launch into the workspace in front of the spectral branch.  Workspace:
 *   cmlpl_infer_tta_workspace_bytes(shape, n) / cmlpl_eval_tta_workspace_bytes(shape, nets, n) (0: not a shape they take).
 *   CMLPL_E_ARG also for a sigma that is negative or not finite; every error is returned before any launch.
 *
 * cmlpl_tta_patches: cmlpl_extract_patches plus the view's noise -- d_out [n][C][w][w] = view `view` of the windows of
 *   the pixels d_pixel_idx[i] (clamped into the scene), and, when d_spectra_out is not NULL, d_spectra_out [n][bands] =
 *   the view of their spectra: row d_spec_row[i] of d_spectra, or row i when d_spec_row is NULL.  (d_out may be NULL when
 *   only the spectra are wanted; then C and w are not looked at.)  It feeds the by-patches path (windows the fused
 *   forward does not take), and it is the observable form of the definition above.  Errors as cmlpl_extract_patches.
 *
 * cmlpl_ensemble_views: cmlpl_ensemble over members x views logit blocks [n][K] (members >= 1, views >= 1, their product
 *   at most 64): block (m, v) starts at d_logits + m member_stride + v view_stride.
 *     p = sum_m sum_v w_{m,v} softmax(z_{m,v}),  w_{m,v} = fl32(weights[m] / sum(weights) / views), formed in double on the
 *     host; the terms are added m ascending and, within m, v ascending, each with cmlpl_ensemble's per-term operation --
 *     at views == 1 every output equals cmlpl_ensemble's bit for bit.
 *     label, conf, entropy, p as in cmlpl_ensemble; disagree = the number of (member, view) blocks whose own label differs.
 *   The same lane scheme (G lanes per pixel, shuffles only, a run-time loop over the blocks, no LDS, no atomics), the same
 *   bytes on every run.  CMLPL_E_ARG before any launch: what cmlpl_ensemble refuses, members x views outside 1..64, blocks
 *   that overlap (with B = n K: neither  view_stride >= B and member_stride >= views view_stride  nor
 *   member_stride >= B and view_stride >= members member_stride;  a stride whose count is 1 is ignored). */
enum { CMLPL_STREAM_TTA_XP = 0x400, CMLPL_STREAM_TTA_X = 0x500 };
size_t cmlpl_infer_tta_workspace_bytes(const cmlpl_shape* shape, int n);
int cmlpl_infer_cube_tta(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                         int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                         float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream,
                         float sigma, uint64_t seed, uint32_t view);
size_t cmlpl_eval_tta_workspace_bytes(const cmlpl_shape* shape, int nets, int n);
int cmlpl_infer_pixels_tta(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                           const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                           const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                           int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream,
                           float sigma, uint64_t seed, uint32_t view);
int cmlpl_tta_patches(const float* d_cube, int rows, int cols, int C, int w, const int64_t* d_pixel_idx, int n,
                      float* d_out, const float* d_spectra, const int64_t* d_spec_row, int bands, float* d_spectra_out,
                      float sigma, uint64_t seed, uint32_t view, void* stream);
int cmlpl_ensemble_views(const float* d_logits, int members, int views, int64_t member_stride, int64_t view_stride,
                         const float* weights, int n, int K, int64_t* d_labels, float* d_probs, float* d_conf,
                         float* d_entropy, int32_t* d_disagree, void* stream);

/* Added after ABI 6, no bump (no struct and no signature changes) -- SPATIAL AUGMENTATION: flipped and rotated windows
 * for the cube-fed training step and as views of test-time augmentation (the reference's `flip` and `Random_rot`,
 * hsi_loader.py:58-88).  No window tensor appears in HBM: a spatial element is a remap of the window index in front of the
 * source address of the gathers that exist (cube_feed_kernel, the TTA forwards' slab staging, tta_patches_kernel).
 *
 * THE DEFINITION OF A SPATIAL ELEMENT.  An element g in 0..7 of the dihedral group D4 acts on the index grid of a square
 * w x w window `win` -- not on scene offsets: the transformed window is a permutation of the SAME w w scene pixels, for
 * even w too; no other scene pixel is read and the mirror rule of the margin is untouched:
 *     out[ch][i][j] = win[ch][i'][j'],   (a, b) = (g & 4) ? (j, i) : (i, j),
 *                                        i' = (g & 2) ? w - 1 - a : a,
 *                                        j' = (g & 1) ? w - 1 - b : b
 *   g = 0  the window as it is                 g = 4  the transpose
 *   g = 1  flip(-1)  (left-right)              g = 5  the quarter turn rot90(k=1)  (counter-clockwise, numpy / torch)
 *   g = 2  flip(-2)  (up-down)                 g = 6  the quarter turn rot90(k=3) = rot90(k=-1)  (clockwise)
 *   g = 3  the rotation by 180 degrees         g = 7  the anti-transpose
 *   Modes: CMLPL_SYM_NONE  S = 1 (g = 0);  CMLPL_SYM_FLIPS  S = 4, g in 0..3 (the four outcomes of the reference's `flip`);
 *          CMLPL_SYM_D4  S = 8 (what `flip` after `Random_rot` generates).
 *   Noise is added AFTER the remap and stays keyed by the OUTPUT position, so no noise stream moves:
 *     training  x = fmaf(z, sigma, win[T_g(p)]) with the counters of the patch noise as they are;
 *     a view    the z of window pixel p = i W + j of "THE DEFINITION OF A VIEW".
 *   The spectrum of a row or of a view is not touched.
 *   TRAINING.  The row with GLOBAL sample index gs at step counter `step` (the cmlpl_dyn row's in a graph replay) takes
 *     g = (noise_hash(seed, step, CMLPL_STREAM_SYM, noise_ctr(gs, 0)).x >> 29) & (S - 1)
 *   (the TOP three bits of the word: noise_ctr leaves the low 24 bits of the counter zero, and the low bits of a pcg4d word
 *   depend on the low bits of its inputs alone -- `.x & (S - 1)` is one element for 256 consecutive samples)
 *   -- the same for both networks (they see one geometry and differ in noise and dropout, as the reference's two networks
 *   read one window), a property of the global sample and so independent of sharding.  The mode travels in
 *   cmlpl_step_io.reserved, bits 8..9 (cmlpl_train_step, cmlpl_step_graph_create); any bit above 9, a mode of 3, or a mode
 *   with d_cube == NULL: CMLPL_E_ARG.  The sharded step (cmlpl_dist_step) does not take it.
 *   TEST-TIME AUGMENTATION.  cmlpl_infer_cube_tta_sym / cmlpl_infer_pixels_tta_sym / cmlpl_tta_patches_sym: the functions
 *   without _sym plus a trailing element `sym`; those are these with sym = 0.  sigma == 0 with sym != 0 is a view of its
 *   own, pure geometry (sigma == 0 with sym == 0 stays the clean forward's launches and bytes).  sym > 7: CMLPL_E_ARG;
 *   H != W with sym & 4: CMLPL_E_SHAPE; both before any launch.  The workspace sizes are those of the functions without
 *   _sym. */
enum { CMLPL_STREAM_SYM = 0x600 };
enum { CMLPL_SYM_NONE = 0, CMLPL_SYM_FLIPS = 1, CMLPL_SYM_D4 = 2 };
int cmlpl_infer_cube_tta_sym(const cmlpl_shape* shape, const float* d_params, const float* d_packed, const float* d_cube,
                             int rows, int cols, const float* d_spectra, int64_t pixel0, int n, int64_t* d_labels,
                             float* d_logits, void* d_workspace, size_t workspace_bytes, void* stream,
                             float sigma, uint64_t seed, uint32_t view, uint32_t sym);
int cmlpl_infer_pixels_tta_sym(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                               const float* d_packed, int64_t packed_stride, const float* d_cube, int rows, int cols,
                               const float* d_spectra, const int64_t* d_spec_row, const int64_t* d_pix, int n,
                               int64_t* d_labels, float* d_logits, void* d_workspace, size_t workspace_bytes,
                               void* stream, float sigma, uint64_t seed, uint32_t view, uint32_t sym);
int cmlpl_tta_patches_sym(const float* d_cube, int rows, int cols, int C, int w, const int64_t* d_pixel_idx, int n,
                          float* d_out, const float* d_spectra, const int64_t* d_spec_row, int bands, float* d_spectra_out,
                          float sigma, uint64_t seed, uint32_t view, void* stream, uint32_t sym);

/* ABI 5 -- the scene itself (reference sample_generation.py:21-73 -> tools/hyper_tools.py:285-292 SampleGen): the z-scored
 * PCA cube the two calls above read, and the z-scored spectra, computed on the device from the raw scene in fp64 as numpy
 * computes them.  d_raw [pixels][bands] row-major in its .mat dtype (CMLPL_SCENE_*, converted exactly to fp64 in the
 * kernels), bands <= 256, pixels >= 2.  Two calls with the host between them:
 *   cmlpl_scene_gram:    d_mean [bands] = mean over the pixels; d_gram [bands][bands] = (X - mean)^T (X - mean)
 *                        (np.cov of the reference's PCANorm is d_gram / (pixels - 1));
 *   -- the caller takes U = svd(d_gram / (pixels - 1))[0] on the host (the reference's LAPACK call, so its signs) --
 *   cmlpl_scene_project: P = (X - mean) d_basis, d_basis = U[:, :n_pc] [bands][n_pc] row-major fp64;
 *                        d_cube [pixels][n_pc] f32 = fp32((P - mean(P)) / std(P)) per component (featureNormalize(., 1),
 *                        population std); d_spectra [pixels][bands] fp64 = (X - mean) / std(X) (optional: NULL = not
 *                        written), std(X)_b = sqrt(d_gram[b][b] / pixels).
 * Both products on v_mfma_f64_16x16x4_f64.  Deterministic: fixed pixel chunks, partials folded in a fixed order, no
 * atomics -- the same scene gives a bit-identical cube on every run and device, whatever its dtype holds the values.
 * Workspace: cmlpl_scene_workspace_bytes(pixels, bands, n_pc) covers both calls (0: a shape the calls do not take). */
enum { CMLPL_SCENE_U16 = 0, CMLPL_SCENE_I16 = 1, CMLPL_SCENE_F32 = 2, CMLPL_SCENE_F64 = 3 };
size_t cmlpl_scene_workspace_bytes(int64_t pixels, int bands, int n_pc);
int cmlpl_scene_gram(const void* d_raw, int dtype, int64_t pixels, int bands, double* d_mean, double* d_gram,
                     void* d_workspace, size_t workspace_bytes, void* stream);
int cmlpl_scene_project(const void* d_raw, int dtype, int64_t pixels, int bands, const double* d_mean,
                        const double* d_gram, const double* d_basis, int n_pc, float* d_cube, double* d_spectra,
                        void* d_workspace, size_t workspace_bytes, void* stream);

/* Caller-side row N4: tools.models.ContrastiveLoss (tools/models.py:14-39) -- NT-Xent over the
 * pairwise cosine similarity of the 2B normalised embeddings, forward + analytic backward.
 * d_emb_i, d_emb_j [B][D]; d_loss [1]; d_grad_i, d_grad_j [B][D] = dLoss/d emb.
 * CMLPL_E_ARG for a batch no kernel holds (cmlpl_debug_ntxent_plan tells), before anything is launched. */
size_t cmlpl_ntxent_workspace_bytes(int B, int D);
int cmlpl_ntxent_fwd_bwd(const float* d_emb_i, const float* d_emb_j, int B, int D, float temperature,
                         float* d_loss, float* d_grad_i, float* d_grad_j,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * loss_helper.py of the reference.  The reference keeps one FIFO per class as a Python list
 * of tensors; here a class's bank is a physical ring d_bank[c][capacity_stride][D] (capacity[c] slots used) with
 * d_state[c] = {rows, head}:
 * LOGICAL row i (what loss_helper.py's queue[0][i] holds) is ring slot (head + i) % capacity.
 * ---------------------------------------------------------------------------------------------- */

/* compute_unsupervised_loss (loss_helper.py:242-261): rows whose teacher entropy reaches the `percent`-th percentile
 * (numpy 'linear') of the valid rows are set to 255 IN d_target; d_loss[0] = (B / kept) * mean-over-kept CE;
 * d_dpredict [B][K] = d loss / d predict.
 * Nothing kept -- percent = 0 (every valid row reaches the threshold) or a batch whose rows are all 255 on entry: every
 * row of d_target is 255 afterwards, d_dpredict is zero everywhere and d_loss[0] is not finite (B / 0 times 0 / 0, like
 * the reference); the call returns 0.  All three forms of the computation (cmlpl_debug_unsup_plan) give this answer. */
size_t cmlpl_unsup_workspace_bytes(int B);
int cmlpl_unsup_loss(const float* d_predict, int64_t* d_target, const float* d_pred_teacher, int B, int K,
                     double percent, float* d_loss, float* d_dpredict, void* d_workspace, size_t workspace_bytes,
                     void* stream);

/* Per-class selection of compute_contra_memobank_loss (loss_helper.py:67-123).  d_prob / d_label [N][K] are the
 * labelled rows followed by the unlabelled ones (n_labeled first), masks [N].  d_lists [K][3][N] receives, in row
 * order: 0 low_valid rows, 1 low-entropy anchor pool, 2 negative-key rows; d_counts [K][3] their lengths. */
int cmlpl_memobank_select(const float* d_prob, const float* d_label, const float* d_low_mask, const float* d_high_mask,
                          int N, int n_labeled, int K, int32_t* d_lists, int32_t* d_counts, void* stream);
/* class prototypes (loss_helper.py:102-106): d_proto[c] = mean of d_rep_teacher over list 0 (NaN when empty) */
int cmlpl_memobank_proto(const float* d_rep_teacher, int N, int D, int K, const int32_t* d_lists,
                         const int32_t* d_counts, float* d_proto, void* stream);
/* dequeue_and_enqueue (loss_helper.py:19-36, call site :126-133) for every class: list 2 of d_rep_teacher is appended,
 * the last d_capacity[c] rows survive (queue_size may differ per class; class c's ring starts at
 * d_bank + c * capacity_stride * D) */
int cmlpl_memobank_enqueue(const float* d_rep_teacher, int N, int D, int K, const int32_t* d_lists,
                           const int32_t* d_counts, float* d_bank, int32_t* d_state, const int32_t* d_capacity,
                           int capacity_stride, void* stream);
/* dequeue_and_enqueue for one class with the keys given directly */
int cmlpl_memobank_push(const float* d_keys, int m, int D, float* d_bank_c, int32_t* d_state_c, int capacity,
                        void* stream);
/* one loop position of loss_helper.py:158-215: `queries` anchors rep[d_pool[d_anchor_draw[q]]], key 0 =
 * d_pos + q * pos_qstride, keys 1.. = logical bank rows d_neg_draw[q][j]; cosine similarity / temperature, CE with
 * target 0.  d_lossq[q] = scale * CE_q / queries; d_ganchor [queries][D]; if d_drep is given the anchor gradients
 * are added into it (rows drawn repeatedly are summed in query order: deterministic).  Indices must be in range. */
int cmlpl_memobank_infonce(const float* d_rep, int N, int D, const int32_t* d_pool, int pool_rows,
                           const int64_t* d_anchor_draw, const float* d_pos, int64_t pos_qstride,
                           const float* d_bank_c, int capacity, int bank_rows, int head, const int64_t* d_neg_draw,
                           int queries, int negatives, float temperature, float scale, float* d_lossq,
                           float* d_ganchor, float* d_drep, void* stream);
/* compute_contra_memobank_loss (loss_helper.py:39-219) in ONE pass -- three launches, no host read-back: selection +
 * prototypes + enqueue per class; the InfoNCE of every (query, loop position) with the valid-class bookkeeping done
 * on device from the counts; anchor-gradient scatter + loss sum.  d_* outputs:
 *   d_lists [K][3][N] i32, d_counts [K][3] i32, d_proto [K][D]: as cmlpl_memobank_select / _proto
 *   d_keys_log [K][2] i32 (optional): (new keys, rows after) per class, for the caller's pointer bookkeeping
 *   d_lossq [K][queries], d_ganchor [K][queries][D], d_arow [K][queries] i32: per (position, query) scratch
 *   d_drep [N][D]: d loss / d rep (written in full);  d_total [1]: the loss
 * Draws: d_anchor_draw [K][queries] / d_neg_draw [K][queries*negatives] int64 indexed by LOOP POSITION replace the two
 * torch.randint calls (:164,:179) -- entries must be in range for the positions that exist; NULL = drawn in-kernel
 * (Philox keyed by seed / call).  d_momentum [K][queries][D] + d_momentum_on (device int: "not all zero", :196) +
 * ema select the prototype blend of :194-203; then d_prototype [K][queries][D] receives `prototype`.
 * Limits: K <= 1024, negatives <= 127, K * queries <= 16384 (the scatter keeps one int per (position, query) slot in
 * 64 KiB of LDS; K = 64 at queries = 256 is exactly the limit and runs).  A call outside them returns CMLPL_E_ARG
 * BEFORE anything is launched: d_bank, d_state and every output are untouched (cmlpl_debug_memobank_plan tells). */
typedef struct cmlpl_memobank_call {
  const float* d_rep; const float* d_rep_teacher;
  const float* d_prob_l; const float* d_prob_u; const float* d_label_l; const float* d_label_u;
  const float* d_low_mask; const float* d_high_mask;
  int32_t N, n_labeled, K, D, queries, negatives;
  float* d_bank; int32_t* d_state; const int32_t* d_capacity; int32_t capacity_stride;
  const int64_t* d_anchor_draw; const int64_t* d_neg_draw; uint64_t seed, call;
  const float* d_momentum; const int32_t* d_momentum_on; float ema; float* d_prototype;
  float temperature;
  int32_t* d_lists; int32_t* d_counts; float* d_proto; int32_t* d_keys_log;
  float* d_lossq; float* d_ganchor; int32_t* d_arow; float* d_drep; float* d_total;
} cmlpl_memobank_call;
int cmlpl_memobank_loss(const cmlpl_memobank_call* call, void* stream);

/* fixed-order sum of n floats (the loss of all loop positions) */
int cmlpl_memobank_sum(const float* d_v, int n, float* d_out, void* stream);


/* Optional per-launch timing, measured with hipEvent pairs recorded on the launch stream around the
 * selected kernels (bit i of kernel_mask selects CMLPL_K_i).  cmlpl_timing_end synchronises the
 * recorded events and returns, per kernel id, the summed milliseconds and the number of launches.
 * This is the only process-global state in the library; it is off unless _begin was called. */
enum {
  CMLPL_K_AUGMENT = 0, CMLPL_K_CONV0_FWD, CMLPL_K_CONV1_FWD, CMLPL_K_CONV2_FWD, CMLPL_K_SPE_FWD,
  CMLPL_K_HEAD_FWD, CMLPL_K_LOSS, CMLPL_K_HEAD_BWD, CMLPL_K_CLS_WGRAD, CMLPL_K_SPE_WGRAD,
  CMLPL_K_CONV2_DGRAD, CMLPL_K_CONV2_WGRAD, CMLPL_K_CONV2_WRED, CMLPL_K_CONV1_DGRAD, CMLPL_K_CONV1_WGRAD,
  CMLPL_K_CONV1_WRED, CMLPL_K_CONV0_WGRAD, CMLPL_K_ADAM, CMLPL_K_PACK, CMLPL_K_LOSS2, CMLPL_K_LOSS_FIN,
  CMLPL_K_LOSS_DFEAT, CMLPL_K_CUBE_FEED /* ABI 6: the cube-fed step's gather + augment launch */,
  CMLPL_K_CPS_LOSS /* after ABI 6: the CPS loss launch */, CMLPL_K_COUNT
};
int cmlpl_timing_begin(uint32_t kernel_mask, int max_launches);
int cmlpl_timing_end(double* ms_sum /*[CMLPL_K_COUNT]*/, int64_t* launches /*[CMLPL_K_COUNT]*/);

/* Inspection aid (tests, debugging): byte offset and size inside d_workspace of a saved
 * activation of cmlpl_basenet2_fwd/_bwd for (nets, n).  Names: "a0" conv0 output
 * [nets][n][H*W][64] f32; "p1"/"p2" pooled stage outputs [nets][n][P][64] f32; "m1"/"m2" ReLU
 * masks [nets][n][P][64] u8 (bit (h&1)*2+(w&1) = relu(z) > 0 at that pixel of the 2x2 pool
 * window); "y" spectral ReLU output [nets][n][1024] f32; "catd","dropgen" [nets][n][cls_in];
 * "dy","dp2","dp1","da0" backward intermediates; with nets = 2 also "xn": the augmented patch rows [2][n][C*H*W] a
 * step's forward keeps for its backward (cmlpl_forward / cmlpl_train_step); "cps_pseudo": a CPS step's hard labels,
 * int64 [2][btu] at the region's start; "probs": the probability region of cmlpl_train_step, 4 n K floats, of which a
 * CMLPL step fills the front as [4][btu][K] = p_w, p_s (both smoothed once the gate is open), p_w0, p_s0 (the plain
 * softmaxes) -- what cmlpl_pl_stats reads.  Returns CMLPL_E_ARG for an unknown name. */
int cmlpl_debug_region(const cmlpl_shape* shape, int nets, int n, const char* name,
                       size_t* byte_offset, size_t* bytes);

/* Test aid: read the CMLPL_* planner switches from the environment again (they are otherwise read once per
 * process).  Lets ONE test process walk several kernel variants; call it between library calls only -- objects
 * created under the old settings (captured graphs, engines with cached plans) must not be used afterwards.
 * The reference has no counterpart (it has no native code). */
int cmlpl_debug_reload_switches(void);

/* Measurement aid (bench.py's roofline accounting): which products of a step on `nets` networks x n rows run as TWO
 * fp16 pieces (three MFMAs per product) under the current switches -- bit 0: conv1's forward tap loop, bit 1: conv1's
 * data-gradient tap loop, bit 2: both weight gradients, bit 3: conv2's forward and data-gradient tap loops (general
 * path only).  What the planners decide; a sample or network outside the scheme's ranges still takes the three-piece loop
 * at run time.  Negative: CMLPL_E_*. */
int cmlpl_debug_two_piece(const cmlpl_shape* shape, int nets, int n);

/* Added after ABI 6, no bump (nothing existing moves).  Test aid: what the planner of the general 3x3 kernels decides, under the current switches, for one launch of a step on
 * `nets` networks x n rows -- map 0: the window (conv1), 1: its pooled map (conv2); mode 0: forward, 1: data gradient.
 * out3[0] = samples per workgroup, out3[1] = pixel tiles per wave (0: the one-tile kernel whose four waves split the
 * channel halves), out3[2] = waves per workgroup.  The plan exists whether or not a fused per-sample kernel takes the
 * launch instead.  Host arithmetic only.  CMLPL_E_ARG / CMLPL_E_SHAPE (no plan: the map does not fit). */
int cmlpl_debug_conv3_plan(const cmlpl_shape* shape, int nets, int n, int map, int mode, int* out3);

/* Added after ABI 6, no bump (nothing existing moves).  Test aid: the route of a forward and a backward on `nets`
 * networks x n rows under the current switches -- which kernels run, decided once per call and read by everything
 * that launches.  out[CMLPL_ROUTE_INTS]:
 *   [0] forward regime   0 = A the whole sample in one launch, 1 = B conv0 + conv1 fused, 2 = C one launch per stage
 *   [1] backward regime  0 = A the data-gradient chain in one launch, 1 = B conv1 data gradient + conv0 weight gradient
 *                        fused, 2 = C one launch per stage
 *   [2] 1 when a per-sample launch is an eight-tile kernel (windows of 129 .. 256 pixels)
 *   [3..5], [6..8] the per-sample forward / backward launch of regime A or B: waves, pixel tiles per wave, 1 = conv1's
 *                        tap loop on two fp16 pieces (zeros in regime C)
 *   [9 + 5 i ..] i = 0 .. 3: the general plan of conv1 forward, conv1 data gradient, conv2 forward, conv2 data gradient
 *                        as cmlpl_debug_conv3_plan's three, then 1 = the barrier-free tap loop, 1 = two fp16 pieces
 *   [29] 1 when the step's launches write the per-sample maxima its two-piece weight gradient scales by
 * Host arithmetic only.  CMLPL_E_ARG / CMLPL_E_SHAPE (a map does not fit). */
#define CMLPL_ROUTE_INTS 30
int cmlpl_debug_route(const cmlpl_shape* shape, int nets, int n, int* out);

/* Added after ABI 6, no bump (nothing existing moves).  Test aid: what the planner of the two 3x3 weight gradients
 * (plan_wgrad3_both, asked as a backward pass asks it) decides for `nets` networks x n rows under the current switches.
 * out[CMLPL_WGRAD3_PLAN_INTS]:
 *   [0..6], [7..13]  the window's map (conv1), then its pooled map (conv2):
 *                      [0] column pairs per row (the row-split kernels' template parameter CPR; 0 = the general kernel)
 *                      [1] 1 = the split-bf16 kernel (0 with [0] > 0: the f32-input row-split kernel)
 *                      [2] U: pooled rows per stage (general kernel: units per pass)
 *                      [3] UPG: pooled rows per workgroup, a multiple of U (0 for the general kernel)
 *                      [4] G: workgroups per network (and per kernel row in the row-split kernels)
 *                      [5] dynamic LDS bytes of the map's plan, plus the sample list's bytes when [15] is set
 *                      [6] 2 = the general kernel with its output channels split over two workgroups, else 1
 *   [14] 1 = both maps in ONE launch (the pair kernel)
 *   [15] 1 = the pair launch would place the list of samples with a non-zero gradient image (zero samples are skipped)
 *   [16] the compute-unit count the plans were made for
 * Host arithmetic only, nothing is launched.  CMLPL_E_ARG / CMLPL_E_SHAPE. */
#define CMLPL_WGRAD3_PLAN_INTS 17
int cmlpl_debug_wgrad3_plan(const cmlpl_shape* shape, int nets, int n, int* out);

/* Added after ABI 6, no bump (nothing existing moves).  Test aid: what the planner of the loss block's first launch
 * (plan_loss_phase1, the one function launch_loss_phase1 obeys) decides under the current switches for a shard of the
 * batch (one GPU: {bt, btu, 0, bt, 0, btu}), K classes, banks of `bank_rows` rows and the smoothing gate `smooth`, read
 * from plain buffers (the sharded step's packed buffers add one condition to [6]: a local labelled row count that is a
 * multiple of 4).  out[CMLPL_LOSS_PLAN_INTS]:
 *   [0] the kernel of the three exp(f . f^T / T) products: 0 = pair_exp16_kernel (16 x 32 tiles), 1 = pair_exp_kernel
 *       (32 x 32 tiles; the only narrow kernel for K > 32), 2 = pair_exp_tall_kernel (128 x 32), 3 = pair_exp_wide_kernel
 *   [1], [2] the wide kernel's template parameters MB (2 or 4 row blocks) and NBW (column blocks per wave), else 0, 0
 *   [3], [4] grid x and y (z is 3: the three products)
 *   [5] 32-column tiles of the widest product
 *   [6] 1 = the shape allows the feature-gradient GEMMs their operands through LDS (rows in whole 16-byte pieces)
 *   [7] 1 = [6] and CMLPL_DFEAT_LDS does not forbid it: that launch runs when the call's pointers are 16-byte aligned
 *   [8] the compute-unit count the plan was made for
 * Host arithmetic only, nothing is launched.  CMLPL_E_ARG (what cmlpl_loss_fwd_bwd refuses) / CMLPL_E_SHAPE. */
#define CMLPL_LOSS_PLAN_INTS 9
int cmlpl_debug_loss_plan(const cmlpl_shape* shape, const cmlpl_shard* shard, int bank_rows, int smooth, int* out);

/* Added after ABI 6, no bump (nothing existing moves).  Test aids: what the launchers of cmlpl_unsup_loss and
 * cmlpl_memobank_loss (plan_unsup / plan_mb_onepass, the functions they obey) decide under the current switches.
 * cmlpl_debug_unsup_plan, out[CMLPL_UNSUP_PLAN_INTS]:
 *   [0] 0 = one workgroup (us_onewg_kernel: B <= 1024, or B <= 8192 under CMLPL_UNSUP_3L=0 with up to eight rows per
 *       thread), 1 = three launches (us_entropy2 / us_select1 / us_apply: 1024 < B <= 8192), 2 = the five rank-counting
 *       launches (B > 8192, or every B under CMLPL_UNSUP_ONEWG=0)
 *   [1] 1 = the bodies that hold a row of K <= 16 logits in registers (routes 0 and 1 only), 0 = the per-k loops
 * cmlpl_debug_memobank_plan, out[CMLPL_MEMOBANK_PLAN_INTS]:
 *   [0] the InfoNCE kernel: 0 = mb_infonce_all_kernel (general), NCH = 1 .. 4 = mb_infonce_fast_kernel<NCH> (keys in
 *       registers: D a multiple of 4 and <= 1024, K <= 64, ceil((negatives + 1) / 4) * ceil(D / 256) <= 16, CMLPL_MB_FAST
 *       not 0)
 *   [1] its dynamic LDS bytes   [2] the dynamic LDS bytes of mb_scatter_all_kernel (4 * K * queries)
 * Host arithmetic only, nothing is launched.  CMLPL_E_ARG for what the launcher would refuse. */
#define CMLPL_UNSUP_PLAN_INTS 2
#define CMLPL_MEMOBANK_PLAN_INTS 3
int cmlpl_debug_unsup_plan(int B, int K, int* out);
int cmlpl_debug_memobank_plan(int D, int K, int queries, int negatives, int* out);

/* Added after ABI 6, no bump (nothing existing moves).  Test aid: what the launcher of cmlpl_ntxent_fwd_bwd (plan_ntxent,
 * the one function it obeys) decides under the current switches for B pairs of D floats.  `aligned`: what the call forms
 * from its arguments -- D a multiple of 4 AND both embedding pointers on 16-byte boundaries (a D that is no multiple of 4
 * is never aligned, whatever is passed).  out[CMLPL_NTXENT_PLAN_INTS]:
 *   [0] the gradient kernel: 0 = ntx_grad_kernel (vector: rows that are not whole 16-byte pieces, CMLPL_NTX_MFMA=0, or a
 *       column slice that does not fit LDS), 1 = ntx_grad_mfma_kernel
 *   [1] NCW: 64 NCW embedding columns per workgroup (1 / 2 / 4: the widest that still gives 256 workgroups and fits LDS,
 *       or what CMLPL_NTX_NCW names; 0 on the vector kernel)   [2] KC: embedding rows per staged chunk (64, 32 at NCW = 4;
 *       0 on the vector kernel)   [3] waves per workgroup (4, 8 at NCW = 4)
 *   [4], [5] grid x and y of ntx_sim_kernel (32-column tiles, 16-row tiles)   [6], [7] grid x and y of the gradient launch
 *   [8] the dynamic LDS bytes of the gradient launch   [9] CT: the 32-column tiles whose partial denominators are folded
 * Host arithmetic only, nothing is launched.  CMLPL_E_ARG where no route fits (the vector kernel holds 2B <= 1632 rows,
 * the single-slice MFMA kernel 2B <= 1664): cmlpl_ntxent_fwd_bwd returns the same BEFORE anything is launched, every
 * output keeps its bytes. */
#define CMLPL_NTXENT_PLAN_INTS 10
int cmlpl_debug_ntxent_plan(int B, int D, int aligned, int* out);

/* Added after ABI 6, no bump (nothing existing moves) -- EDGE-PRESERVING SPATIAL SMOOTHING of class probability maps: the
 * probabilities of every class are averaged over a small neighbourhood in which a neighbour counts less the farther away
 * it is and the less its guide vector resembles the centre pixel's (Kang, Li and Benediktsson 2014; the reference has no
 * counterpart: each of its labels is the product of a single window).
 *
 * THE DEFINITION OF A SMOOTHED MAP.  Pixel i = (y, x) of a rows x cols scene; probabilities p[i][c], c < K (d_probs
 * [rows * cols][K], what cmlpl_ensemble / cmlpl_ensemble_views write); guide vectors g[i][0 .. G - 1] = the first G =
 * guide_ch floats at d_guide + i guide_stride (the resident cube [rows][cols][C]: its leading principal components;
 * 0 <= G <= 8, G = 0: no guide, d_guide is not read); radius R, 1 <= R <= 8;
 *   a = fl32(1 / (2 sigma_s^2)),  b = fl32(1 / (2 sigma_r^2)), formed in double on the host from the fp32 arguments;
 *   sigma_r = +inf gives b = 0.
 *     q[i][c] = ( sum_j w_ij p[j][c] ) / ( sum_j w_ij )
 *     w_ij    = exp( -( (dy^2 + dx^2) a + |g_i - g_j|^2 b ) )
 *     j = (y + dy, x + dx),  |dy| <= R,  |dx| <= R,  j INSIDE the scene
 *   Taps outside the scene are left out -- there is no mirror, the normalisation takes care of the border.  The centre
 *   tap has weight exactly 1, so the denominator is >= 1.
 *   The fp32 evaluation, in this order and with these operations (every one rounded once):
 *     taps run dy ascending and, within dy, dx ascending; per tap
 *       d2 = 0;  for ch = 0 .. G - 1 ascending:  d = g_i[ch] - g_j[ch];  d2 = fmaf(d, d, d2)
 *       e  = fmaf(d2, b, fl(s a)),  s = (float)(dy^2 + dx^2) (exact);  w = expf(-e)
 *       den = den + w;  num[c] = fmaf(w, p[j][c], num[c]) for every c
 *     then q[i][c] = num[c] / den (a correctly rounded division).  G = 0 and sigma_r = +inf give the same bits.
 *   A pixel's result is therefore a function of the scene alone: it depends neither on the tile the pixel falls in nor on
 *   the grid, and it is the same bytes on every run.
 *   NaN: a NaN probability of ANY class of a neighbour inside the scene makes the pixel's WHOLE ROW of q NaN (also where
 *   the neighbour's weight has underflowed to 0: 0 x NaN is NaN) -- one NaN row of p spoils exactly the pixels within R
 *   of it, in both directions.  An infinite probability does the same wherever its weight is 0.
 *   From q, by cmlpl_ensemble's rules: label = the FIRST maximum of q, a NaN counts as the maximum and the first NaN wins
 *   (a NaN row: 0); conf = q[label]; entropy = 0 - sum_c t_c, t_c = q_c logf(q_c) with 0 log 0 = 0, the sum running c
 *   ascending from 0 (one thread owns a pixel's row: no butterfly), NaN when q is NaN.
 *
 * cmlpl_smooth_probs: one launch of that definition.  d_out_probs [rows * cols][K] (or NULL) = q; d_labels [rows * cols]
 *   int64, d_conf, d_entropy [rows * cols] (each or NULL).  The filter is NOT in place: d_out_probs must not overlap
 *   d_probs (several passes ping-pong two buffers).  A workgroup stages a tile of 32 x 8 pixels and its halo once into
 *   LDS, channel-planar, and every thread walks the taps of its pixel with up to 16 classes in registers (K > 16: chunks
 *   of 16 over the guide staged once); no atomics, no workspace, no synchronisation (it can be captured in a graph once
 *   an eager call has set the kernels' LDS attribute).
 *   CMLPL_E_ARG before any launch: K outside 1..64, radius outside 1..8, guide_ch outside 0..8, rows or cols < 1 (or
 *   rows * cols past 2^31 - 1); guide_ch > 0 with a null d_guide or guide_stride < guide_ch; sigma_s not finite or <= 0;
 *   sigma_r <= 0 or NaN; a sigma so small that a or b is not finite in fp32; a null d_probs; d_out_probs and d_labels both
 *   null; a misaligned pointer; d_out_probs overlapping d_probs. */
int cmlpl_smooth_probs(const float* d_probs, const float* d_guide, int64_t guide_stride, int guide_ch,
                       int rows, int cols, int K, int radius, float sigma_s, float sigma_r,
                       float* d_out_probs, int64_t* d_labels, float* d_conf, float* d_entropy, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- the PSEUDO-LABEL MONITOR: a step's targets scored against the
 * truth of its unlabelled rows (the reference's loader carries the unlabelled split's labels and never reads them).
 *
 * THE DEFINITION OF THE PSEUDO-LABEL COUNTERS.  The counter block is int64 counts[CMLPL_PL_HEAD + 2 K K].  Every launch
 * ADDS to it and nothing else writes it (the caller zeroes a fresh one).
 *   Direction d = 0 is Base's targets: p = p_w (block 0 of d_probs), p0 = p_w0 (block 2), both made by Base1; direction
 *   d = 1 is Base1's targets: p = p_s (block 1), p0 = p_s0 (block 3).  p is what the step trains against (smoothed over
 *   the memory bank once the gate is open), p0 the plain softmax.
 *   Row r has truth t = d_truth[d_idx ? d_idx[r] : r]; it is KNOWN iff 0 <= t < K.  A row whose truth is not known
 *   contributes nothing anywhere.
 *   counts[8 d + s], per direction:
 *     s = 0 rows      rows with known truth
 *         1 nan_rows  rows where any entry of p[r] or p0[r] is NaN (they count in `rows` and nowhere else)
 *         2 sel       rows with m = 1
 *         3 hit_raw   l0 == t
 *         4 hit       l == t
 *         5 sel_hit   m and l == t
 *         6 fixed     l0 != t and l == t
 *         7 broken    l0 == t and l != t
 *   where, for a NaN-free row, l0 = the FIRST index of the maximum of p0[r], l = the first index of the maximum of p[r],
 *   m = (p[r][l] >= adap_mask) compared in fp32 -- the step's mask.
 *   cm[d][t][l] += 1 for every selected row, at counts[CMLPL_PL_HEAD + (d K + t) K + l].
 *   counts[16 .. 23], over ORDERED pairs (i, j), i != j, both truths known:
 *     16 pairs      pairs considered
 *     17 nan_pairs  q is NaN; the pair counts nowhere else
 *     18 pos        q >= pos_thr
 *     19 pos_same   positive and t_i == t_j
 *     20 neg        q <= neg_thr
 *     21 neg_diff   negative and t_i != t_j
 *     22 launches   launches folded in
 *     23 reserved, stays 0
 *   q = the step's pseudo-label graph entry, in its fp32 evaluation: q = 0; for k ascending: q = fmaf(p_s[i][k],
 *   p_w[j][k], q).  counts[24 .. 31] are reserved and stay 0.
 *   For one step with every truth known and no NaN: sel[0] = n_mask_w, sel[1] = n_mask_s, pos + btu = n_pos (the step
 *   counts its diagonal, which it sets to 1), neg = n_neg -- the step's own logged scalars.
 *   Hard labels (CPS: d_pseudo int64 [2][btu], row 0 = Base's targets): a label outside [0, K) goes to nan_rows; every
 *   other row is selected; hit_raw = hit = sel_hit, fixed = broken = 0; cm as above; no graph part; `launches` counts.
 *
 * cmlpl_pl_stats / cmlpl_pl_stats_hard: one launch each of that definition.  K <= 64, any btu >= 1.  One wavefront per
 *   row (lanes = classes for the row part, lanes striding j for the pair part), counts by ballot and popcount, at most
 *   one 64-bit integer atomic per non-zero head counter and workgroup, one per selected row into cm: integer atomics
 *   only, so the result is exact and independent of the order of arrival.  No workspace, no synchronisation.  d_idx is
 *   followed without a bounds check, as the step follows it.  CMLPL_E_ARG: a null d_probs / d_pseudo / d_truth /
 *   d_counts, btu < 1, K outside 1 .. 64, a misaligned pointer. */
#define CMLPL_PL_HEAD 32
int cmlpl_pl_stats(const float* d_probs /* [4][btu][K] */, int btu, int K, const int64_t* d_truth,
                   const int64_t* d_idx /* or NULL */, float adap_mask, float pos_thr, float neg_thr,
                   int64_t* d_counts, void* stream);
int cmlpl_pl_stats_hard(const int64_t* d_pseudo /* [2][btu] */, int btu, int K, const int64_t* d_truth,
                        const int64_t* d_idx /* or NULL */, int64_t* d_counts, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- CALIBRATION: does a written confidence mean what it says?  The
 * reliability counters of a probability map against the truth of listed pixels, the map at another temperature, and the
 * negative log-likelihood at many candidate temperatures in one launch (temperature scaling: Guo et al., "On Calibration of
 * Modern Neural Networks", ICML 2017).  The reference has no counterpart.
 *
 * THE DEFINITION OF THE RELIABILITY COUNTERS.  The block is int64 counts[CMLPL_REL_HEAD + 3 B] for B bins.  Every launch
 * ADDS to it and nothing else writes it (the caller zeroes a fresh one); chunks of a list, or several launches, sum to the
 * launch over the whole list, bit for bit.
 *   Item i < n scores row r = d_row ? d_row[i] : i of d_probs [rows][K] against t = d_truth[i].
 *   It is KNOWN iff 0 <= t < K; otherwise it counts in `ignored` and nowhere else.
 *   label = the FIRST maximum of the row; a NaN counts as the maximum and the first NaN wins (cmlpl_ensemble's rule).
 *   conf = p[label].  A known row whose conf is NaN (a row that holds a NaN) counts in `nan` and in no bin and no sum.
 *   Every other known row is SCORED: hit = (label == t); its bin is b = min(B - 1, (int)(conf * (float)B)) -- ONE fp32
 *   multiply, truncated: conf == 1 lands in the last bin, conf exactly on an edge k / B in the upper bin k; a product that
 *   is negative goes to bin 0, one >= B (conf > 1, +inf) to bin B - 1.
 *   counts[0] items      n of the launch
 *         [1] known
 *         [2] ignored
 *         [3] nan
 *         [4] hits       scored rows with hit
 *         [5] sum_conf   sum over scored rows of fix24(conf)
 *         [6] sum_nll    sum over scored rows with p[t] > 0 of fix24(nll), nll = -logf(p[t])
 *         [7] n_inf      scored rows with p[t] <= 0: they are kept out of sum_nll
 *         [8] sum_brier  sum over scored rows of fix24(brier), brier = sum_c (p_c - [c == t])^2 in fp32: d_c = p_c - 1 for
 *                        c == t, p_c otherwise; s_c = fl32(d_c d_c) (a product of its own, never fused into the sum), s_c = 0
 *                        for K <= c < G, G the smallest power of two >= K; then the butterfly of cmlpl_ensemble: for o = G / 2,
 *                        G / 4 .. 1: s_c = s_c + s_(c xor o), all c at once; brier = s_0
 *         [9 .. 15]      reserved, stay 0 (CMLPL_REL_HEAD = 16)
 *   counts[16 + b] count[b], counts[16 + B + b] hits[b], counts[16 + 2 B + b] conf_sum[b] = sum of fix24(conf) of bin b.
 *   Every real-valued sum is FIXED POINT: a row contributes fix24(x) = llrintf(x * 2^24), rounded to nearest, ties to even;
 *   the product is exact (a power of two).  For the probabilities this is made for, x <= 104 (the -logf of the smallest
 *   positive fp32 is 103.3; conf <= 1, brier <= 2), so a row adds less than 2^31 and, with n < 2^31 rows, an int64 sum
 *   stays below 2^62: it cannot overflow.  (Rows that are no probabilities are binned as said above; their sums are defined
 *   only while |x| < 2^38.)  So the whole block is integer additions: order-free, exact, the same bytes on every run.
 *
 * cmlpl_reliability: one launch of that definition.  K 1 .. 64, bins 1 .. 1024, n >= 1.  cmlpl_ensemble's lane scheme: a
 *   group of G lanes per item, shuffle butterflies; a workgroup keeps count / hits (int32) and conf_sum (int64) of every bin in
 *   LDS (16 KB at 1024 bins), one LDS atomic each per scored row, then one 64-bit global integer atomic per NON-ZERO word;
 *   the head counts are ballots and popcounts.  (A launch has n < 2^31 items: an int32 cell cannot overflow.)  No float atomics, no
 *   workspace, no synchronisation.  d_row is followed without a bounds check.  CMLPL_E_ARG: a null d_probs / d_truth /
 *   d_counts, n < 1, K outside 1 .. 64, bins outside 1 .. 1024, a misaligned pointer. */
#define CMLPL_REL_HEAD 16
int cmlpl_reliability(const float* d_probs /* [rows][K] */, int K, const int64_t* d_row /* [n] or NULL */,
                      const int64_t* d_truth /* [n] */, int n, int bins, int64_t* d_counts, void* stream);

/* cmlpl_temper_probs: q = softmax(beta log p), that is p^beta renormalised, of every row of d_probs [n][K].  For one
 *   network this is its softmax at temperature T = 1 / beta; for an ensemble, a TTA average or a smoothed map it is the same
 *   operation on the mixture: it is defined behind every stage that produces probabilities.  beta = fl32(1 / T) is formed in
 *   double by the caller.  THE fp32 CHAIN of a row:
 *     l_c = logf(p_c)                     (a zero gives -inf)
 *     m   = max_c l_c
 *     e_c = expf(fl32(beta * fl32(l_c - m)))   (an -inf l_c gives exactly 0)
 *     s   = sum_c e_c in cmlpl_ensemble's butterfly order (e_c = 0 for K <= c < G; for o = G / 2 .. 1: e_c = e_c + e_(c xor o))
 *     q_c = e_c / s
 *   A row with a NaN, a negative entry, a +inf or no positive entry is NaN everywhere.  label = the first maximum of the
 *   INPUT row p under cmlpl_ensemble's rule (a NaN counts as the maximum, the first NaN wins): the chain is monotone, so
 *   q[label] is a maximum of q, and a temperature never moves a label, not even where rounding makes two q_c equal.
 *   conf = q[label]; entropy = -sum_c q_c logf(q_c) (0 log 0 = 0, NaN when q is NaN; the same butterfly).  ANY output pointer may be NULL.  d_out_probs may BE d_probs (in place: a group reads its whole row before it
 *   stores and touches no other row); it may not overlap it otherwise.  One launch in cmlpl_ensemble's lane scheme, no LDS,
 *   no atomics, no workspace; the same bytes on every run, and a row's bytes do not depend on where in the launch it lies.
 *   CMLPL_E_ARG: a null d_probs, n < 1, K outside 1 .. 64, a beta that is not finite or not positive, a misaligned pointer. */
int cmlpl_temper_probs(const float* d_probs, int n, int K, float beta, float* d_out_probs, int64_t* d_labels,
                       float* d_conf, float* d_entropy, void* stream);

/* cmlpl_nll_temps: the negative log-likelihood of the listed pixels at S candidate values of beta = 1 / T, one launch.
 *   Items as in cmlpl_reliability (row r = d_row ? d_row[i] : i against t = d_truth[i]); an item of unknown truth is
 *   skipped (its d_row entry is followed all the same, without a bounds check).  `betas` is a HOST array [S], read during the call (passed on by value, as cmlpl_ensemble's weights); S is
 *   1 .. 64 and every beta lies in [1/16, 16].  A known item is LEFT OUT when p_t is not positive (zero, negative, NaN) or
 *   its row holds a NaN, a negative entry or a +inf; it then counts in d_sums[S + s] for every s.  Every other known item
 *   adds llrintf(nll(beta_s) * 2^20) (to nearest, ties to even; the product is exact) to d_sums[s], where, in fp32,
 *     l_c = logf(p_c), m = max_c l_c,
 *     z   = 0; for c ASCENDING: z = z + expf(fl32(beta * fl32(l_c - m)))
 *     nll = logf(z) - fl32(beta * fl32(l_t - m))          (no product is fused into a sum)
 *   nll < 2^11 (beta <= 16, l_t - m >= -104, logf(z) <= logf(64)), and 2^11 2^20 2^31 = 2^62: the int64 cannot overflow.
 *   d_sums is int64 [2][S]; the launch ADDS to it (the caller zeroes a fresh one), so chunks and launches add up bit for
 *   bit like the reliability counters.  Lanes = candidates, one wavefront per row at a time: lane c < K takes the logf of
 *   class c once for the whole wave, lane s walks its own chain and keeps its int64 in registers over the wave's rows; one
 *   LDS fold per workgroup, one 64-bit global integer atomic per non-zero word.  No float atomics, no workspace.
 *   CMLPL_E_ARG: a null d_probs / d_truth / betas / d_sums, n < 1, K outside 1 .. 64, S outside 1 .. 64, a beta outside
 *   [1/16, 16] (a NaN too), a misaligned pointer. */
int cmlpl_nll_temps(const float* d_probs /* [rows][K] */, int K, const int64_t* d_row /* [n] or NULL */,
                    const int64_t* d_truth /* [n] */, int n, const float* betas /* host, [S] */, int S,
                    int64_t* d_sums /* [2][S] */, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- kNN EVALUATION OF THE SPECTRAL EMBEDDING: the embedding of listed
 * spectra rows, and the weighted kNN classifier of Wu et al. ("Unsupervised Feature Learning via Non-Parametric Instance
 * Discrimination", CVPR 2018, section 3.4) over such rows.  The reference has no counterpart.
 *
 * cmlpl_embed: feat = the 1024-wide L2-normalised output of the spectral branch (tools/models.py:142-146) of item i < n,
 *   whose spectrum is row d_spec_row[i] of d_spectra [.][bands], or row i when d_spec_row is NULL.  `nets` (1 or 2) flat
 *   parameter blocks param_stride floats apart, as cmlpl_infer_pixels takes them; every network reads the same rows.
 *   d_feat [nets][n][1024], d_norm [nets][n] = the row's length before the division -- REQUIRED: a zero there marks a
 *   dead-ReLU row, whose feat row is 0 / 0 = NaN, as everywhere else.  Two launches of kernels that exist (feat_spe + ReLU
 *   from the canonical weights, then the normalisation in place: a thread reads its own four values before it stores them),
 *   no workspace: bit-equal to the feat cmlpl_basenet2_fwd returns in eval mode for the same spectra rows.  d_spec_row is
 *   followed without a bounds check.  CMLPL_E_SHAPE: a shape cmlpl_layout refuses; CMLPL_E_ARG: a null pointer, n < 1, nets
 *   outside 1 .. 2, a stride shorter than a network, a d_feat that is not 16-byte aligned.
 *
 * THE DEFINITION OF A kNN VOTE.  Query rows q_i (i < n) and gallery rows g_j (j < m), 1024 floats each.
 *   Similarity.  s_ij is the dot product of q_i and g_j to fp32 accuracy.  The BITS of s_ij are a function of the two rows'
 *     bytes alone: not of i, j, n, m, the tile, the grid or the run.  (Each row is split once into two fp16 pieces at the
 *     scale 2^12, x 2^12 = hi + lo; the 64 steps of 16 elements run in ascending order, each adding the products lo.hi,
 *     hi.lo and hi.hi of its 16 elements in that order to an fp32 accumulator; 2^-24 is folded in at the end; tails are
 *     rows of zeros.  The rows are meant to be unit vectors: an element of magnitude 16 or more leaves fp16's range, and
 *     its row's similarities are then not finite.)
 *   Candidates.  Gallery row j is a candidate of query i iff s_ij is finite (a NaN row on either side is never a
 *     neighbour), j != d_skip[i] (NULL or -1: nothing is skipped; leave-one-out passes the query's own gallery index), and,
 *     when labels are given, 0 <= d_gallery_label[j] < K (unknown truths are never neighbours).
 *   Neighbours.  The first k' = min(k, candidates) candidates in the order (s descending, j ascending); equal floats, +0
 *     and -0 included, go by index.  Those are ranks 0 .. k' - 1; ranks k' .. k - 1 store idx = -1, sim = -inf.  A query
 *     without any candidate stores a NaN d_probs row and label -1.
 *   Vote.  A fixed fp32 chain: w_r = expf(fl32(fl32(s_r - s_0) inv_T)), so w_0 is exactly 1; den and score[label_r] are
 *     accumulated r ASCENDING from 0 (den = den + w_r, score[label_r] = score[label_r] + w_r); p[c] = score[c] / den; label =
 *     the FIRST maximum of p.  inv_T = fl32(1 / T) is formed in double by the caller.
 *   Determinism.  No float atomics; the same bytes on every run; a query's outputs do not depend on where it stands in the
 *     list or on how the list is chunked.
 *
 * cmlpl_knn: that definition.  n, m >= 1; 1 <= k <= 32; with labels 1 <= K <= 64 and a finite inv_T > 0; with
 *   d_gallery_label == NULL, K is 0 and d_probs / d_labels must be NULL.  d_nbr_idx [n][k] int32, d_nbr_sim [n][k],
 *   d_probs [n][K], d_labels [n] int64: ANY of them may be NULL.  Four launches (three when d_query == d_gallery and
 *   n == m: one set of pieces): the split of each side into fragment planes in the workspace, the streaming pass --
 *   similarity tiles on v_mfma_f32_32x32x16_f16, the queries on the lanes, selection against a per-lane threshold, the lists
 *   in LDS; the [n][m] matrix never exists -- and the merge + vote, one wavefront per query.  d_skip and the labels are
 *   DATA ON THE DEVICE; nothing synchronises or allocates.  Workspace: cmlpl_knn_workspace_bytes(n, m, k) (0 for arguments
 *   outside the ranges): 4 KiB per row of either side, padded to 128 rows, and the partial lists.
 *   CMLPL_E_ARG: a null d_query / d_gallery / d_workspace, a range above, K / d_probs / d_labels without labels, d_query /
 *   d_gallery / d_workspace not 16-byte aligned, another misaligned pointer; CMLPL_E_WORKSPACE -- all before any launch. */
int cmlpl_embed(const cmlpl_shape* shape, int nets, const float* d_params, int64_t param_stride,
                const float* d_spectra, const int64_t* d_spec_row /* [n] or NULL */, int n,
                float* d_feat /* [nets][n][1024] */, float* d_norm /* [nets][n] */, void* stream);
size_t cmlpl_knn_workspace_bytes(int n, int m, int k);
int cmlpl_knn(const float* d_query /* [n][1024] */, int n, const float* d_gallery /* [m][1024] */, int m,
              const int64_t* d_gallery_label /* [m] or NULL */, int K, const int64_t* d_skip /* [n] or NULL */,
              int k, float inv_T,
              int32_t* d_nbr_idx /* [n][k] or NULL */, float* d_nbr_sim /* [n][k] or NULL */,
              float* d_probs /* [n][K] or NULL */, int64_t* d_labels /* [n] or NULL */,
              void* d_workspace, size_t workspace_bytes, void* stream);

/* Added after ABI 6, no bump (nothing existing moves; cmlpl_dyn.reserved keeps its name, type and offset and gains a
 * meaning that every earlier caller's zero spells "off") -- LEARNING-RATE SCHEDULES, DECOUPLED WEIGHT DECAY AND
 * GRADIENT-NORM CLIPPING.  The reference trains with torch.optim.Adam at one fixed --lr (train.py:131-132); these are
 * torch.optim.AdamW's decay (Loshchilov & Hutter, "Decoupled Weight Decay Regularization", ICLR 2019) and
 * torch.nn.utils.clip_grad_norm_, per network, since the reference keeps one optimiser per network.
 *
 * THE DEFINITION OF A CLIPPED, DECAYED ADAM STEP.  Network n (0 or 1) has the gradients g of its flat block, d_grads +
 * n * grad_stride, laid out as the parameters are (cmlpl_layout_t).
 *   Gradient norm.  S_n = the sum, over the elements of the ten live tensors (tensor by tensor: param_off[t] ..
 *     param_off[t] + param_numel[t], t < CMLPL_NUM_LIVE), of (double)g * (double)g.  The up4(K) - K pad floats behind
 *     classifier.bias lie inside param_live and do NOT count; nothing of the dead tensors counts.  The sum is taken in
 *     fp64 in an order fixed by the launch geometry alone: the same bytes on every run, no floating-point atomics.
 *     norm_n = (float)sqrt(S_n).
 *   Clip coefficient.  coef_n = max_norm / (norm_n + 1e-6f) in fp32 (one addition, one correctly rounded division),
 *     then coef_n = 1.0f where coef_n > 1.0f.  A NaN norm gives a NaN coefficient (the comparison is false), as
 *     torch's clamp does.  max_norm == 0 means NO clipping: coef_n = 1.0f whatever the norm is.
 *   Update, per element of the ten live tensors (the pad floats behind classifier.bias go through the same chain, as
 *     they go through cmlpl_adam_step; their gradients are whatever the caller left there):
 *       1. g' = g * coef_n                 one fp32 multiply, never fused into what follows
 *       2. p' = p * keep                   one fp32 multiply, never fused; keep = (float)(1.0 - (double)lr_t *
 *                                          (double)weight_decay), formed on the HOST in double -- AdamW's
 *                                          param.mul_(1 - lr * weight_decay).  All ten live tensors, biases included,
 *                                          as torch.optim.AdamW(Base.parameters()) would; dead tensors never move.
 *       3. cmlpl_adam_step's update of (p', g'), unchanged: m, v and the new parameter.
 *     coef_n == 1.0f and keep == 1.0f are exact identities: the step is then cmlpl_adam_step's, bit for bit.
 *   Side effects.  The packed weight copies and the two-piece range flag follow the new parameters exactly as they
 *     follow cmlpl_adam_step's.
 *   Learning rate.  lr_t is hp->lr of the call for a by-value step; for a table-fed (replayed) step it is what formed
 *     the row's adam_step_size, and keep is the float whose BIT PATTERN the row's `reserved` holds -- all-zero bits
 *     mean no decay (keep = 1.0f), which is what every caller before this section writes.  A keep of exactly 0.0f
 *     (lr_t * weight_decay == 1) is refused on the host: its bits would say "off".
 *   The norms row.  Four floats {norm_0, norm_1, coef_0, coef_1}; a call over one network writes slots 0 and 2 only.
 *     d_norms follows d_scalars' addressing: the four floats AT the pointer for a by-value step, at d_norms + 4 *
 *     hist_row of the step's row for a table-fed one.
 *
 * cmlpl_optim: the options of a step.  max_norm >= 0 and weight_decay >= 0, both finite.  d_norms is optional (NULL:
 *   no row is written).  d_partials: cmlpl_grad_norm_partials_bytes() bytes of device memory, 8-byte aligned, required
 *   when max_norm > 0 or d_norms != NULL; it needs no initialisation and carries nothing from step to step.
 * cmlpl_grad_norm: the reduction alone, two launches -- grad_norm_kernel (64 workgroups per network, each leaves ONE
 *   fp64 partial: thread -> wavefront butterfly -> four wavefronts added ascending; no ticket word, no memset) and a
 *   one-wavefront-per-network launch that folds the 64 partials by the same butterfly and writes the norms row AT
 *   d_norms.  grad_stride >= param_total is the distance between the networks' blocks.
 * cmlpl_adam_step_opt: cmlpl_adam_step with options.  opt == NULL IS cmlpl_adam_step (the same launch of the same
 *   kernel).  Otherwise: grad_norm_kernel when max_norm > 0 or d_norms is given, then ONE launch of the Adam kernel's
 *   second instantiation (a template parameter, no run-time branch per element), in which every wavefront folds its
 *   network's 64 L2-resident partials itself and workgroup 0 of each network writes the norms row: one launch more than
 *   cmlpl_adam_step, none when neither clipping nor the row is asked for.
 * cmlpl_train_step_opt / cmlpl_step_graph_create_opt: cmlpl_train_step / cmlpl_step_graph_create with options; opt ==
 *   NULL is the old call.  With io->apply_update == 0 the norms row is still written (cmlpl_grad_norm's two launches
 *   behind the backward), so gradients and norms of the same step can be read together.
 * cmlpl_dyn_adam_opt: cmlpl_dyn_adam, and the decay factor of the row (store its bit pattern in cmlpl_dyn.reserved).
 * CMLPL_E_ARG: a null opt where one is required, a negative / NaN / infinite max_norm or weight_decay, a keep of 0.0f,
 *   missing or misaligned d_partials, a misaligned d_norms, nets outside 1 .. 2, grad_stride < param_total. */
typedef struct cmlpl_optim {
  float max_norm;       /* clip_grad_norm_'s max_norm; 0 = no clipping     */
  float weight_decay;   /* AdamW's weight_decay; 0 = none                  */
  float* d_norms;       /* optional: {norm0, norm1, coef0, coef1}          */
  void* d_partials;     /* cmlpl_grad_norm_partials_bytes() bytes          */
} cmlpl_optim;
size_t cmlpl_grad_norm_partials_bytes(void);
int cmlpl_grad_norm(const cmlpl_shape* shape, int nets, const float* d_grads, int64_t grad_stride, float max_norm,
                    void* d_partials, float* d_norms, void* stream);
int cmlpl_adam_step_opt(const cmlpl_shape* shape, int nets, float* d_params, int64_t param_stride,
                        const float* d_grads, int64_t grad_stride, float* d_m, float* d_v,
                        int64_t t, const cmlpl_hparams* hp, float* d_packed, const cmlpl_optim* opt, void* stream);
int cmlpl_train_step_opt(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io,
                         const cmlpl_optim* opt, void* stream);
int cmlpl_step_graph_create_opt(const cmlpl_shape* shape, const cmlpl_hparams* hp, const cmlpl_step_io* io,
                                const cmlpl_optim* opt, void* stream, void** graph_out);
int cmlpl_dyn_adam_opt(const cmlpl_hparams* hp, int64_t adam_t, float weight_decay, float* step_size, float* bc2_sqrt,
                       float* keep);

/* Added after ABI 6, no bump (nothing existing moves) -- LABEL PROPAGATION OVER THE EMBEDDING'S kNN GRAPH: the transductive
 * "label spreading" of Zhou et al. ("Learning with Local and Global Consistency", NIPS 2003), as Iscen et al. use it on
 * deep embeddings ("Label Propagation for Deep Semi-supervised Learning", CVPR 2019), over the neighbour lists cmlpl_knn
 * writes.  The reference has no counterpart.
 *
 * THE DEFINITION OF A PROPAGATED LABELLING.
 *   Inputs.  n nodes; neighbour lists nbr_idx [n][k] int32 and nbr_sim [n][k] float exactly as cmlpl_knn writes them
 *     (pads are idx = -1), 1 <= k <= 32; an integer exponent gamma in 1 .. 8; a dense non-negative Y [n][K] float,
 *     1 <= K <= 64 (one-hot rows for seeds and zero rows elsewhere is the usual case; any non-negative matrix is allowed,
 *     e.g. a classifier's probabilities); 0 <= alpha < 1; iters in 1 .. 10,000; an optional start F0 [n][K], NULL = Y.
 *   Edges.  Entry (i, r) with j = idx[i][r], 0 <= j < n, j != i is a FORWARD edge i -> j of weight a = s^gamma, formed by
 *     repeated fp32 multiplication (a = s; gamma - 1 times a = a * s), when 0 < s <= FLT_MAX, else a = 0: NaN, -inf and
 *     negative similarities give weight 0, and an edge of weight 0 STAYS an edge.  Pads and self entries are no edges.
 *     Indices >= n are followed without a check.
 *   Symmetrisation.  W = A + A^T.  Node i's EDGE LIST is its forward edges, r ascending, followed by its REVERSE edges
 *     -- every (j, r) with idx[j][r] == i -- ordered by j ascending (and r ascending within one j).  A mutual pair simply
 *     appears in both parts: its weight counts twice, nothing is de-duplicated.
 *   Degree and coefficients.  d_i = the fp32 sum of the list's weights in that order (one chain from 0).  c_i = 1 /
 *     sqrtf(d_i) when d_i > 0, else 0.  The coefficient of an edge of node i to j is (c_i * a) * c_j, two fp32
 *     multiplications in that order: Zhou's S = D^-1/2 W D^-1/2.
 *   Iteration.  F_{t+1}[i][c] = alpha * SUM_e coef_e * F_t[j_e][c] + beta * Y[i][c]; the sum runs over the node's list
 *     in list order in fp32, acc = fma(coef_e, F_t[j_e][c], acc) from 0, and the result is fma(alpha, acc, fl32(beta *
 *     Y[i][c])).  beta = (float)(1 - (double)alpha) is formed on the host.  With alpha = 0 the result is Y's bytes after
 *     any number of iterations (finite F).
 *   Finish.  z = SUM_c F[i][c], c ascending.  When z > 0: p = F / z, label = the FIRST maximum of p, confidence =
 *     p[label], entropy = -SUM_c p log p, c ascending, the terms at p = 0 left out.  When z is not > 0 (an unreached node,
 *     or NaN): label -1 and NaN p / confidence / entropy -- cmlpl_knn's rule for a query without candidates.
 *   Residual.  max |F_T - F_{T-1}| over all entries of the last iteration: a float obtained with an INTEGER max on the bit
 *     patterns of non-negative floats (a NaN difference gives a NaN).  No float atomics.
 *   Determinism.  The same bytes on every run, every byte of the graph workspace included.  Splitting iters into legs
 *     changes no byte: 10 iterations, then 10 more from the result passed as F0, are the bytes of 20.
 *
 * THE GRAPH WORKSPACE: cmlpl_lp_graph_bytes(n, k) = 4 (3 n + 1 + 5 n k) bytes, arrays of 4-byte words one behind the
 *   other with no padding, N = n k:
 *       cinv      float [n]        c_i                                              word 0
 *       fwd_coef  float [n][k]     the coefficient of entry (i, r); 0 for a pad / self entry    n
 *       rev_ptr   int32 [n + 1]    node i's reverse edges are slots rev_ptr[i] .. rev_ptr[i + 1] - 1;  n + N
 *                                  rev_ptr[n] = E, the number of edges
 *       rev_src   int32 [N]        the source node of each reverse edge; -1 in slots >= E       2 n + 1 + N
 *       rev_coef  float [N]        its coefficient (c_i * a) * c_src; 0 in slots >= E           2 n + 1 + 2 N
 *       fwd_dst   int32 [n][k]     idx[i][r] of a forward edge, -1 for a pad / self entry       2 n + 1 + 3 N
 *       rev_edge  int32 [N]        the entry j k + r a reverse edge came from; -1 past E        2 n + 1 + 4 N
 *       in_deg    int32 [n]        rev_ptr[i + 1] - rev_ptr[i]                                  2 n + 1 + 5 N
 *   The propagation reads the workspace alone (the lists may be freed).
 *
 * cmlpl_lp_graph: builds it.  Six stream operations: a memset of in_deg, the in-degree count (one integer atomic per
 *   edge), an exclusive scan by one workgroup, the fill (the same atomic hands out slots: the order inside a segment is
 *   the run's), the per-node pass that REMOVES that order -- a segment of up to 2,048 edges is sorted in LDS by counting
 *   (edge ids are unique), a longer one (a hub: in-degree has no bound) is re-found in ascending order by a compaction
 *   scan over all N entries -- and adds the node's degree as one chain, and the coefficients.  rev_ptr / rev_src are
 *   identical on every run.  CMLPL_E_ARG: a null or misaligned (4 bytes) pointer, n < 1, k outside 1 .. 32, n k >= 2^31,
 *   gamma outside 1 .. 8; CMLPL_E_WORKSPACE: bytes < cmlpl_lp_graph_bytes(n, k) (which is 0 for n, k outside the ranges).
 * cmlpl_lp_propagate: `iters` launches, ping-pong between d_F and d_tmp ([n][K] each; the final F always ends in d_F;
 *   d_tmp holds F_{T-1} or garbage), then one finishing launch unless all of d_probs [n][K], d_labels [n] int64, d_conf
 *   [n], d_entropy [n] are NULL; d_residual (one float) is cleared by a memset node first when given.  A group of G =
 *   2^ceil(log2 K) lanes per node, one class per lane; the group reads indices and coefficients once, G at a time, and a
 *   neighbour's F row as one contiguous segment.  One group walks one list whatever its length.  d_Y is only read.
 *   CMLPL_E_ARG: a null d_graph / d_Y / d_F / d_tmp, a range above, n K >= 2^31, alpha outside [0, 1) (NaN too), two of
 *   d_F / d_tmp / d_Y / d_F0 the same pointer, a misaligned pointer.
 * All before any launch; nothing synchronises or allocates. */
size_t cmlpl_lp_graph_bytes(int n, int k);
int cmlpl_lp_graph(const int32_t* d_nbr_idx /* [n][k] */, const float* d_nbr_sim /* [n][k] */, int n, int k, int gamma,
                   void* d_graph, size_t bytes, void* stream);
int cmlpl_lp_propagate(const void* d_graph, int n, int k, const float* d_Y /* [n][K] */, int K, float alpha, int iters,
                       const float* d_F0 /* [n][K] or NULL */, float* d_F /* [n][K] */, float* d_tmp /* [n][K] */,
                       float* d_probs /* [n][K] or NULL */, int64_t* d_labels /* [n] or NULL */,
                       float* d_conf /* [n] or NULL */, float* d_entropy /* [n] or NULL */,
                       float* d_residual /* [1] or NULL */, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- SUPERPIXELS AND REGION VOTES: object-based classification.  The
 * scene is over-segmented into superpixels (SLIC, Achanta et al. 2012, in its per-pixel GPU form gSLIC, Ren & Reid 2011),
 * every region votes, and the region is labelled as one.  The reference has no counterpart: each of its labels is the
 * product of a single window.
 *
 * THE DEFINITION OF A SUPERPIXEL MAP.
 *   Inputs.  A scene of rows x cols pixels, i = y cols + x.  Guide g[i][0 .. G - 1] = the first G floats at d_guide + i
 *     guide_stride, 0 <= G <= 8.  Grid step S, 2 .. 64.  Compactness m, finite and > 0.  Iterations T, 1 .. 100.
 *     w = fl32(m^2 / S^2), formed in double on the host from the fp32 m; it must be finite and > 0.
 *   Cells and centres.  ny = ceil(rows / S), nx = ceil(cols / S), N = ny nx segments; N >= 2^24 is refused.  Segment
 *     s = a nx + b is cell (a, b).  A pixel is REGULAR when every guide channel is finite and |g| <= 2^20; with G = 0 every
 *     pixel is regular.  Initial centre c_s = (cy, cx, g..): cy = (float)min(rows - 1, a S + S / 2) and cx likewise, with
 *     integer division; the guide part is that pixel's guide, or all zeros if that pixel is irregular.
 *   Assign (per pixel, from centres c^(t-1)).  Candidates are the cells (y / S + da, x / S + db) for da, db in -1, 0, 1
 *     that lie inside the grid, scanned da ascending and, within da, db ascending.  Per candidate, in this order:
 *       dc2 = 0;  for ch ascending:  d = g[ch] - c[ch];  dc2 = fmaf(d, d, dc2)
 *       dy = (float)y - cy,  dx = (float)x - cx
 *       ds2 = fmaf(dx, dx, fl(dy dy))
 *       D = fmaf(ds2, w, dc2)
 *     Every operation is rounded once; nothing else is contracted.  The label is the candidate with the smallest D under
 *     strict <, starting from best = +inf and label = the pixel's own cell: a tie keeps the earlier candidate, a NaN or
 *     +inf D never wins.  An irregular pixel computes nothing and keeps its own cell.
 *   Update.  Over the regular pixels of segment s accumulate int64 n, Sy, Sx and Sg[ch] = sum llrintf(g[ch] * 2^24) (the
 *     product is exact).  For n > 0: cy = (float)((double)Sy / (double)n), cx likewise, c[ch] = (float)((double)Sg[ch] /
 *     ((double)n * 16777216.0)).  For n == 0 the centre stays what it was.  All sums are integers, so the result does not
 *     depend on any order.
 *   Iteration.  For t = 1 .. T: assign, then update.  Outputs: seg int32 [rows cols] from the T-th assignment; centres
 *     float [N][2 + G] after the T-th update; counts int32 [N], the regular pixels per segment.
 *   Consequence.  A segment's pixels lie inside its 3 x 3 block of cells, so n <= 9 S^2: no int64 can overflow, and an
 *     implementation may gather per segment in place of scattering per pixel.
 *   Not built: moving the seeds to the lowest gradient.  A segment of this map need not be connected -- small detached
 *     fragments can exist, confined to a 3 x 3 cell block; SLIC's connectivity post-pass is the sieve of the segment ids
 *     followed by the component ids of the result ("THE DEFINITION OF A COMPONENT MAP" and "THE DEFINITION OF A SIEVED
 *     MAP" below).
 *
 * THE DEFINITION OF A REGION VOTE.
 *   Inputs.  Any int32 map seg[n], N, K <= 64, and one of two sources.
 *   Soft source.  Probabilities p[n][K]; a row is valid when every entry is finite and 0 <= p <= 2.  P[s][c] = sum
 *     llrintf(p[i][c] * 2^24) over the valid rows with 0 <= seg[i] < N, cnt[s] their number, q[s][c] = (float)((double)
 *     P[s][c] / ((double)cnt[s] * 16777216.0)).
 *   Hard source.  int64 labels l[n]; a row is valid when 0 <= l < K (and 0 <= seg[i] < N); P[s][c] counts rows, q[s][c] =
 *     (float)((double)P / (double)cnt).
 *   Per segment, by cmlpl_ensemble's rules: label = the FIRST maximum of q; conf = q[label]; entropy = 0 - sum_c q_c
 *     logf(q_c), c ascending, 0 log 0 = 0.  A segment with cnt == 0 gets label -1 and NaN for q / conf / entropy (cmlpl_knn's
 *     rule for an unreached row).
 *   Broadcast.  Pixel i takes its segment's label, q, conf and entropy -- an invalid row inside a voted segment is repaired
 *     by its region; a pixel with seg[i] outside 0 .. N - 1 gets -1 and NaNs.
 *   Optional outputs: int64 P[N][K], int64 cnt[N], the per-segment table q[N][K] and the segment labels int64 [N].
 *   ASA (achievable segmentation accuracy): hard-vote a truth map -- the scene's labels at the listed test pixels, -1
 *     everywhere else, so those rows are invalid and left out; ASA = sum_s max_c P[s][c] / sum_s cnt[s], host arithmetic
 *     on P.  It is the best overall accuracy ANY region-level labelling of the map could reach.
 *
 * cmlpl_sp_workspace_bytes(rows, cols, G, S) = 4 (N (2 + G) + G n) + n rounded up to 4, n = rows cols: the centres, the
 *   guide packed planar [G][n] once per call, and a regular-pixel byte per pixel; 0 for arguments outside the ranges.
 * cmlpl_sp_segment: pack, init, then T times assign (a workgroup per tile of 32 x 8 pixels, its candidate centres staged in
 *   LDS) and update (one wavefront gathers a segment's clipped 3S x 3S block: no atomics, no memset).  d_seg [rows cols];
 *   d_centres [N][2 + G] and d_counts [N] each or NULL.  The result does not depend on the workspace's prior contents.
 *   CMLPL_E_ARG before any launch: rows or cols < 1 (or rows cols past 2^31 - 1), G outside 0 .. 8, S outside 2 .. 64,
 *   N >= 2^24, iters outside 1 .. 100, m not finite or <= 0, w not finite or zero, G > 0 with a null d_guide or guide_stride
 *   < G, a null d_seg or d_ws, a misaligned pointer (4 bytes), ws_bytes < cmlpl_sp_workspace_bytes.
 * cmlpl_sp_vote_workspace_bytes(N, K) = 12 N (K + 2): int64 P [N][K], cnt [N], segment labels [N]; float q [N][K], conf
 *   [N], entropy [N]; 0 for N < 1, K outside 1 .. 64 or N K past 2^31 - 1.
 * cmlpl_sp_vote_probs / cmlpl_sp_vote_labels: a memset node over P and cnt, the accumulation (64-bit INTEGER atomics; a run
 *   of neighbouring lanes with one segment id is summed inside the wave first), one finishing launch per segment, and a
 *   broadcast launch when a per-pixel output is asked for (d_out_probs [n][K], d_labels [n] int64, d_conf, d_entropy [n],
 *   each or NULL); d_sums int64 [N][K], d_cnt int64 [N], d_seg_probs [N][K], d_seg_labels int64 [N], each or NULL.
 *   CMLPL_E_ARG before any launch: n or N < 1, K outside 1 .. 64, N K past 2^31 - 1, a null d_seg / source / d_ws, every
 *   output null, a misaligned pointer (8 bytes for int64 arrays and the workspace, else 4), ws_bytes too small.
 * Nothing allocates or synchronises; everything can be captured in a graph.  No float atomics: every output is the same
 * bytes on every run. */
size_t cmlpl_sp_workspace_bytes(int rows, int cols, int G, int S);
int cmlpl_sp_segment(const float* d_guide, int64_t guide_stride, int G, int rows, int cols, int S, float m, int iters,
                     int32_t* d_seg, float* d_centres, int32_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);
size_t cmlpl_sp_vote_workspace_bytes(int N, int K);
int cmlpl_sp_vote_probs(const int32_t* d_seg, const float* d_probs, int n, int K, int N, float* d_out_probs,
                        int64_t* d_labels, float* d_conf, float* d_entropy, int64_t* d_sums, int64_t* d_cnt,
                        float* d_seg_probs, int64_t* d_seg_labels, void* d_ws, size_t ws_bytes, void* stream);
int cmlpl_sp_vote_labels(const int32_t* d_seg, const int64_t* d_src_labels, int n, int K, int N, float* d_out_probs,
                         int64_t* d_labels, float* d_conf, float* d_entropy, int64_t* d_sums, int64_t* d_cnt,
                         float* d_seg_probs, int64_t* d_seg_labels, void* d_ws, size_t ws_bytes, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- WHICH WINDOWS THE CUTS TAKE.  cmlpl_extract_patches and
 * cmlpl_tta_patches(_sym) hold one window of w x w pixels x C channels in LDS and return CMLPL_E_SHAPE for one that does
 * not fit in 160 KiB (about w w C <= 40,960 floats: at 20 x 20, 101 channels fit and 102 do not).  A caller that scores a
 * scene by patches -- windows the fused forward of cmlpl_infer_cube does not take -- asks here BEFORE it builds anything:
 * bit 0 = the clean cut (cmlpl_extract_patches) takes (C, w), bit 1 = the view cut (cmlpl_tta_patches / _sym, d_out != NULL)
 * does; 0 for C < 1 or w < 1.  Answered from the two launchers' own LDS sizes, which the entry points above compare as well.
 * Host arithmetic only. */
int cmlpl_patches_fit(int C, int w);

/* Added after ABI 6, no bump (nothing existing moves) -- CONNECTED REGIONS: which pixels of a map form one region.
 *
 * THE DEFINITION OF A COMPONENT MAP.
 *   Inputs.  An int32 map v[n] of a rows x cols scene, i = y cols + x, n = rows cols <= 2^31 - 1; conn in {4, 8}.
 *   Terms.  A pixel with v[i] < 0 is VOID.  Two pixels are adjacent when they differ by one step in y or in x (conn 4), or
 *     by at most one step in each and not both zero (conn 8), inside the scene.  Adjacent non-void pixels with equal values
 *     are joined; a component is a class of the transitive closure.
 *   Outputs.  comp[i] = the smallest pixel index of i's component, -1 for a void pixel; a ROOT is a pixel with comp[i] == i.
 *     size[i] (int32) = the number of pixels of i's component, 0 for a void pixel.  id[i] = the number of roots with a
 *     smaller index than comp[i], so the components are numbered 0 .. M - 1 in the order of their first pixel; -1 for a void
 *     pixel.  M, an int32 word on the device.
 *   Every output is an integer that does not depend on any order.
 *
 * THE DEFINITION OF A SIEVED MAP (the operation GDAL calls sieve, with a parallel merge order).
 *   Inputs.  v and conn as above; min_size in 1 .. 2^31 - 1; passes T in 1 .. 16.
 *   u_0 = v.  Pass t works on the components of u_(t-1).  A component is SMALL when its size is less than min_size, else
 *     LARGE.  The candidates of a small component a are the large components that hold a pixel adjacent (under the same
 *     conn) to a pixel of a.  Its target is the candidate with the greatest size; ties go to the smaller root -- the maximum
 *     of the 64-bit integer (size << 32) | (0xFFFFFFFF - root).  If a has a target, every pixel of a takes u_(t-1)[root of
 *     the target]; otherwise a stays.  All components move at once, from u_(t-1).  Void pixels are never sources, never
 *     targets, and never change.
 *   Outputs.  u_T, and int32 stats[T][4] = {components, small components, small components with a target, pixels
 *     relabelled} of pass t.
 *   Consequences.  Large components only grow.  A relabelled pixel never changes again.  A pass with 0 relabelled pixels
 *     makes every later pass the identity.  min_size = 1 returns v's bytes.  T passes in one call are the bytes of the same
 *     passes in several calls.  A small component with only small neighbours waits for a later pass, possibly for ever:
 *     that is the definition, not a defect.
 *   Not built: GDAL's smallest-first sequential merge order, merging by class-weighted boundary length, 3-D connectivity.
 *
 * cmlpl_cc_workspace_bytes(rows, cols) = 8 + 16 n + 4 (ceil(n / 1024) + 2) + 272: a 64-bit target word, a parent word and a
 *   size word per pixel, the root counts per block of 1024 pixels, the counters; 0 for rows or cols < 1 or n past 2^31 - 1.
 * cmlpl_cc_label: union-find in a fixed number of launches whatever the map holds -- tile (a workgroup labels 32 x 32
 *   pixels in LDS), border (unites across tile borders in global memory, the larger root always linked under the smaller
 *   by a 32-bit atomic min), flatten (every pixel takes its root; sizes by 32-bit atomic adds, a run of lanes with one root
 *   summed in the wave first); with d_id or d_M a one-workgroup scan of the per-block root counts and a rank launch; with
 *   d_id or d_size a broadcast launch.  d_comp [n]; d_size [n], d_id [n], d_M [1], each or NULL.
 * cmlpl_cc_sieve: per pass tile, border, flatten, candidates (64-bit integer atomic max per small root), apply; with
 *   d_probs [n][K] AND d_conf [n] a finishing launch writes conf[i] = probs[i][out[i]] for 0 <= out[i] < K, else NaN.
 *   d_out [n] may be d_map.  d_stats int32 [passes][4] or NULL.
 * CMLPL_E_ARG before any launch: rows or cols < 1 (or rows cols past 2^31 - 1), conn not 4 or 8, min_size < 1, passes
 *   outside 1 .. 16, a null d_map / d_comp / d_out / d_ws, one of d_probs and d_conf without the other, K < 1 with them, a
 *   misaligned pointer (4 bytes), ws_bytes < cmlpl_cc_workspace_bytes.
 * Nothing allocates, synchronises or reads back, so a call can be captured in a graph; no loop waits for another thread
 * (csrc/regions.hip argues the termination).  Integer atomics only: every output is the same bytes on every run, and none
 * depends on what the workspace held before. */
size_t cmlpl_cc_workspace_bytes(int rows, int cols);
int cmlpl_cc_label(const int32_t* d_map, int rows, int cols, int conn, int32_t* d_comp, int32_t* d_size /* or NULL */,
                   int32_t* d_id /* or NULL */, int32_t* d_M /* or NULL */, void* d_ws, size_t ws_bytes, void* stream);
int cmlpl_cc_sieve(const int32_t* d_map, int rows, int cols, int conn, int min_size, int passes, int32_t* d_out,
                   int32_t* d_stats /* [passes][4] or NULL */, const float* d_probs /* [n][K] or NULL */, int K,
                   float* d_conf /* [n] or NULL */, void* d_ws, size_t ws_bytes, void* stream);

/* Added after ABI 6, no bump (nothing existing moves) -- THE REGION GRAPH: from a region map to the neighbour lists that
 * cmlpl_lp_graph takes, so that the regions of a scene become the nodes of a label propagation.
 *
 * The map.  int32 ids[n] of a rows x cols scene, i = y cols + x, n = rows cols <= 2^27; M in 1 .. 2^27.  Pixel p BELONGS to
 *   region ids[p] when 0 <= ids[p] < M; anything else -- a negative value, a value >= M -- is VOID.  Any such map is taken:
 *   a superpixel map, the ids of connected segments, the ids of a component map.  A region need not be connected and may be
 *   empty.  (n <= 2^27: the adjacency's tables hold fewer than 16 n entries, which 31 bits index.)
 *
 * THE DEFINITION OF A REGION DESCRIPTOR.
 *   Inputs.  The map; X float32 [n][B] under a row stride >= B (in floats), 1 <= B <= 1024.
 *   Pixel p is POOLED iff it belongs to a region and every X[p][b], b < B, is finite with |x| <= 256 (z-scored spectra never
 *     leave that range).  S[s][b] = sum over the pooled p of region s of llrintf(X[p][b] * 2^24), an int64: the product is
 *     exact, a term is at most 2^32 in magnitude and a region has at most 2^31 - 1 pixels, and 2^32 x (2^31 - 1) < 2^63, so
 *     no sum can overflow at any map size.  cnt[s] = the pooled pixels of s, an int64.
 *     mean[s][b] = fl32(double(S[s][b]) / (double(cnt[s]) * 2^24)) -- the expression of the superpixel centres --, and a
 *     row of zeros for cnt[s] == 0.
 *   Every output is an integer sum, or one rounding of one: it does not depend on any order.
 *
 * THE DEFINITION OF A REGION ADJACENCY (4-connected only).
 *   Inputs.  The map; A in 0 .. 16.
 *   For every pixel p and its right and its lower neighbour q inside the scene: if both belong to regions and ids[p] !=
 *     ids[q], 1 is added to b[ids p][ids q] and to b[ids q][ids p].  So b is symmetric, and b[s][t] is the length of the
 *     boundary between s and t in pixel edges.
 *   Outputs, all int32 and exact.  deg[s] = the number of t with b[s][t] > 0.  boundary[s] = sum_t b[s][t].  The LIST of s is
 *     those t sorted by (b[s][t] descending, t ascending), cut to its first A entries: adj_idx[s][a] the region, -1 past
 *     the end; adj_len[s][a] its b[s][t], 0 past the end.  A region with deg[s] > A is TRUNCATED.
 *
 * THE DEFINITION OF A REGION GRAPH.
 *   Inputs.  feat float32 [M][1024], a row per region; the lists knn_idx int32 / knn_sim float32 [M][k] as cmlpl_knn writes
 *     them (k >= 0); adj_idx [M][A]; 1 <= k + A <= 32 (the longest list cmlpl_lp_graph takes).
 *   Outputs.  nbr_idx int32 / nbr_sim float32 [M][k + A].  Slots 0 .. k - 1 of row s are the kNN entries, copied.  Slot k + a
 *     holds t = adj_idx[s][a]: -1 / -inf when t is outside 0 .. M - 1 or already stands in one of the k kNN slots of s;
 *     otherwise t with sim = the fp32 dot product of feat[s] and feat[t] -- in any summation order, fused or not: within
 *     1024 x 2^-24 x sum_i |a_i b_i| (first order) of the exact value.  A dot product that is not finite is stored as it is
 *     (cmlpl_lp_graph gives such an entry the weight 0).
 *   The graph is cmlpl_lp_graph of these lists and the labelling cmlpl_lp_propagate from Y[s] = the region vote's q[s] (a
 *     NaN row becomes a zero row), both unchanged ("THE DEFINITION OF A PROPAGATED LABELLING"); every pixel of region s takes
 *     the label, probabilities, confidence and entropy of s, a void pixel and a pixel of an unreached region -1 and NaN.
 *   Not built: 8-connected adjacency, edge weights from the boundary length, a sharded version.
 *
 * cmlpl_rg_workspace_bytes(rows, cols, M, A) = 16 + 4 (3 M + 1 + ceil(M / 1024) + 2 + 33 n): what one call of
 *   cmlpl_rg_pool or cmlpl_rg_adjacency needs; 0 for arguments outside the definitions.
 * cmlpl_rg_pool: the pixel index by region (a histogram and a scatter with 32-bit integer atomics around an exclusive
 *   scan), then a wavefront per region of up to 64 pixels and a workgroup per larger one, lanes along the bands, int64 sums
 *   in registers.  d_mean [M][B], d_cnt int64 [M], d_S int64 [M][B] or NULL.  Eight launches.
 * cmlpl_rg_adjacency: the directed contacts per region (= boundary), a scan that gives every region an open-addressing
 *   table of the next power of two >= 2 boundary[s] entries, an init launch, an insert launch (32-bit atomicCAS on the key,
 *   atomicAdd on the count: no thread waits for another), and a wavefront per region that picks the list in A rounds of a
 *   wave-wide 64-bit integer maximum.  d_adj_idx / d_adj_len [M][A] (NULL allowed for A == 0), d_deg [M], d_boundary [M].
 *   Eight launches.
 * cmlpl_rg_lists: one launch, a wavefront per region.  d_knn_idx / d_knn_sim may be NULL for k == 0, d_adj_idx for A == 0.
 * CMLPL_E_ARG before any launch: rows, cols or M < 1, n or M past 2^27, B outside 1 .. 1024, x_stride < B, A outside
 *   0 .. 16, k < 0, k + A outside 1 .. 32, a null pointer that is not optional, a misaligned pointer (4 bytes; 8 for d_cnt
 *   and d_S; 16 for d_feat); CMLPL_E_WORKSPACE: ws_bytes < cmlpl_rg_workspace_bytes.
 * Nothing allocates, synchronises or reads back, and the number of launches does not depend on the map, so a call can be
 * captured in a graph.  Integer atomics only: the integer outputs are the same bytes on every run, whatever the workspace
 * and the output buffers held before; the sims of cmlpl_rg_lists are a fixed order of fp32 operations, so they are too. */
size_t cmlpl_rg_workspace_bytes(int rows, int cols, int M, int A);
int cmlpl_rg_pool(const int32_t* d_ids, int rows, int cols, int M, const float* d_X, int64_t x_stride, int B, float* d_mean,
                  int64_t* d_cnt, int64_t* d_S /* or NULL */, void* d_ws, size_t ws_bytes, void* stream);
int cmlpl_rg_adjacency(const int32_t* d_ids, int rows, int cols, int M, int A, int32_t* d_adj_idx, int32_t* d_adj_len,
                       int32_t* d_deg, int32_t* d_boundary, void* d_ws, size_t ws_bytes, void* stream);
int cmlpl_rg_lists(const float* d_feat, int M, const int32_t* d_knn_idx, const float* d_knn_sim, int k,
                   const int32_t* d_adj_idx, int A, int32_t* d_nbr_idx, float* d_nbr_sim, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMLPL_H */
