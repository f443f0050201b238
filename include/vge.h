/*
 * vge.h -- C ABI of libvge.so, the MI355X (gfx950) implementation of the Action-Consistency /
 * Temporal-Coherence scoring path of XThomasBU/video-gen-evals.
 *
 * The reference has no FFI layer: its boundary is the set of Python functions eval.py composes.
 * Each entry point below replaces one of them (reference file:line cited per function).
 *
 * Conventions
 *   - Plain pointers and sizes; no torch types.  Pointers marked "device" are HBM buffers owned by
 *     the caller (hipMalloc / torch), "host" pointers are ordinary host memory.
 *   - Every compute call is asynchronous on the hipStream_t passed in (nullptr = default stream)
 *     and never synchronises, allocates or frees inside (graph-capture safe), except the create /
 *     reserve / destroy calls.
 *   - Return value: 0 (VGE_OK) or a vge_status code; nothing throws across the ABI.
 *     vge_last_error() returns a static description of the most recent failure on this thread.
 *   - Feature-column order is the reference's feats layout (utils.py:496-514):
 *       raw  = vit[1024] | global_orient[9] | pose[207] | betas[10] | kp2d[120]      (1370)
 *       diff = vit[1024] | global_orient[3] | pose[69]  | betas[10] | kp2d[120]      (1226)
 *     or, when the reference runs without keypoints (keypoint_dir None: no kp2d columns, 4 modalities),
 *       raw  = vit[1024] | global_orient[9] | pose[207] | betas[10]                   (1250)
 *       diff = vit[1024] | global_orient[3] | pose[69]  | betas[10]                   (1106)
 */
#ifndef VGE_H
#define VGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* vge_stream_t; /* == hipStream_t */

typedef enum {
  VGE_OK = 0,
  VGE_ERR_ARG = 1,            /* bad argument / unsupported shape */
  VGE_ERR_HIP = 2,            /* a HIP runtime call failed */
  VGE_ERR_MISSING_WEIGHT = 3, /* a required state_dict key is absent (the reference's
                                 load_state_dict(strict=False) would silently random-init it) */
  VGE_ERR_WEIGHT_SHAPE = 4,   /* a state_dict tensor has the wrong shape */
  VGE_ERR_NOMEM = 5,
  VGE_ERR_WORKSPACE = 6,      /* vge_encoder_reserve() was not called for this many windows */
  VGE_ERR_UNSUPPORTED = 7,    /* a model shape the kernels are not built for (vge_encoder_create): clip_len != 32,
                                 a modality set / input dims other than the reference's five or its keypoint-less
                                 four (clip / dino modalities, other vit or pose widths), or d_model / time_heads
                                 other than 256 / 8 outside the exact-f32 generic path (VGE_F32 only: d_model a
                                 multiple of 32 in [32, 256], head dim <= 64).  load_model (eval.py:136-165) reads
                                 these from the checkpoint; time_layers is free (any >= 1). */
  VGE_ERR_DEVICE = 8          /* a kernel detected a broken invariant and raised the encoder's status word (the
                                 staggered conv kernel's half-workgroup exchange wait ran out of its bound): the
                                 outputs of that launch are wrong.  Reported by vge_encoder_status, by
                                 vge_encoder_profile_read and by every later vge_encode until cleared. */
} vge_status;

/* Encoder compute modes.  VGE_F32: exact f32 MFMA (v_mfma_f32_16x16x4_f32, bitwise an fmaf chain).
 * VGE_F32X3: f32-class split precision -- every GEMM operand carried as fp16 hi + fp16 lo*2^11 and
 * each product formed as hi*hi + 2^-11 (hi*lo + lo*hi) on v_mfma_f32_32x32x16_f16 with f32
 * accumulation (relative error ~2^-21 per product; AC/TC within ~1e-7 of the f32 mode).  Its conv encoders
 * run staggered (vge_encoder_x3s.hip): each block's GroupNorm is folded into the next GEMM's weights and
 * epilogue, and GELU is a one-exp2 form within ~1 f32 ulp at |x| <= 6 (f32 rounding-level, as the reference's
 * own erf-based GELU); env VGE_X3S=0 keeps the unstaggered kernel and unfolded weights. */
typedef enum { VGE_F32 = 0, VGE_F32X3 = 1, VGE_F16 = 2 } vge_dtype;
/* VGE_F16: the throughput mode (BASELINE configs 2 / 5 "bf16" / "fp16 MFMA path"): the ten
 * MovementConvEncoders (85% of the FLOPs) take every GEMM operand as a single fp16 (the hi planes of the
 * VGE_F32X3 image, same power-of-two scaling), one v_mfma_f32_32x32x16_f16 per product, f32 accumulation
 * and f32 epilogues (GELU, GroupNorm); the transformer keeps the 3xfp16 split, because it carries most of
 * the fp16 error for ~10% of the FLOPs (env VGE_F16_MIX: bit 1 = transformer split [default 2], bit 0 =
 * stem split).  Measured AC/TC within 3e-5 of the reference on the golden set (tests/test_gpu_parity.py),
 * asserted at 1e-4 on the bench and config-5 workloads (tests/test_bench_parity.py); bench.py reports it. */

#define VGE_FEAT_DIM 2596
#define VGE_RAW_DIM 1370
#define VGE_FEAT_DIM_NOKP 2356 /* keypoint-less layout (keypoint_dir None) */
#define VGE_RAW_DIM_NOKP 1250

/* Feature layouts: which columns WindowDataset._try_one concatenates (utils.py:496-514).  The reference picks it by
 * whether keypoint_dir is set; infer_dims_from_stats (eval.py:104-133) then gives the model 5 or 4 modalities. */
typedef enum { VGE_LAYOUT_KP = 0, VGE_LAYOUT_NOKP = 1 } vge_layout;
int vge_layout_feat_dim(vge_layout layout); /* 2596 / 2356, 0 for an unknown layout */
#define VGE_CLIP_LEN 32
#define VGE_D_MODEL 256

/* Model shape (infer_dims_from_stats, eval.py:104-133; HumanActionScorer, model.py:102-148).
 * The kernels are built for the reference configuration: 5 modalities in the order
 * vit, global, pose, beta, kp2d with dims {1024,9,207,10,120} / {1024,3,69,10,120}, or the first 4 of them
 * (keypoint-less layout: 8 conv encoders, a 4-way fusion, feats rows of 2356), d_model 256, post-norm
 * layers, 8 heads, FFN 1024, clip_len 32.  Other checkpoint shapes (d_model 32..256 in steps of 32, any head count
 * with a head dim <= 64, FFN 4 d_model) run on the generic exact-f32 kernels (vge_encoder_gen.hip) when created
 * with VGE_F32; seq / frame embeddings are then d_model wide. */
typedef struct {
  int n_modalities;
  int dims_raw[8];
  int dims_diff[8];
  int d_model;
  int time_layers;
  int time_heads;
  int clip_len;
} vge_dims;

/* A named host tensor, named exactly as the reference state_dict key (model.py parameter names),
 * e.g. "state_enc.vit.blocks.0.conv1.weight" [256,256,5] or "temporal.layers.3.norm2.bias" [256]. */
typedef struct {
  const char* name;
  const float* data; /* host, contiguous float32 */
  int ndim;
  int64_t shape[4];
} vge_tensor_view;

typedef struct vge_encoder vge_encoder;

/* ---- frame store: the per-frame features of a set of videos, resident in HBM ----------------
 * Replaces the npz/keypoints.npy reads of WindowDataset._try_one (utils.py:383-425).
 * videos[v] = {frame_off, n_frames, kp_off, kp_frames} (int32, device); kp_frames = 0 means the
 * video has no keypoint file. */
typedef struct {
  const float* pose;   /* device [F,207] (23 rotmats) */
  const float* gori;   /* device [F,9]                */
  const float* betas;  /* device [F,10]               */
  const float* vit;    /* device [F,1024]             */
  const float* kp;     /* device [Fk,120]             */
  const int32_t* videos; /* device [V,4]              */
  int n_videos;
} vge_frame_store;

/* ---------------------------------------------------------------------------------------------
 * Featurisation.  Replaces WindowDataset._try_one (utils.py:383-516) incl. _slice_or_pad
 * (366-381), _vit_delta (142-147), _rotmat_delta/_log_so3 (130-140,165-174), _betas_delta
 * (161-163), _procrustes_kp_delta with LAPACK-convention 2x2 SVD (177-217) and the z-norm
 * (x-mean)/(std+1e-6) (472-494).
 *   windows : device int32 [n_windows,2] = {video index, start frame}
 *   mean,std: device float [2596] (ModalityStats in feats column order)
 *   feats   : device float [n_windows,32,2596]
 * vge_featurize_layout: the same for either layout; VGE_LAYOUT_NOKP (keypoint_dir None) reads no keypoints and
 *   takes mean/std [2356] and feats [n_windows,32,2356] in that layout's column order.
 */
int vge_featurize(const vge_frame_store* store, const int32_t* windows, int n_windows,
                  const float* mean, const float* std, float* feats, vge_stream_t stream);
int vge_featurize_layout(const vge_frame_store* store, const int32_t* windows, int n_windows, const float* mean,
                         const float* std, vge_layout layout, float* feats, vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * ModalityStats.  Replaces compute_stats_from_npz (utils.py:595-801) with _update_sum_sum2
 * (589-593): float64 per-column sum / sum of squares over all frames of the selected videos,
 * diffs on the full sequences; keypoint columns over keypoint frames only.
 *   host_videos    : host copy of store->videos [V,4] (tile planning happens on the host)
 *   host_video_sel : host int32 [n_sel] video indices into the store
 *   sums      : device double [2,2596] (sum, sum of squares) -- ACCUMULATED INTO (zero it first)
 *   counts    : host int64 [2] += {mesh frames, keypoint frames} of the selection
 *   workspace : device scratch of >= vge_stats_workspace_bytes(1) bytes; videos are processed in
 *               chunks of as many 32-frame tiles as fit (this call may synchronise the stream)
 * vge_stats_finalize turns (sums, counts) into float32 mean/std (std = sqrt(max(var,0)+1e-6),
 * utils.py:746-750).  Sums are the RCCL exchange payload when the real set is sharded.
 * vge_stats_finalize_layout writes mean/std in a layout's column order (VGE_LAYOUT_NOKP: [2356], the kp2d
 * columns dropped -- the reference's keypoint-less ModalityStats); the sums are always [2,2596].
 */
size_t vge_stats_workspace_bytes(int chunk_tiles);
int vge_stats_accumulate(const vge_frame_store* store, const int32_t* host_videos, const int32_t* host_video_sel,
                         int n_sel, double* sums, int64_t* counts, void* workspace, size_t workspace_bytes,
                         vge_stream_t stream);
int vge_stats_finalize(const double* sums, const int64_t* counts, float* mean, float* std, vge_stream_t stream);
int vge_stats_finalize_layout(const double* sums, const int64_t* counts, vge_layout layout, float* mean, float* std,
                              vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Encoder.  Replaces load_model (eval.py:136-165) + HumanActionScorer.forward (model.py:162-193).
 * create: validates every required key (missing -> VGE_ERR_MISSING_WEIGHT) and repacks the
 * weights into the library's MFMA panel layout in HBM (the handle owns them).
 * reserve: allocates the activation workspace for up to max_windows windows (outside timed
 * regions; compute calls never allocate).
 * encode: feats device [B,T,D] -> seq_embed device [B,256] (L2-normalised CLS), D = vge_encoder_feat_dim
 *   (2596, or 2356 for a 4-modality keypoint-less model),
 *   frame_embed device [B,T+1,256] or NULL, tc_window device [B] (per-window temporal coherence,
 *   eval.py:216-224) or NULL.
 */
int vge_encoder_create(const vge_dims* dims, const vge_tensor_view* weights, int n_weights, vge_dtype compute,
                       vge_encoder** out);
int vge_encoder_reserve(vge_encoder* enc, int max_windows);
int vge_encoder_destroy(vge_encoder* enc);
int vge_encoder_feat_dim(const vge_encoder* enc); /* feats row width the encoder reads: 2596 or 2356 (0: null) */
int vge_encode(vge_encoder* enc, const float* feats, int B, int T, float* seq_embed, float* frame_embed,
               float* tc_window, vge_stream_t stream);
/* Pipelining hook (no reference counterpart; the reference featurises batch k+1 in DataLoader workers while batch k
 * is encoded, eval.py:410-418): make `stream` wait until the conv stage of the most recent vge_encode on this
 * encoder -- the last reader of its feats -- has finished, so the next batch's vge_featurize can overwrite feats on
 * `stream` while this batch's fusion / transformer still run. */
int vge_encoder_wait_conv(vge_encoder* enc, vge_stream_t stream);
/* Pipelining hook (no reference counterpart): subsequent vge_encode calls run the stages after the fusion (token
 * GEMM, transformer, output normalisation / TC) on `tail` instead of their own stream (NULL: back to it).  The encode
 * stream keeps the conv stage and the fusion, so the caller can featurise and encode the next batch there while this
 * batch's transformer runs; seq_embed / frame_embed / tc_window are complete in `tail`'s order (read them there).
 * The next vge_encode's fusion waits for the previous encode's tail stages, which read the buffer it overwrites. */
int vge_encoder_set_tail_stream(vge_encoder* enc, vge_stream_t tail);

/* Per-stage device time of vge_encode, measured with hipEvents recorded on the encode stream around
 * each stage (used by bench.py for the roofline line).  profile_begin pre-creates events for up to
 * max_calls subsequent vge_encode calls (no allocation inside encode); profile_read synchronises on
 * the recorded events and returns the summed milliseconds per stage and the number of calls seen.
 * Stages: 0 conv encoders (MovementConvEncoder x10), 1 fusion pool, 2 token GEMM (+CLS/PE),
 *         3 transformer layers, 4 output normalisation + per-window TC. */
#define VGE_N_STAGES 5
int vge_encoder_profile_begin(vge_encoder* enc, int max_calls);
int vge_encoder_profile_read(vge_encoder* enc, double* stage_ms, int* n_calls);

/* The encoder's device status word: VGE_OK, or VGE_ERR_DEVICE once a completed launch raised it (the word is
 * host-mapped: no synchronisation here -- synchronise the encode stream first to cover launches in flight).
 * vge_encoder_clear_status resets it (tests).  No reference counterpart: the reference's torch ops cannot fail this
 * way; this is the kernel-side guard that keeps a broken invariant from being a silent wrong score. */
int vge_encoder_status(const vge_encoder* enc);
int vge_encoder_clear_status(vge_encoder* enc);
/* Which of the VGE_N_STAGES + 1 stage-boundary events profiled vge_encode calls record (bit k = event before stage k;
 * default all): each event is a queue marker, so a timed loop that only needs the conv stage records 0x3 and
 * profile_read reports the stages both of whose events were recorded (the others as 0).  Mask 0: later calls are not
 * profiled and take no slot (a caller can sample every k-th call inside a timed loop). */
int vge_encoder_profile_mask(vge_encoder* enc, int event_mask);

/* ---------------------------------------------------------------------------------------------
 * Metrics.
 * vge_tc_windows: compute_temporal_coherence_scores' per-window term (eval.py:216-224):
 *   tc[w] = mean_t ||f[w,t+1]-f[w,t]||_2 over rows 1..T of frame_embed [B,T+1,d] (CLS dropped).
 * vge_score_videos: per-video AC (eval.py:229-257) and TC (np.mean over windows, eval.py:226):
 *   windows of video v are [video_first_win[v], video_first_win[v+1]) (device int32 [V+1]);
 *   video_class[v] = centroid row or -1 (class not in label_dict -> ac[v] = NaN, no "ac" key).
 *   ac: device float [V]; tc: device double [V].
 */
int vge_tc_windows(const float* frame_embed, int B, int T1, int d, float* tc, vge_stream_t stream);
int vge_score_videos(const float* seq_embed, const float* tc_window, const int32_t* video_first_win,
                     const int32_t* video_class, const float* centroids, int V, int d, float* ac, double* tc,
                     vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Real-class centroids.  Replaces build_train_centroids_subset (utils.py:1018-1045):
 * sums.index_add_(0, y, z); counts.index_add_ -- a deterministic segmented reduction (segments of 512
 * windows, CENT_SEG in vge_score.hip, summed in window order, then the segment partials in segment order: the same bits for any
 * device or launch, within a few ulps of a sequential index_add_); d <= 256; class ids outside [0, C)
 * are ignored.  finalize = normalize(sums / counts.clamp_min(1)).
 * sums [C,d] / counts [C] (device float) are ACCUMULATED INTO and are the RCCL all-gather payload.
 */
int vge_centroid_accumulate(const float* seq_embed, const int32_t* class_id, int n_windows, int C, int d,
                            float* sums, float* counts, vge_stream_t stream);
int vge_centroid_finalize(const float* sums, const float* counts, int C, int d, float* centroids,
                          vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Held-out validation loss: the checkpoint-selection criterion of the reference's training loop
 * (evaluate_test_set, train.py:286-333: TCL + 10 x SupConWithHardNegatives against shuffled, reversed and static
 * windows; train.py:450-455 keeps the checkpoint with the lowest value), and the gradients of its two losses for the
 * training step (the *_grad entries at the end).  Every reduction runs in an
 * order fixed by the problem size (no floating-point atomics): two calls on the same input give the same bits.
 *
 * vge_time_gather: out[b,t,:] = feats[b, src[b,t], :] -- partial_shuffle_within_window, reverse_sequence and
 *   get_static_window (utils.py:65-95) as one index table (reverse: src[t] = T-1-t; static: src[t] = 0).
 *   feats / out: device float [B,T,D], 16-byte aligned, out must not alias feats; src: device int32 [B,T];
 *   T = 32, D a multiple of 4.  A bit-exact copy.  The caller owns the contract 0 <= src < T: the table is not
 *   validated on the device (an entry outside the range gives an unspecified row of the same window).
 *
 * vge_tcl_loss: TCL.forward (losses.py:6-34) with its [B,B] / [B] broadcast stated literally -- element (i,j) is
 *   divided by the denominator of row j.  With e_ij = exp(<z_i,z_j> / temperature), P(i) the same-label rows without
 *   i and N(i) the other-label rows:
 *     den_j  = sum_{k in P(j)} e_jk + k1 sum_{k in P(j)} exp(-<z_j,z_k>) + k2 sum_{k in N(j)} e_jk
 *     loss_i = (1 / |P(i)|) sum_{j in P(i)} -log(e_ij / den_j);   loss = mean_i loss_i
 *   emb: device float [B,d] (16-byte aligned); labels: device int32 [B]; loss: device double [1];
 *   1 <= B <= 8192; d a multiple of 32 in [32, 256]; workspace: device scratch of >= vge_tcl_workspace_bytes(B).
 *   Dot products, exp / log and sums in f64.  A row whose label appears once in the batch has |P(i)| = 0: its loss
 *   is 0/0 = NaN and so is the batch loss, exactly as in the reference, whose evaluate_test_set then skips the batch
 *   (train.py:312-313); every other input with finite exponentials gives a finite loss.
 *
 * vge_hardneg_loss: SupConWithHardNegatives.forward(anchor, anchor, neg) (losses.py:37-56):
 *   loss = mean_i [ logsumexp(s_ap, s_ah) - s_ap ], s_ap = <a_i,a_i> / temperature, s_ah = <a_i,n_i> / temperature
 *   (s_ap is computed, not taken as 1 / temperature).  anchor / neg: device float [B,d], 16-byte aligned, d a
 *   multiple of 4; loss: device double [1].
 *   The reference's weight of 10 (train.py:516-521) is the caller's.
 *
 * vge_centroid_distance: evaluate_test_set_centroid_distance's per-sample term (train.py:366-378):
 *   dist[i] = || normalize(emb_i) - centroids[labels[i]] ||_2 (F.normalize eps 1e-12), float32; a label outside
 *   [0, C) gives NaN (the reference's `continue`).  emb [n,d], centroids [C,d], dist [n]: device float.
 *
 * vge_tcl_loss_grad / vge_hardneg_loss_grad: the same losses with their gradients (what a training step needs), one
 *   call each.  `loss` is written by the forward entry's own kernels, so it has the forward's bits, NaN included.  The
 *   gradients are float64 inside (f32 products accumulated in f64, f64 exp) and are rounded to float32 once, at the
 *   store; no floating-point atomics, every sum in an order fixed by (B, d): two calls give the same bits.  The
 *   [B,B] matrix is never stored (the dot products are recomputed) and the workspace stays O(B).
 *   vge_tcl_loss_grad: grad: device float [B,d], not aliasing emb;  with s_jk = <z_j,z_k>, e_jk = exp(s_jk / t):
 *       k in P(j): W_jk = (e_jk / t - k1 exp(-s_jk)) / den_j - 1 / (t |P(j)|)
 *       k in N(j): W_jk = k2 e_jk / (t den_j);   W_jj = 0;   grad_j = (1 / B) sum_k (W_jk + W_kj) z_k
 *     the derivative of the loss above wherever every |P| >= 1 (the row-j broadcast and the row-i reading are then
 *     the same function of z).  When a label appears once `loss` is NaN as the forward's is and `grad` is
 *     unspecified: the caller skips that step.  Limits of vge_tcl_loss; workspace >= vge_tcl_grad_workspace_bytes(B).
 *   vge_hardneg_loss_grad: grad_anchor / grad_neg: device float [B,d], 16-byte aligned, aliasing nothing;  with
 *       p_i = sigmoid((<a_i,n_i> - <a_i,a_i>) / t):  grad_neg_i = p_i a_i / (t B),
 *       grad_anchor_i = p_i (n_i - 2 a_i) / (t B)   (anchor is the positive too: both of its uses carry gradient).
 */
int vge_time_gather(const float* feats, const int32_t* src, int B, int T, int D, float* out, vge_stream_t stream);
size_t vge_tcl_workspace_bytes(int B);
int vge_tcl_loss(const float* emb, const int32_t* labels, int B, int d, double temperature, double k1, double k2,
                 void* workspace, size_t workspace_bytes, double* loss, vge_stream_t stream);
int vge_hardneg_loss(const float* anchor, const float* neg, int B, int d, double temperature, double* loss,
                     vge_stream_t stream);
size_t vge_tcl_grad_workspace_bytes(int B);
int vge_tcl_loss_grad(const float* emb, const int32_t* labels, int B, int d, double temperature, double k1, double k2,
                      void* workspace, size_t workspace_bytes, double* loss, float* grad, vge_stream_t stream);
int vge_hardneg_loss_grad(const float* anchor, const float* neg, int B, int d, double temperature, double* loss,
                          float* grad_anchor, float* grad_neg, vge_stream_t stream);
int vge_centroid_distance(const float* emb, const int32_t* labels, const float* centroids, int n, int C, int d,
                          float* dist, vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One residual block of MovementConvEncoder (the reference's TemporalConvBlock, model.py:21-58) for training:
 * a forward that keeps what the backward needs, and the backward to every input and parameter.  Exact f32 on the
 * f32-input MFMA; activations channels-last.
 *
 *   x [B,T,C];  w1, w2 [C,C,5] in torch's Conv1d layout [C_out, C_in, k];  dilation d in {1, 2, 4, 8}, zero padding
 *   2 d;  mask [B,T,C] the dropout multiplier (entries 0 or 1 / (1 - p)), or NULL for all ones;  gamma, beta [C];
 *   eps 1e-5.   conv(v; W)[b,t,o] = sum_j sum_i v[b, t + (j - 2) d, i] W[o,i,j], rows outside 0 .. T-1 read as zero.
 *
 *   forward    a = conv(x; w1)          h = gelu(a) mask        u = conv(h; w2) + x        g = gelu(u)
 *              mean_b, rstd_b over the sample's (T, C), biased variance      g^ = (g - mean_b) rstd_b
 *              y = g^ gamma + beta          gelu(z) = z Phi(z) (the erf form),  gelu'(z) = Phi(z) + z phi(z)
 *   backward   dbeta[c] = sum_{b,t} dy      dgamma[c] = sum_{b,t} dy g^      q = dy gamma
 *              dg = rstd_b (q - mean_{t,c}(q) - g^ mean_{t,c}(q g^))         du = dg gelu'(u)
 *              dw2[o,i,j] = sum_{b,t} du[b,t,o] h[b, t + (j - 2) d, i]
 *              dh[b,s,i]  = sum_j sum_o du[b, s - (j - 2) d, o] w2[o,i,j]    da = dh mask gelu'(a)
 *              dw1[o,i,j] = sum_{b,t} da[b,t,o] x[b, t + (j - 2) d, i]
 *              dx = du + sum_j sum_o da[b, s - (j - 2) d, o] w1[o,i,j]
 *
 * Saved tensors: the forward writes a, u [B,T,C] and mean, rstd [B]; the backward takes them back with x, mask, the
 * weights and gamma (h is recomputed from a and mask).  Pass a, u, mean and rstd all NULL to a forward whose backward
 * will not run: nothing is saved then.
 * Shapes: C a multiple of 32 in [32, 256], 1 <= T <= 64, B >= 1 with B T C < 2^31, dilation in {1, 2, 4, 8}; anything
 * else returns VGE_ERR_UNSUPPORTED.  Every pointer is device memory, 16-byte aligned (VGE_ERR_ARG otherwise, and for
 * a NULL other than mask or the saved set); inputs may alias each other, an output or the workspace may overlap
 * nothing else that is passed (VGE_ERR_ARG).  workspace: >= vge_convblock_workspace_bytes(B, T, C) bytes for the
 * backward, which is enough for either call; the forward alone needs vge_convblock_forward_workspace_bytes(C), its two
 * weight images (VGE_ERR_WORKSPACE otherwise; 0 is returned for an unsupported shape); its contents do not carry over from one
 * call to the next -- the weights are repacked on the device in every call, because a training step changes them.
 * All of these checks run before the first HIP call.  No allocation, no host synchronisation, everything on `stream`.
 * Sums: a sample is owned by one workgroup, which forms its statistics; dgamma, dbeta, dw1 and dw2 are per-workgroup
 * partials in the workspace added by a second pass in index order.  No floating-point atomics; the order of every
 * sum is fixed by (B, T, C, dilation), so two calls on the same input give the same bits.  A NaN in one sample's x
 * stays in that sample's y (and reaches the parameter gradients); other samples' y and dx do not see it.
 */
size_t vge_convblock_workspace_bytes(int B, int T, int C);
size_t vge_convblock_forward_workspace_bytes(int C);
int vge_convblock_forward(const float* x, const float* w1, const float* w2, const float* mask, const float* gamma,
                          const float* beta, int B, int T, int C, int dilation, float* a, float* u, float* mean,
                          float* rstd, float* y, void* workspace, size_t workspace_bytes, vge_stream_t stream);
int vge_convblock_backward(const float* dy, const float* x, const float* w1, const float* w2, const float* mask,
                           const float* gamma, const float* a, const float* u, const float* mean, const float* rstd,
                           int B, int T, int C, int dilation, float* dx, float* dw1, float* dw2, float* dgamma,
                           float* dbeta, void* workspace, size_t workspace_bytes, vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * One layer of the temporal stack for training: nn.TransformerEncoderLayer(d_model = D, nhead = H,
 * dim_feedforward = F, batch_first = True), post-norm, ReLU, eps 1e-5; a forward that keeps what the backward needs,
 * and the backward to x and all twelve parameter tensors.  Exact f32; row-major activations [B,S,*].
 *
 *   x [B,S,D], S tokens (CLS + frames), d = D / H.  Parameters in torch's layouts: in_proj_weight Win [3D,D] (rows
 *   q, k, v) and in_proj_bias b_in [3D]; out_proj Wo [D,D], b_o [D]; linear1 W1 [F,D], c1 [F]; linear2 W2 [D,F],
 *   c2 [D]; norm1 g1, beta1 [D]; norm2 g2, beta2 [D].  Dropout multipliers (entries 0 or 1 / (1 - p)), each NULL for
 *   all ones: m_attn [B,H,S,S], m1 [B,S,D], m_ff [B,S,F], m2 [B,S,D].
 *   LN(u; g, beta) = u^ g + beta,  u^ = (u - mean_row) rstd_row,  rstd = 1 / sqrt(biased variance over D + eps).
 *
 *   forward    qkv = x Win^T + b_in     (q, k, v: columns 0, D, 2D; head h: columns h d .. h d + d - 1 of each)
 *              P[b,h,i,:] = softmax_j(<q_i, k_j> / sqrt(d))         o = (P m_attn) v          z = o Wo^T + b_o
 *              u1 = x + z m1            x1 = LN(u1; g1, beta1)      f = relu(x1 W1^T + c1) m_ff
 *              g = f W2^T + c2          u2 = x1 + g m2              y = LN(u2; g2, beta2)
 *   backward   LayerNorm, for (dy, u2, g2) and then (dx1, u1, g1):  dbeta = sum_rows dy,  dgamma = sum_rows dy u^,
 *                q = dy gamma,  du = rstd (q - mean_D(q) - u^ mean_D(q u^))
 *              dg = du2 m2              dW2 = dg^T f                dc2 = sum_rows dg
 *              da = (dg W2) m_ff [f > 0]       dW1 = da^T x1        dc1 = sum_rows da         dx1 = du2 + da W1
 *              dz = du1 m1              dWo = dz^T o                db_o = sum_rows dz        do = dz Wo
 *              per (b, h):  dv = (P m_attn)^T do      dP = (do v^T) m_attn     dS = P (dP - sum_j dP P)
 *                           dq = dS k / sqrt(d)       dk = dS^T q / sqrt(d)
 *              dWin = dqkv^T x          db_in = sum_rows dqkv       dx = du1 + dqkv Win
 *
 * Saved tensors: the forward writes qkv [B,S,3D], u1 [B,S,D], f [B,S,F], u2 [B,S,D] and stats [4][B S] = (mean1,
 * rstd1, mean2, rstd2); the backward takes them back with x, the masks, the four weights, g1, beta1 and g2.  P, o
 * and x1 are recomputed in the backward (from qkv and m_attn, and from u1).  Pass all five NULL to a forward whose
 * backward will not run: nothing but y is written then.
 * Shapes: D a multiple of 32 in [32, 256]; H divides D and d = D / H is a multiple of 16 and at most 64; F = 4 D;
 * 1 <= S <= 65; B >= 1 and every tensor below 2^31 elements; anything else returns VGE_ERR_UNSUPPORTED and the
 * workspace queries return 0.  Every pointer is device memory, 16-byte aligned (VGE_ERR_ARG otherwise, and for a NULL
 * other than a mask or the saved set); inputs may alias each other, an output or the workspace may overlap nothing
 * else that is passed (VGE_ERR_ARG).  workspace: >= vge_timelayer_workspace_bytes for the backward, which is enough for
 * either call; the forward alone needs vge_timelayer_forward_workspace_bytes (VGE_ERR_WORKSPACE otherwise); its
 * contents do not carry over from one call to the next.  All of these checks run before the first HIP call.  No
 * allocation, no host synchronisation, everything on `stream`.
 * Sums: a GEMM output is MFMA chains of 16 exact f32 products added in f64 and rounded to f32 once; the attention's
 * products are formed and summed in f64; softmax (row maximum subtracted) and LayerNorm row sums are f64 sums of f32
 * values.  Only the parameter gradients are summed across samples: f64 partials per chunk of rows in the workspace,
 * added by a second launch in chunk order.  No floating-point atomics; the order of every sum is fixed by
 * (B, S, D, H), so two calls on the same input give the same bits.  A NaN in one sample's x reaches that sample's y
 * and dx and the parameter gradients, and no other sample's y or dx.
 */
size_t vge_timelayer_workspace_bytes(int B, int S, int D, int H, int F);
size_t vge_timelayer_forward_workspace_bytes(int B, int S, int D, int H, int F);
int vge_timelayer_forward(const float* x, const float* in_proj_weight, const float* in_proj_bias,
                          const float* out_proj_weight, const float* out_proj_bias, const float* linear1_weight,
                          const float* linear1_bias, const float* linear2_weight, const float* linear2_bias,
                          const float* norm1_weight, const float* norm1_bias, const float* norm2_weight,
                          const float* norm2_bias, const float* m_attn, const float* m1, const float* m_ff,
                          const float* m2, int B, int S, int D, int H, int F, float* qkv, float* u1, float* f, float* u2,
                          float* stats, float* y, void* workspace, size_t workspace_bytes, vge_stream_t stream);
int vge_timelayer_backward(const float* dy, const float* x, const float* in_proj_weight, const float* out_proj_weight,
                           const float* linear1_weight, const float* linear2_weight, const float* norm1_weight,
                           const float* norm1_bias, const float* norm2_weight, const float* m_attn, const float* m1,
                           const float* m_ff, const float* m2, const float* qkv, const float* u1, const float* f,
                           const float* u2, const float* stats, int B, int S, int D, int H, int F, float* dx,
                           float* d_in_proj_weight, float* d_in_proj_bias, float* d_out_proj_weight,
                           float* d_out_proj_bias, float* d_linear1_weight, float* d_linear1_bias,
                           float* d_linear2_weight, float* d_linear2_bias, float* d_norm1_weight, float* d_norm1_bias,
                           float* d_norm2_weight, float* d_norm2_bias, void* workspace, size_t workspace_bytes,
                           vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * A bias-free linear map for training: the movement encoders' stems (1 x 1 convolutions) and projections.
 *
 *   x [R,K] with row stride ldx (floats) -- a column slice of a wider tensor is read in place --, W [N,K] as
 *   _ConvWeight.weight[:, :, 0] and _Linear.weight hold it, y and dy [R,N] dense.
 *
 *   forward    y[r,n]  = sum_k x[r,k] W[n,k]
 *   backward   dx[r,k] = sum_n dy[r,n] W[n,k]        (dx [R,K] dense; skipped when dx is NULL)
 *              dW[n,k] = sum_r dy[r,n] x[r,k]
 *
 * Shapes: R >= 1, 1 <= K <= 4096, N a multiple of 32 in [32, 256], R max(K, N, ldx) < 2^31: anything else returns
 * VGE_ERR_UNSUPPORTED (and the workspace query 0); ldx < K returns VGE_ERR_ARG.  x needs 4-byte alignment only -- it is
 * read with 16-byte loads where its address, ldx and K are all multiples of 4 floats, with scalar loads otherwise --;
 * every other pointer is device memory, 16-byte aligned (VGE_ERR_ARG otherwise, and for a NULL other than dx); inputs
 * may alias each other, an output or the workspace may overlap nothing else that is passed (VGE_ERR_ARG).  workspace:
 * >= vge_linear_workspace_bytes(R, K, N) bytes for the backward (VGE_ERR_WORKSPACE otherwise); the forward needs none.
 * All of these checks run before the first HIP call.  No allocation, no host synchronisation, everything on `stream`.
 * Sums: the temporal layer's GEMM rule -- MFMA chains of 16 exact f32 products added in f64 and rounded to f32 once; K
 * past the operand is zero in LDS and is never read from memory nor stored; dW is f64 partials per chunk of rows in the
 * workspace, added by a second launch in chunk order.  No floating-point atomics: two calls give the same bits.
 */
size_t vge_linear_workspace_bytes(int R, int K, int N);
int vge_linear_forward(const float* x, int ldx, const float* W, float* y, int R, int K, int N, vge_stream_t stream);
int vge_linear_backward(const float* dy, const float* x, int ldx, const float* W, float* dx, float* dW,
                        void* workspace, size_t workspace_bytes, int R, int K, int N, vge_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The modality fusion for training: the affine-free LayerNorm over each modality's token and the learned-query
 * attention over the M tokens of a row (vge/model.py _Fusion), forward and backward, in the folded form.  eps 1e-5.
 *
 *   s [R,M,D]: the per-modality sums of R = B T frames.  Parameters: latent [D], q_ln g_q, b_q [D], kv_ln g_kv, b_kv
 *   [D], Wq, Wk, Wv, Wo [D,D] (out, in), logit_temp, logit_bias [M].  m_attn [R,M]: the dropout multiplier of the
 *   attention weights (entries 0 or 1 / (1 - p)), NULL for all ones.
 *   LN^(v) = (v - mean_D(v)) rstd,  rstd = 1 / sqrt(biased variance over D + eps).
 *
 *   forward    t_m = LN^(s_m)          h_m = LN^(t_m)             kv_m = h_m g_kv + b_kv
 *              ql = LN^(latent) g_q + b_q      qv = Wq ql          u = Wk^T qv          (the same for every row)
 *              c_m = 1 / sqrt(D) / (softplus(logit_temp_m) + 1e-3)
 *              l_m = <kv_m, u> c_m + logit_bias_m      a = softmax_m(l)        ad_m = a_m m_attn_m
 *              p = sum_m ad_m kv_m     vp = Wv p        out = Wo vp
 *   backward   dWo = d_out^T vp        dvp = d_out Wo   dWv = dvp^T p          dp = dvp Wv
 *              da_m = <dp, kv_m> m_attn_m              dl_m = a_m (da_m - sum_j a_j da_j)
 *              dlogit_bias_m = sum_rows dl_m           dc_m = sum_rows dl_m <kv_m, u>
 *              dlogit_temp_m = -dc_m c_m sigmoid(logit_temp_m) / (softplus(logit_temp_m) + 1e-3)
 *              dkv_m = ad_m dp + dl_m c_m u            du = sum_rows sum_m dl_m c_m kv_m
 *              dg_kv = sum_rows sum_m dkv_m h_m        db_kv = sum_rows sum_m dkv_m
 *              LN^ backward, for (dkv_m g_kv, h_m, rstd1) and then (dt_m, t_m, rstd0):
 *                dv = rstd (q - mean_D(q) - v^ mean_D(q v^));   ds_m is the second one's result
 *              dWk = qv (x) du          dqv = Wk du     dWq = dqv (x) ql       dql = Wq^T dqv
 *              dg_q = dql LN^(latent)   db_q = dql      dlatent = LN^ backward of (dql g_q)
 *
 * Saved tensors: the forward writes stats [4][R M] = (mean0, rstd0 of s_m; mean1, rstd1 of t_m), a [R,M], p [R,D] and
 * vp [R,D]; the backward takes them back with s, m_attn and the parameters.  t, h and kv are recomputed from s.  Pass
 * all four NULL to a forward whose backward will not run: nothing but out is written then.
 * Shapes: R >= 1, 1 <= M <= 8, D a multiple of 32 in [32, 256], R M D < 2^31; anything else returns
 * VGE_ERR_UNSUPPORTED and the workspace queries return 0.  Every pointer is device memory, 16-byte aligned
 * (VGE_ERR_ARG otherwise, and for a NULL other than m_attn or the saved set); inputs may alias each other, an output
 * or the workspace may overlap nothing else that is passed (VGE_ERR_ARG).  workspace: >= vge_fusion_workspace_bytes for
 * the backward, which is enough for either call; the forward alone needs vge_fusion_forward_workspace_bytes
 * (VGE_ERR_WORKSPACE otherwise).  All of these checks run before the first HIP call.  No allocation, no host
 * synchronisation, everything on `stream`.
 * Sums: the four GEMMs over R rows and their gradients follow the linear node's rule.  Row sums (LayerNorm means and
 * variances, the dot products, the softmax sum, the pooling) are f64 sums rounded once; the softmax subtracts the row
 * maximum.  Only parameter gradients are summed across rows: f64 partials per 16 rows in the workspace, added by a
 * second launch in chunk order.  No floating-point atomics: two calls give the same bits.  A row's out and ds depend
 * on that row of s, d_out and m_attn alone.
 */
size_t vge_fusion_workspace_bytes(int R, int M, int D);
size_t vge_fusion_forward_workspace_bytes(int R, int M, int D);
int vge_fusion_forward(const float* s, const float* latent, const float* q_ln_weight, const float* q_ln_bias,
                       const float* kv_ln_weight, const float* kv_ln_bias, const float* Wq, const float* Wk,
                       const float* Wv, const float* Wo, const float* logit_temp, const float* logit_bias,
                       const float* m_attn, int R, int M, int D, float* stats, float* a, float* p, float* vp, float* out,
                       void* workspace, size_t workspace_bytes, vge_stream_t stream);
int vge_fusion_backward(const float* d_out, const float* s, const float* latent, const float* q_ln_weight,
                        const float* q_ln_bias, const float* kv_ln_weight, const float* kv_ln_bias, const float* Wq,
                        const float* Wk, const float* Wv, const float* Wo, const float* logit_temp,
                        const float* logit_bias, const float* m_attn, const float* stats, const float* a, const float* p,
                        const float* vp, int R, int M, int D, float* ds, float* d_latent, float* d_q_ln_weight,
                        float* d_q_ln_bias, float* d_kv_ln_weight, float* d_kv_ln_bias, float* d_Wq, float* d_Wk,
                        float* d_Wv, float* d_Wo, float* d_logit_temp, float* d_logit_bias, void* workspace,
                        size_t workspace_bytes, vge_stream_t stream);

const char* vge_last_error(void);
const char* vge_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VGE_H */
