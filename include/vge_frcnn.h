/*
 * vge_frcnn.h -- C ABI of TokenHMR's single-person gate detector in libvge.so: detectron2's COCO Faster R-CNN
 * X101-32x8d-FPN (ResNeXt-101 32x8d + FPN + RPN + ROIAlignV2 box head) on gfx950.
 *
 * Replaces (reference file:line):
 *   mesh_generator.py:69-73     get_cfg() + merge_from_file("COCO-Detection/faster_rcnn_X_101_32x8d_FPN_3x.yaml"),
 *                               ROI_HEADS.SCORE_THRESH_TEST = 0.25, DefaultPredictor(det2_cfg)
 *   mesh_generator.py:103-117   per frame: det2_predictor(f) -> instances; valid = (pred_classes == 0) & (scores >
 *                               0.5); a frame is used iff exactly one box is valid (its box is then the crop box);
 *                               a video with < 80 % such frames is rejected
 * and the third-party code it calls (detectron2, NOT in /root/reference, no pinned version, weights from the model
 * zoo at run time): DefaultPredictor (ResizeShortestEdge 800 / 1333 through PIL bilinear), GeneralizedRCNN
 * (pixel normalisation, size_divisibility 32), build_resnet_backbone (ResNeXt, FrozenBN, STRIDE_IN_1X1 False), FPN +
 * LastLevelMaxPool, StandardRPNHead + find_top_rpn_proposals, ROIPooler (ROIAlignV2), FastRCNNConvFCHead,
 * FastRCNNOutputLayers.inference, detector_postprocess.  Restated from the published code (oracle/frcnn.py lists every
 * convention); parity vs detectron2's trained weights is UNPINNED.
 *
 * Conventions as in vge.h: device pointers unless stated, asynchronous on the given stream, int status return.
 * Arithmetic: bf16 operands and activations, f32 accumulation / epilogues / box arithmetic, FrozenBN folded into the
 * conv weights at load.  Grouped 3x3 convolutions run as 64-channel block-diagonal slices of the implicit-GEMM conv.
 *
 * Frames are H x W with any aspect ratio; a detector takes a new frame size at any call (the workspace is rebuilt).
 * Pinned against the oracle (tests/test_frcnn.py, tests/test_frcnn_shapes.py): resized sizes from 1 x 333 and 64 x 107
 * to 800 x 800 and 750 x 1333, landscape and portrait, upscaled and downscaled, padded on either or both axes (padded
 * 32 x 352 .. 768 x 1344, P5 from 1 x 11 and 2 x 4 to 25 x 25 and 24 x 42).  Refused with VGE_ERR_ARG by
 * vge_frcnn_shapes / vge_frcnn_reserve / vge_frcnn_detect before any launch: a frame whose short edge rounds to 0
 * pixels under the max_size cap (aspect ratio above ~2 max_size, e.g. 1 x 667 at max_size 333), and a chunk whose
 * row or thread counts would pass 2^31.
 *
 * The non-GEMM kernels are also pinned one at a time, through the vge_op_* entries at the end of this header, on
 * crafted inputs (tests/test_frcnn_ops.py; the cases and the property each one carries: tests/frcnn_op_cases.py,
 * checked under the oracle alone by tests/test_frcnn_op_cases.py):
 *   vge_op_frcnn_preprocess   resized bytes == the oracle's PIL resample; the bf16 tensor bit for bit against
 *                             bf16((v - mean) / std) in numpy float32, BGR, +0 in channels 3..7 and in the padding
 *   vge_op_frcnn_pool_s2      == torch max_pool2d of the bf16 values (K 3 and 1, odd and even sizes)
 *   vge_op_frcnn_stem_pool    float64 conv 7x7 / 2 + bias + ReLU, one bf16 rounding, max_pool2d(3, 2, 1): 2^-7 |ref| + 1e-4
 *   vge_debug_gconv3          torch conv2d(groups) in f32, 2^-7 |ref| + 1e-4, at 1, 8, 9 and 17 images per call
 *   vge_op_rpn_proposals      oracle proposals(): counts and scores bit-equal in order (ties at the top-k cut, across
 *                             levels, IoU within 4 ulp of the threshold, NaN / inf logits and deltas, no valid box)
 *   vge_op_roi_align          oracle box_features(): 2^-7 |ref| + max(1e-6, 2^-20 sum |w v| / count), the three kernels
 *                             (vge_debug_set_roi_direct 0 / 1 / 2) at every level boundary, 13 / 14 samples per bin,
 *                             samples outside the map, empty slots
 *   vge_op_det_post           oracle inference() + postprocess(): counts, classes, order, persons equal; scores 2e-6
 */
#ifndef VGE_FRCNN_H
#define VGE_FRCNN_H

#include "vge.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int min_size, max_size;            /* INPUT.MIN_SIZE_TEST 800, MAX_SIZE_TEST 1333 */
  int depth;                         /* RESNETS.DEPTH 101 (blocks 3, 4, 23, 3); 50 and 152 accepted */
  int groups, width_per_group;       /* NUM_GROUPS 32, WIDTH_PER_GROUP 8 (bottleneck 256 .. 2048) */
  int stem_ch, res2_ch, fpn_ch;      /* 64, 256, 256 (fpn_ch must be 256) */
  int rpn_pre_topk, rpn_post_topk;   /* PRE_NMS_TOPK_TEST 1000, POST_NMS_TOPK_TEST 1000 (each <= 1024) */
  float rpn_nms;                     /* RPN.NMS_THRESH 0.7 */
  int fc_dim, num_classes;           /* ROI_BOX_HEAD.FC_DIM 1024, ROI_HEADS.NUM_CLASSES 80 */
  float score_thresh, nms_thresh;    /* 0.25 (mesh_generator.py:71), ROI_HEADS.NMS_THRESH_TEST 0.5 */
  int det_per_img;                   /* TEST.DETECTIONS_PER_IMAGE 100 */
  float gate_thresh;                 /* 0.5 (mesh_generator.py:106) */
} vge_frcnn_config;

typedef struct vge_frcnn vge_frcnn;

/* Weights: float32 host views with detectron2's state_dict keys:
 *   backbone.bottom_up.stem.conv1.{weight, norm.{weight,bias,running_mean,running_var}},
 *   backbone.bottom_up.res<2..5>.<b>.{conv1,conv2,conv3[,shortcut]}.{weight, norm.*} (conv2: [w, w / groups, 3, 3]),
 *   backbone.fpn_lateral<2..5>.{weight,bias}, backbone.fpn_output<2..5>.{weight,bias},
 *   proposal_generator.rpn_head.{conv, objectness_logits, anchor_deltas}.{weight,bias},
 *   roi_heads.box_head.{fc1,fc2}.{weight,bias}, roi_heads.box_predictor.{cls_score,bbox_pred}.{weight,bias}.
 * Missing key -> VGE_ERR_MISSING_WEIGHT, wrong shape -> VGE_ERR_WEIGHT_SHAPE. */
int vge_frcnn_create(const vge_frcnn_config* cfg, const vge_tensor_view* weights, int n_weights, vge_frcnn** out);
/* workspace for chunks of up to chunk_frames frames of H x W pixels (~250 MB per 800 x 800 frame) */
int vge_frcnn_reserve(vge_frcnn* m, int chunk_frames, int H, int W);
int vge_frcnn_destroy(vge_frcnn* m);

/* Geometry for frames of H x W: out[0..1] = resized (newh, neww), out[2..3] = padded (Hp, Wp), out[4 + 2 l],
 * out[5 + 2 l] = (h, w) of FPN level P(2 + l), l = 0..4; out[14] = row stride of the head tap (floats). */
int vge_frcnn_shapes(const vge_frcnn* m, int H, int W, int* out /* [15] */);

/* Optional intermediates for the parity tests (all device pointers, NULL = not wanted), frame-major: */
typedef struct {
  uint8_t* resized;       /* [F][newh][neww][3] RGB: the PIL bilinear resize of each frame */
  void* fpn[5];           /* bf16 [F][h_l][w_l][256]: P2..P6 */
  float* rpn[5];          /* f32 [F][h_l][w_l][16]: objectness logits (3) | anchor deltas (12) | unused */
  float* proposals;       /* f32 [F][rpn_post_topk][5]: x1 y1 x2 y2 (resized-image pixels), objectness logit */
  int32_t* n_proposals;   /* [F] */
  void* box_features;     /* bf16 [F][rpn_post_topk][49][256]: ROIAlign bins (ph, pw) x channels */
  float* head;            /* f32 [F][rpn_post_topk][shapes[14]]: cls logits (K + 1) | class box deltas (4 K) */
  float* pre_dets;        /* f32 [F][det_per_img][6]: fast_rcnn_inference output (resized-image pixels) */
  int32_t* n_pre_dets;    /* [F] */
} vge_frcnn_taps;

/* frames: device uint8 [F][H][W][3] RGB.  Outputs (device):
 *   dets      f32 [F][det_per_img][6] = x1 y1 x2 y2 (frame pixels), score, class -- the predictor's instances in
 *             score order (detector_postprocess applied); n_dets int32 [F]
 *   person    f32 [F][2][5] = box + score of the first two class-0 instances (zeros where absent)
 *   n_person  int32 [F] = number of class-0 instances with score > gate_thresh: the frame passes the gate of
 *             mesh_generator.py:106-108 iff it is 1 (the box is then person[f][0])
 * Any output may be NULL except n_person. */
int vge_frcnn_detect(vge_frcnn* m, const uint8_t* frames, int n_frames, int H, int W, float* dets, int32_t* n_dets,
                     float* person, int32_t* n_person, const vge_frcnn_taps* taps, vge_stream_t stream);

/* Device time over the next max_calls detect calls: stage_ms[0] = backbone + FPN + RPN convolutions (implicit
 * GEMMs), [1] = box head GEMMs (fc1 as a 7 x 7 valid conv, fc2, predictor), [2] = resize, pooling, proposal
 * selection / NMS, ROIAlign, box inference; flops_per_call[0] / [1] = the algorithmic GEMM FLOPs of stages 0 / 1
 * (grouped convolutions counted at their grouped size). */
int vge_frcnn_profile_begin(vge_frcnn* m, int max_calls);
int vge_frcnn_profile_read(vge_frcnn* m, double* stage_ms, int* n_calls, double* flops_per_call);

/* ---- The detector's non-GEMM kernels one at a time (tests, tools).  Each entry checks its arguments (VGE_ERR_ARG,
 * vge_last_error names the entry and the rule, no GPU work) and then calls the launcher vge_frcnn_detect calls.
 * Device pointers unless stated; an entry that packs weights, builds tables or needs scratch allocates them, runs on
 * `stream` and waits for it before returning. */

/* DefaultPredictor's preprocessing of n frames uint8 [n][H][W][3] RGB: resized (optional) uint8 [n][nh][nw][3], out
 * bf16 [n][hp][wp][8] = (B, G, R) normalised, channels 3..7 and the padding +0; (nh, nw) = ResizeShortestEdge(min_size,
 * max_size), (hp, wp) = those rounded up to 32 (vge_frcnn_shapes out[0..3]). */
int vge_op_frcnn_preprocess(const uint8_t* frames, int n, int H, int W, int min_size, int max_size, uint8_t* resized,
                            void* out, vge_stream_t stream);
/* max_pool2d(K, stride 2, pad K / 2) of x bf16 [n][H][W][C] -> y [n][(H - 1) / 2 + 1][(W - 1) / 2 + 1][C]; K 3 (after
 * the stem) or 1 (P6), C a multiple of 8. */
int vge_op_frcnn_pool_s2(const void* x, void* y, int n, int H, int W, int C, int K, vge_stream_t stream);
/* The fused stem: in bf16 [n][hp][wp][8], w HOST f32 [64][3][7][7] and b HOST f32 [64] (FrozenBN already folded;
 * packed as vge_frcnn_create packs them) -> out bf16 [n][hp / 4][wp / 4][64]; hp, wp multiples of 32. */
int vge_op_frcnn_stem_pool(const void* in, const float* w, const float* b, void* out, int n, int hp, int wp,
                           vge_stream_t stream);
/* find_top_rpn_proposals: levels = HOST array of 5 device pointers f32 [n][h_l][w_l][16] (vge_frcnn_taps.rpn), level_hw
 * = HOST int [10] (h_0, w_0, ...); level l has stride 4 << l and anchors of size 32 << l.  -> props f32
 * [n][post_topk][5], n_prop int32 [n].  Optional (NULL = internal): sel and kept f32 [n][5][1024][8] (per level: the
 * top-k entries x1 y1 x2 y2 logit valid, in key order; the boxes NMS kept, x1 y1 x2 y2 logit), kcount int32 [n][5]. */
int vge_op_rpn_proposals(const float* const* levels, const int* level_hw, int n, int pre_topk, int post_topk,
                         float nms_thresh, int img_h, int img_w, float* props, int32_t* n_prop, float* sel, float* kept,
                         int32_t* kcount, vge_stream_t stream);
/* ROIPooler: levels = HOST array of 4 device pointers bf16 [n][h_l][w_l][256] (P2..P5), level_hw = HOST int [8];
 * props f32 [n][P][5], n_prop int32 [n] (each <= P) -> out bf16 [n][P][49][256], slots from n_prop[f] on +0.  The
 * kernel is the one vge_debug_set_roi_direct selects. */
int vge_op_roi_align(const void* const* levels, const int* level_hw, const float* props, const int32_t* n_prop, int n,
                     int P, void* out, vge_stream_t stream);
/* FastRCNNOutputLayers.inference + detector_postprocess + the gate count: head f32 [n * P][ld] (logits K + 1 | deltas
 * 4 K), props f32 [n][P][5], n_prop int32 [n] (each <= P); img = the resized image, out = the frame.  vge_frcnn_create's
 * rules hold: score_thresh in [0.2, 1), K in [1, 127], det_per_img and P <= 1024.  Outputs as in vge_frcnn_taps
 * (pre_dets, n_pre) and vge_frcnn_detect (dets, n_dets, person, n_person); all optional but n_person. */
int vge_op_det_post(const float* head, int ld, int P, int K, int det_per_img, const float* props, const int32_t* n_prop,
                    int n, int img_h, int img_w, int out_h, int out_w, float score_thresh, float nms_thresh,
                    float gate_thresh, float* pre_dets, int32_t* n_pre, float* dets, int32_t* n_dets, float* person,
                    int32_t* n_person, vge_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VGE_FRCNN_H */
