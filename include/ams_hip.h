/*
 * ams_hip.h — C ABI of the MI355X-native AMS student hot path (libams_hip.so).
 *
 * The reference (modelstreaming/ams) has NO native boundary: its hot path is a Python object,
 * `SemanticNetwork` (reference SemanticNetwork.py:24), whose methods call `tf.Session.run` on a graph
 * assembled by `create_student_v3` (reference utils/graph_utils.py:338-533).  This header is the seam
 * a maintainer binds UNDER that class (ctypes stub in INTEGRATION.md): every entry point names the
 * reference call it replaces.  Plain pointers and sizes only; all `*_dev` pointers are HIP device
 * pointers owned by the caller (the Python host allocates them through PyTorch-ROCm); `stream` is a
 * `hipStream_t` passed as `void*` (0 = the null stream).  All functions return 0 on success or a
 * negative AMS_E_* code; `ams_last_error()` gives the message of the calling thread's last failure.
 *
 * Layouts: activations NHWC, dense; conv weights HWIO, depthwise weights HWC1 (TF layouts, so the
 * reference's `.npy` weight dicts load without transposition); frames `[B,H,W,3]` RGB 0..255 as uint8
 * or float32; label maps `[B,H,W]` (uint8 teacher ids in, int32 subset indices out).
 */
#ifndef AMS_HIP_H
#define AMS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMS_ABI_VERSION 6

enum {
    AMS_OK = 0,
    AMS_E_INVALID = -1,     /* bad argument (shape, dtype, mode, null pointer)           */
    AMS_E_HIP = -2,         /* a HIP runtime call or kernel launch failed                 */
    AMS_E_STATE = -3,       /* call not valid in this state (e.g. training a frozen net)  */
    AMS_E_NOMEM = -4        /* arena too small                                            */
};

/* layer roles: how the engine wires a row of the layer table (ams_amd/spec.py -> Appendix A of SURVEY.md) */
enum {
    AMS_ROLE_STEM = 0,       /* MobilenetV2/Conv: dense 3x3 s2 on the normalised frame          */
    AMS_ROLE_EXPAND = 1,     /* 1x1, BN, ReLU6                                                  */
    AMS_ROLE_DEPTHWISE = 2,  /* 3x3 depthwise (stride 1/2, rate 1/2), BN, ReLU6                 */
    AMS_ROLE_PROJECT = 3,    /* 1x1, BN, linear, optional residual add of the block input       */
    AMS_ROLE_POOL_CONV = 4,  /* image_pooling: global mean -> 1x1 -> BN -> ReLU (per image)     */
    AMS_ROLE_ASPP = 5,       /* aspp0: 1x1 -> BN -> ReLU                                        */
    AMS_ROLE_CONCAT_PROJ = 6,/* concat_projection over [pool branch, aspp0] -> BN -> ReLU       */
    AMS_ROLE_LOGITS = 7      /* logits/semantic: 1x1 + bias                                     */
};
enum { AMS_ACT_NONE = 0, AMS_ACT_RELU = 1, AMS_ACT_RELU6 = 2 };
enum { AMS_DT_F32 = 0, AMS_DT_U8 = 1, /* 2 was AMS_DT_BF16: bf16 activation storage, measured and dropped (profiles/r03_bf16_storage_study.json) */
       AMS_DT_I32 = 3, AMS_DT_F64 = 4 };
enum {
    AMS_MODE_FROZEN = 0,     /* BN with the statistics captured by ams_student_freeze, eps 1e-3 everywhere
                                (reference utils/graph_utils.py:52-76, :362-369; the graph the edge runs) */
    AMS_MODE_LIVE = 1        /* BN with batch statistics, per-layer eps (the live graph, is_training=True) */
};

/* one row of the layer table; offsets are in floats into the trainable / statistics arenas */
typedef struct ams_layer_desc {
    int32_t role;
    int32_t cin, cout;
    int32_t stride, rate;
    int32_t act;
    int32_t residual_from;   /* 1-based index of the layer whose output is added after BN, 0 = none */
    float bn_eps;            /* < 0: no BN (bias instead) */
    int64_t w_off;           /* weights    (trainable arena) */
    int64_t gamma_off;       /* BN gamma   (trainable arena), or bias offset when bn_eps < 0 */
    int64_t beta_off;        /* BN beta    (trainable arena) */
    int64_t mean_off;        /* moving_mean     (statistics arena) */
    int64_t var_off;         /* moving_variance (statistics arena) */
} ams_layer_desc;

typedef struct ams_student_config {
    int32_t abi_version;     /* AMS_ABI_VERSION */
    int32_t height, width;   /* frame size (reference: width = 2*height, run.py:71; not required here) */
    int32_t max_batch;       /* largest B any call will pass */
    int32_t num_classes;     /* 19 (Cityscapes) or 21 (VOC) */
    int32_t n_selected;      /* K: size of the per-video class subset */
    int32_t class_indices[32]; /* the K selected class ids, ascending (np.where(class_weights==1)) */
    int32_t n_layers;
    int32_t trainable;       /* 1: allocate activations/gradients/Adam state for ams_student_train_step */
    int32_t act_dtype;       /* AMS_DT_F32, the only storage type of activations.  bf16 storage of the output-stride-16 section was judged on
                                fine-tuned ("trained-like") weights, emulated by rounding (AMS_OPT_EMULATE_BF16_STORAGE): logits move by
                                8.4e-3 max / 3.3e-3 rms relative — outside the 1e-3 tolerance — although the labels change on 0.1 % of the
                                pixels only and mIoU by 0.002 pt (profiles/r03_bf16_storage_study.json); the bf16 variant that exists is
                                AMS_MATMUL_BF16 = bf16 products over f32 storage */
    int64_t n_trainable;     /* floats in the trainable arena (2 113 043 for Cityscapes) */
    int64_t n_stats;         /* floats in the statistics arena (33 088) */
    float bn_decay;          /* 0.9 (node BatchNorm/Const_2) */
    float bn_eps_frozen;     /* 1e-3 */
    float pixel_scale;       /* 1/127.5 as f32 (node mul_4/x) */
} ams_student_config;

typedef struct ams_student ams_student;

/* arena regions addressable from the host side (ams_student_region) */
enum {
    AMS_REGION_PARAMS = 0,   /* trainable arena, f32[n_trainable], tf.trainable_variables() order      */
    AMS_REGION_STATS = 1,    /* moving_mean / moving_variance, f32[n_stats]                             */
    AMS_REGION_GRADS = 2,    /* d loss / d params, f32[n_trainable] (valid after a train step phase)    */
    AMS_REGION_ADAM_M = 3,   /* f32[n_trainable]                                                         */
    AMS_REGION_ADAM_V = 4,   /* f32[n_trainable]                                                         */
    AMS_REGION_FROZEN = 5,   /* snapshot taken by ams_student_freeze: params followed by stats           */
    AMS_REGION_BN_SYNC = 6,  /* per-layer BN partial sums exchanged across ranks in data-parallel steps  */
    AMS_REGION_LOGITS = 7    /* low-resolution logits of the last forward, f32[B,h,w,num_classes]        */
};

const char* ams_last_error(void);
int ams_abi_version(void);
int ams_device_info(char* name_out, size_t name_cap, int32_t* n_cu, int64_t* hbm_bytes);

/* ---- lifecycle: replaces SemanticNetwork.__init__ (SemanticNetwork.py:32-159) / create_student_v3 ------- */
/* Bytes of device memory the engine needs for this configuration (activations, gradients, Adam, scratch). */
int ams_student_arena_bytes(const ams_student_config* cfg, const ams_layer_desc* layers, size_t* bytes_out);
/* Build the launch plan over caller-owned device memory `arena_dev` (>= arena_bytes, 256-byte aligned).
 * Parameters are NOT initialised: write them through ams_student_region views, then call
 * ams_student_freeze before the first AMS_MODE_FROZEN call. */
int ams_student_create(const ams_student_config* cfg, const ams_layer_desc* layers, void* arena_dev,
                       size_t arena_bytes, ams_student** out);
/* replaces SemanticNetwork.close_model (SemanticNetwork.py:716-717) */
void ams_student_destroy(ams_student* s);
/* byte offset into the arena and element count of a region */
int ams_student_region(const ams_student* s, int32_t region, size_t* offset_bytes, size_t* n_elems);
/* low-resolution feature size (h, w) = output stride 16 of the padded frame */
int ams_student_lowres_size(const ams_student* s, int32_t* h, int32_t* w);
/* Debugging / parity bisection (tools/grad_gap_bisect.py; no reference counterpart: tf.Session.run can fetch any tensor by name): byte offset
 * and element count of a per-layer training tensor of a TRAINABLE student, NHWC [max_batch, Hout, Wout, cout] — which = 0 raw conv output z,
 * 1 activated output a (= the next layer's input), 2 gradient wrt a (after a fine-tune step it holds dz where the step computed dz in
 * place), 3 gradient wrt z of a backbone layer (in place over 2, or a tensor of its own where 2 is read again as a skip gradient).  layer is 1-based (ams_layer_desc order).  Which of them a step actually writes depends on the fusion options: with every
 * AMS_OPT_TRAIN_* / FUSE_* fine-tune option at 0 all of them are.
 * The DEFAULT step (train_recompute 2, fuse_dgrad_bn 3, fuse_gemm_red 3, fuse_operand_bn 1) writes, with their plain meaning:
 *   z   of every layer but the expand layers of expanded_conv_1 .. _6 (those blocks go from their input straight to the depthwise z);
 *   a   of the project layers and of image_pooling, aspp0, concat_projection only (the stem's, the expand layers' and the depthwise layers'
 *       activations are applied on the consumer's loads of z and never stored);
 *   3   (dz) of the project layers, of the expand layers of expanded_conv_7 .. _16, of the depthwise layers of expanded_conv .. _6, of aspp0
 *       and concat_projection;
 *   2   (da) of the project layers that close a residual block.
 * 3 of a depthwise layer of expanded_conv_7 .. _16 holds dy = da * act'(BN(z)) where the apply pass ran inside the depthwise backward
 * kernel (from 256 rows = batch * pixels of that layer on, where the project layer's input-gradient GEMM fuses the BN-backward sums), and dz
 * below that; 2 / 3 of the stem and of the expand layers of expanded_conv_1 .. _6 are never written
 * (tests/layer_links.py default_step_stored gives the rule and the source line behind each entry). */
int ams_student_layer_tensor(const ams_student* s, int32_t layer, int32_t which, size_t* offset_bytes, size_t* n_elems);

/* ---- server -> edge hand-off: replaces save_to_frozen_graph / trim_graph_frozen / convert_batchnorms -----
 * (SemanticNetwork.py:706-714, utils/graph_utils.py:52-126).  Snapshots params + moving statistics into the
 * FROZEN region and folds every BN into (scale, shift) with eps = bn_eps_frozen.  Device-side, no protobuf. */
int ams_student_freeze(ams_student* s, void* stream);

/* ---- inference: replaces predict_input (SemanticNetwork.py:170-182), north-star `infer` ------------------
 * frames_dev: [B,H,W,3] uint8 or float32; labels_out_dev: int32 [B,H,W], index into the K selected classes. */
int ams_student_predict(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch,
                        int32_t mode, int32_t* labels_out_dev, void* stream);

/* ---- inference + metrics: replaces predict_with_metric (SemanticNetwork.py:196-213) ----------------------
 * teacher_dev: uint8 [B,H,W] teacher class ids (ids outside the subset are ignored, weight 0).
 * conf_mat_dev: int64 [K*K], rows = teacher, cols = student; OVERWRITTEN (the wrapper resets it per call).
 * loss_dev: double[2] = {sum of per-pixel CE over valid pixels, number of valid pixels}; loss = [0]/[1]. */
int ams_student_predict_with_metric(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch,
                                    int32_t mode, const uint8_t* teacher_dev, int32_t* labels_out_dev,
                                    int64_t* conf_mat_dev, double* loss_dev, void* stream);

/* ---- phi-score: replaces calc_cross_miou's confusion matrix (SemanticNetwork.py:124-139, :184-194) -------
 * labels_dev: uint8 [2,H,W] (before, after); conf_mat_dev: int64 [K*K] overwritten. */
/* The edge's per-frame call, several frames at a time: what ams_student_predict_with_metric computes for ONE frame, for each of `batch`
 * frames in one pass — labels [batch,H,W], conf_mats_dev [batch][K][K], losses_dev [batch][2] (teacher_dev NULL: labels only).  A frame at
 * a time the forward is ~45 dependent launches of 30-70 blocks on a 256-CU chip (0.49 ms); two frames take 0.59 ms, three 0.68 ms (MI355X):
 * a caller that can hold a frame for one or two frame times (33 ms at 30 fps) gets 1.7x / 2.2x the frames per second.  Every frame's result
 * is what a one-frame call returns (batch-composition invariance: tests/test_gpu_fullsize.py). */
int ams_student_predict_frames(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode,
                               const uint8_t* teacher_dev, int32_t* labels_out_dev, int64_t* conf_mats_dev, double* losses_dev, void* stream);

/* The same with the label maps as uint8 [batch,H,W] (an index inside the subset of K <= 32 classes fits a byte): what a caller that takes the
 * results to the HOST uses — a quarter of the device -> host bytes of the int32 maps, widened on the host (SemanticNetwork.predict_input /
 * predict_with_metric return int32 as the reference does: the widening of 0.5 MB costs less there than copying 2 MB out of the pinned buffer). */
int ams_student_predict_frames_u8(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode,
                                  const uint8_t* teacher_dev, uint8_t* labels_out_dev, int64_t* conf_mats_dev, double* losses_dev, void* stream);

/* The student's certainty about the frames of the LAST forward pass (any ams_student_predict* call; the fine-tune step leaves its batch's
 * logits there too): ams_k_upsample_confidence on the low-resolution logits that pass left on the device (AMS_REGION_LOGITS), one launch over
 * `batch` frames.  teacher_dev uint8 [batch,H,W] or NULL; conf_u8 / conf_f32 / stats as there, each may be NULL.  Launch it on the stream of
 * the pass and before the next one, which overwrites the logits.  batch outside 1..max_batch: AMS_E_INVALID, nothing written. */
int ams_student_confidence(ams_student* s, int32_t batch, const uint8_t* teacher_dev, uint8_t* conf_u8, float* conf_f32, int64_t* stats,
                           void* stream);

/* The soft-teacher loss and the probabilistic confusion matrices of the frames of the LAST forward pass: ams_k_upsample_soft_metric on the
 * low-resolution logits that pass left on the device (AMS_REGION_LOGITS, read in place), one launch over `batch` frames.  teacher_dev uint8
 * [batch,H,W] or NULL; teacher_logits_dev f32 [batch,th,tw,num_classes]; stats / p_f32 / ce_f32 as there, each may be NULL.  Launch it on the
 * stream of the pass and before the next one, which overwrites the logits.  The batch and the teacher grid are arguments: the call does not read
 * the feed armed by ams_student_feed_teacher_logits.  batch outside 1..max_batch: AMS_E_INVALID, nothing written. */
int ams_student_soft_metric(ams_student* s, int32_t batch, const uint8_t* teacher_dev, const float* teacher_logits_dev, int32_t th, int32_t tw,
                            int64_t* stats, float* p_f32, float* ce_f32, void* stream);
/* The same for teacher logits in either layout (AMS_TLOGITS_*, below; utils/graph_utils.py:359, 375-376): AMS_TLOGITS_SELECTED reads
 * teacher_logits_dev as f32 [batch,th,tw,n_selected].  A layout other than the two: AMS_E_INVALID, nothing launched, nothing written. */
int ams_student_soft_metric_layout(ams_student* s, int32_t batch, const uint8_t* teacher_dev, const float* teacher_logits_dev, int32_t th, int32_t tw,
                                   int64_t* stats, float* p_f32, float* ce_f32, void* stream, int32_t layout);

int ams_cross_confusion(const ams_student* s, const uint8_t* labels_dev, int64_t n_pixels, int64_t* conf_mat_dev,
                        void* stream);

/* ---- one optimisation step: replaces sess.run({train, loss}) in _train (SemanticNetwork.py:253-260),
 * north-star `train_step`.  forward (BN batch stats) -> masked mean CE over the K classes -> backward ->
 * BN moving-average update (decay bn_decay) -> Adam (TF1 form, beta 0.9/0.999, eps 1e-8).
 * mask_dev: NULL for 'full_model', else uint8[n_trainable]: entries with 0 are reverted after the Adam step
 * while their moments still advance (utils/graph_utils.py:482-493).  loss_dev: double[2] as above (the loss of
 * the forward pass, before the update).  Adam's step counter lives in the handle and is never reset. */
int ams_student_train_step(ams_student* s, const void* frames_dev, int32_t frames_dtype, const uint8_t* teacher_dev,
                           int32_t batch, float lr, const uint8_t* mask_dev, double* loss_dev, void* stream);

/* Range of the default product form (AMS_MATMUL_SPLIT_F16): fp16 holds |x| < 65520, and the two-part split keeps 22 bits only while its parts
 * are normal fp16 numbers (|x| >= 2^-14).  ams_student_freeze checks the frozen weights of every layer that has fp16 panels; a layer with a weight
 * beyond 65504 (or a non-finite one), or whose largest |w| is below 2^-10, runs on three bf16 parts (f32's range) until a later freeze finds it
 * inside again — *n_layers = how many layers the last freeze moved.  Activations are not checked. */
int ams_student_f16_fallback_layers(const ams_student* s, int32_t* n_layers);

/* ---- create_student_v3's remaining kwargs (utils/graph_utils.py:338-339; run.py:150 leaves all three off) -------------------------------
 * soft_teacher=True (option AMS_OPT_SOFT_TEACHER): pixel_loss = softmax_cross_entropy_with_logits(logits = filtered_logits, labels =
 * softmax(gather(teacher_labels_logits_pl, class_weights))) (:375-376, 403-404) — per pixel sum_k p_k (logsumexp(z) - z_k), gradient
 * softmax(z) - p; the pixel mask and the mean's denominator still come from the hard labels (:397, 406-408), which every step keeps taking.
 * ams_student_feed_teacher_logits replaces feed_dict[student['teacher_labels_logits_pl']]: f32 [batch, th, tw, num_classes] on the device,
 * valid until the step that uses it has run; it stays armed until replaced or cleared with NULL.  th x tw = height x width is the reference's
 * feed (the loss needs the shape of filtered_logits); a smaller grid (cached low-resolution teacher logits: 1 / 256 of the bytes at output
 * stride 16) is interpolated to height x width like the student's own logits (ResizeBilinear, align_corners) — an extension, at the full size
 * the identity bit for bit.  A step with the option on and nothing fed fails (TensorFlow: "You must feed a value for placeholder tensor").
 *
 * regularize=True / train_biases_only=True: loss += coef * reduce_mean([l2_loss(v) for v in tvars]) with coef = 0.01, l2_loss(v) = sum(v^2) / 2,
 * tvars = the trainable variables, or only those without 'weight' in their name (:451-456; the optimizer still updates every variable — the
 * reference's minimize() has no var_list).  reg_mask_dev: uint8 [n_trainable], 1 on the entries of tvars (it stays referenced: keep it alive;
 * NULL switches the term off); n_vars = len(tvars).  The gradient term (coef / n_vars) v is added after the cross-rank gradient sum of a
 * data-parallel step, the loss term to loss_dev[0] scaled by the valid-pixel count, so that loss_dev[0] / loss_dev[1] is the fetched loss. */
int ams_student_feed_teacher_logits(ams_student* s, const float* teacher_logits_dev, int32_t th, int32_t tw);

/* Layouts of teacher logits (the feed of teacher_labels_logits_pl, utils/graph_utils.py:359; the loss reads gather(teacher logits,
 * class_weights) alone, :375-376).  AMS_TLOGITS_FULL: f32 [..., num_classes], what the reference feeds.  AMS_TLOGITS_SELECTED: f32 [..., K],
 * channel k holding what the full layout holds at class_indices[k] — the gather done once, when a frame enters the replay memory
 * (ams_replay_pack_logits), instead of per pixel and step.  Every kernel that reads teacher logits runs the same instantiation on either
 * layout, so the results are equal bit for bit.  The entries without _layout take AMS_TLOGITS_FULL. */
enum { AMS_TLOGITS_FULL = 0, AMS_TLOGITS_SELECTED = 1 };

/* ams_student_feed_teacher_logits with the layout named (utils/graph_utils.py:359, 375-376): AMS_TLOGITS_SELECTED feeds f32 [batch, th, tw,
 * n_selected] in the order of the student's class_indices.  A layout other than the two: AMS_E_INVALID, the armed feed stays as it was. */
int ams_student_feed_teacher_logits_layout(ams_student* s, const float* teacher_logits_dev, int32_t th, int32_t tw, int32_t layout);
int ams_student_set_regularizer(ams_student* s, const uint8_t* reg_mask_dev, int32_t n_vars, float coef);

/* The two knowledge-distillation knobs of the soft-teacher step (this project's own objective; the reference has neither).  Per valid pixel,
 * z = the student's K logits, t = the teacher's, y = the hard label's index: q = softmax(z / T), p = softmax(t / T), s = softmax(z),
 *   pixel = alpha T^2 sum_k p_k (logsumexp(z / T) - z_k / T) + (1 - alpha) (logsumexp(z) - z_y),
 *   d pixel / d z_k = alpha T (q_k - p_k) + (1 - alpha) (s_k - [k = y]);
 * mask and denominator from the hard labels as before.  temperature finite and > 0 (1 / T and T^2 finite in f32), alpha in [0, 1]; anything else:
 * AMS_E_INVALID and the student keeps what it had.  Needs a trainable student.  Read only while AMS_OPT_SOFT_TEACHER is on.  The default
 * (1, 1) is the reference's soft loss and alpha = 0 the hard-label loss, each by the very kernel that computes it without this call.  The
 * evaluation entries (ams_student_soft_metric, ams_k_upsample_soft_metric) keep reporting the reference's T = 1 soft loss. */
int ams_student_set_kd(ams_student* s, float temperature, float alpha);

/* Weights of the fine-tune loss (this project's own; the reference has none).  class_weights_host: HOST array of n = n_selected floats cw_k in the
 * order of class_indices, each 0 or in [2^-6, 16]; NULL = all ones.  conf_gamma in [0, 8]: the exponent of the teacher's confidence
 * c = max_k p_k, p = softmax(t / T) the very target distribution of ams_student_set_kd; read only on a soft-teacher step, where a step with
 * conf_gamma > 0 and AMS_OPT_SOFT_TEACHER off is refused.  Per valid pixel w = cw_y c^gamma, quantised once to w_q = rint(w 2^20) 2^-20, and
 *   loss = sum w_q pixel / sum w_q,   dlogits = sum w_q d / sum w_q      (pixel, d: whichever form of the loss is set),
 * so loss_dev[1] of a step is sum w_q instead of the pixel count; a class of weight 0 is left out like an ignored label, and sum w_q = 0 is the
 * batch without a valid pixel (NaN loss, zero gradients; AMS_OPT_NAN_GRADS).  AMS_E_INVALID, the student keeping what it had: n != n_selected;
 * a weight that is NaN, negative, in (0, 2^-6) or above 16; conf_gamma outside [0, 8] or not finite.  Needs a trainable student.  All ones
 * with conf_gamma = 0 (the default) run the kernels that run without this call: the same bits.  Evaluation entries stay unweighted. */
int ams_student_set_loss_weights(ams_student* s, const float* class_weights_host /* n_selected, or NULL = ones */, int32_t n, float conf_gamma);

/* Hard-pixel mining (DeepLab's top_k_percent_pixels; the reference has none): the step's loss and gradient are those of the objective above over
 * the fraction top_k of the valid pixels whose own objective value is largest.  Per pixel, in f32,
 *   key = max(0, w_q pixel)            (pixel, w_q: as ams_student_set_kd and ams_student_set_loss_weights define them; a NaN counts as 0);
 * a pixel is valid when its label is in the class subset and w_q > 0, n = the valid pixels of the batch, k = max(1, floor((double)top_k n)),
 * threshold = the k-th largest key, kept = the valid pixels with key >= threshold: ties at the threshold are all kept (kept >= k) and nothing
 * depends on an order.  The mean is over the kept pixels: loss_dev[1] is their number (their weight sum under weights).  n, k and the threshold
 * are formed on the device: a memset pair and eight launches in front of the loss kernel (mining_key_kernel, three mining_hist_kernel +
 * mining_scan_kernel passes of a radix select, mining_relabel_kernel), no host round trip.  The loss kernels are the unmined step's: they run
 * on a label map in which every dropped pixel reads 255.
 *
 * scratch_dev: the caller's, 16-byte aligned, at least ams_k_loss_mining_scratch(max_batch, height, width) bytes (the key map, the mined labels,
 * the histograms and the result); it stays referenced: keep it alive.  The student's arena does not change.  top_k = 1 switches mining off (NULL
 * scratch allowed): the step then launches what it launches without this call, the same bits.  AMS_E_INVALID, the student keeping what it had:
 * top_k outside (0, 1] or not finite; with top_k < 1 a scratch that is NULL, misaligned or too small, or a student whose size is outside the
 * one-pass loss kernel (ams_k_ce_loss_grad).  Needs a trainable student.  A step with top_k < 1 and an all-reduce callback or an RCCL
 * communicator is refused before anything is launched: a global threshold needs the ranks' histograms summed.  Evaluation stays unmined. */
typedef struct ams_mining_result {
    float threshold;         /* the k-th largest key (0 without a valid pixel) */
    int64_t valid;           /* n */
    int64_t rank;            /* k */
    int64_t kept;            /* valid pixels with key >= threshold */
} ams_mining_result;
/* A scratch block for batches of up to B frames, n = B H W: the result at byte 0, the histograms behind it, the key map f32 [n] at
 * AMS_MINING_KEYS_OFFSET and the mined labels uint8 [n] at AMS_MINING_KEYS_OFFSET + 4 n rounded up to 16 (a step of fewer frames fills the
 * front of both maps). */
#define AMS_MINING_KEYS_OFFSET 24832
size_t ams_k_loss_mining_scratch(int32_t B, int32_t H, int32_t W);      /* bytes; 0 for a size < 1 */
int ams_student_set_loss_mining(ams_student* s, float top_k, void* scratch_dev, size_t scratch_bytes);
/* The result block of the last mined step, copied to the host after `stream` has drained.  AMS_E_STATE before the first mined step. */
int ams_student_mining_result(ams_student* s, ams_mining_result* out_host, void* stream);

/* ---- data-parallel split of the same step (one process per GPU) -------------------------
 * Callback form (any transport; what the gloo CPU tests and a host without RCCL use): `cb` is invoked on the host
 * whenever cross-rank sums are needed and must all-reduce (sum) `count` values of `dtype` at arena byte offset
 * `offset_bytes`, ordered after the work already enqueued on `stream`.  With cb == NULL the step is the single-GPU
 * step above.  Call sites: per-BN-layer (sum, sumsq) forward, (CE sum, valid-pixel count), per-BN-layer
 * (sum dy, sum dy*xhat) backward, and the flat gradient arena before Adam.  ams_student_train_step_rccl below is
 * the production form. */
typedef int (*ams_allreduce_cb)(void* user, size_t offset_bytes, size_t count, int32_t dtype);
int ams_student_train_step_dp(ams_student* s, const void* frames_dev, int32_t frames_dtype,
                              const uint8_t* teacher_dev, int32_t batch, int32_t global_batch, float lr,
                              const uint8_t* mask_dev, double* loss_dev, ams_allreduce_cb cb, void* user,
                              void* stream);

/* The same step with the exchange done by the library itself: every cross-rank sum is one ncclAllReduce on `stream`, issued in launch
 * order with no host round trip in between (110 per step: 54 BN forward, loss, 54 BN backward, the gradient arena).  librccl is
 * resolved at run time (dlopen; inside a PyTorch-ROCm process the copy PyTorch loaded is reused), so the library loads without it.
 *   rank 0: ams_comm_unique_id(id, 128) -> ship the 128 bytes to every rank (torch.distributed broadcast, a file, ...)
 *   all   : hipSetDevice(local gpu); ams_comm_create(id, 128, rank, world, &comm)   (world == 1: a no-op communicator)
 * One process per GPU, as the reference runs one process per --gpu (run.py:28). */
typedef struct ams_comm ams_comm;
int ams_comm_unique_id(uint8_t* id_out, size_t cap);
int ams_comm_create(const uint8_t* id, size_t id_len, int32_t rank, int32_t world, ams_comm** out);
void ams_comm_destroy(ams_comm* c);
int ams_comm_stats(const ams_comm* c, int32_t* rank, int32_t* world, int64_t* calls, int64_t* bytes);
/* Diagnostics of a multi-GPU run (bench.py `collective_ms_per_step`): with timing enabled every collective the communicator issues is
 * bracketed by a HIP event pair on its stream (the pair costs a few microseconds of stream time per collective: enable it for a few
 * diagnostic steps, not for the timed ones).  ams_comm_timing_read synchronises the device and returns the summed and the longest span and
 * their count since the last ams_comm_set_timing; a span is the time the stream spent INSIDE the collective (wait for the peers included). */
int ams_comm_set_timing(ams_comm* c, int32_t enable);
int ams_comm_timing_read(ams_comm* c, double* total_ms, double* max_ms, int64_t* spans);
int ams_comm_allreduce(ams_comm* c, void* buf_dev, size_t count, int32_t dtype, void* stream);
int ams_student_train_step_rccl(ams_student* s, const void* frames_dev, int32_t frames_dtype, const uint8_t* teacher_dev,
                                int32_t batch, int32_t global_batch, float lr, const uint8_t* mask_dev, double* loss_dev,
                                ams_comm* comm, void* stream);

/* ---- options -----------------------------------------------------------------------------------------------
 * AMS_OPT_MATMUL selects how the products of the 1x1-conv layers that would be matrix-pipe bound in exact f32 are formed
 * (few rows, a large weight panel, or >= 20 FLOP per byte: the output-stride-16 layers and the head):
 *   AMS_MATMUL_F32           exact f32 MFMA (v_mfma_f32_16x16x4_f32) everywhere
 *   AMS_MATMUL_SPLIT_BF16_X6 (default) operands split into three bf16 parts (all 24 significand bits), 6 bf16 MFMAs per 32 k,
 *                            f32 accumulate: products at f32 rounding level; 512x1024 logits 4e-5 from the f64 oracle, the
 *                            same as exact f32 and as the f32 CPU oracle (tools/logit_error.py)
 *   AMS_MATMUL_SPLIT_F16     frozen inference with two fp16 parts / 3 MFMAs, f32-level (see the enum below)
 *   AMS_MATMUL_SPLIT_BF16    frozen inference with two parts / 3 MFMAs: +5 % frames/s, ~1e-5 per layer, 2e-4 .. 5e-4 on
 *                            the logits (inside the 1e-3 tolerance, not at f32 level); the fine-tune step stays three-part. */
enum { AMS_OPT_FUSE_HEAD = 26 /* frozen inference, two bits (default 3).  Bit 0: the head's three GEMMs (aspp0, concat_projection, logits) as ONE chained
                                kernel where all three run the two-fp16-part product (k_head_chain.hip: the 256-wide f32 tensors between them are never
                                written; not under AMS_OPT_LATE_SUBBATCH).  Bit 1: the project GEMMs whose f32 result nothing reads (the next block streams
                                on the part planes and adds no residual) store the planes only.  0 = three launches, every store.  Same bits for every value */,
       AMS_OPT_SOFT_TEACHER = 25 /* fine-tune step: 1 = soft-teacher loss (ams_student_feed_teacher_logits); 0 (default) hard labels */,
       AMS_OPT_TRAIN_FWD_F16 = 24 /* fine-tune step under AMS_MATMUL_SPLIT_F16: 1 = the FORWARD 1x1 products of the split layers run on two fp16
                                      parts (3 MFMAs; the per-step weight split leaves fp16 planes beside the bf16 ones), the input-gradient and weight-
                                      gradient products stay on three bf16 parts (gradients span a range fp16 cannot hold); 0 (default) = three bf16
                                      parts everywhere.  Measured on MI355X: 7.455 -> 7.368 ms per 8-frame step — the step's GEMMs are not MFMA-bound
                                      at 17160 rows — so the default keeps one product form for the whole step */,
       AMS_OPT_WGRAD_FORK_EVERY = 23 /* fine-tune step with AMS_OPT_OVERLAP_WGRAD: weight gradients handed to the side stream n at a time, 1 .. 64
                                         (default 1 = each as soon as its operands exist).  A hand-over is an event on the main stream (a gap of
                                         6-8 us in the rocprofv3 timeline), and a weight gradient feeds only the optimizer, so it may start late —
                                         but measured on MI355X batching is SLOWER: 7.98 / 8.07 / 8.16-8.30 / 8.30 / 8.58 ms per step for n = 1 / 2 /
                                         4 / 8 / 16 (a weight gradient that runs beside the input-gradient GEMM of the same dz shares its cache
                                         lines).  Bit-identical for every n. */,
       AMS_OPT_FUSE_OPERAND_BN = 22 /* fine-tune step: 1 (default) BN + activation of every depthwise layer that feeds a project layer is applied by the
                                        CONSUMERS on their operand loads (project GEMM forward, project weight gradient backward: PwArgs / WgArgs
                                        x_mode 1) with the same IEEE operations in the same order, and the depthwise activation is never written:
                                        bit-identical to 0 = the pass written (bn_act).  The same move for dz = A dy + B + C z of the project and the
                                        stride-16 expand layers (x_mode / dy_mode 2, kept at kernel level: ams_k_pointwise_xform) measured SLOWER in
                                        the step on MI355X (8.31 -> 8.64 / 8.87 ms: those GEMMs are bound by their operand path) and is not wired in. */,
       AMS_OPT_NAN_GRADS = 18 /* fine-tune step on a batch WITHOUT a valid pixel: 0 (default) the reference's result — NaN loss (utils/graph_utils.py:408:
                                  tf.reduce_mean over the empty tf.boolean_mask) and ZERO gradients (the backward of that mean over a [0]-shaped tensor is
                                  empty, boolean_mask's gather gradient densifies it to zeros): parameters, Adam moments and BN statistics stay finite;
                                  1 = every gradient NaN instead, for callers who want such a batch to fail loudly */,
       AMS_OPT_OVERLAP_WGRAD = 19 /* fine-tune step: 1 (default) weight gradients on a side stream beside the input-gradient chain, 2 depthwise ones on a
                                     third stream (measured slower), 3 hand-overs alternate between two side streams (measured slower: 8.14 vs 7.98 ms),
                                     0 everything on the caller's stream.  Same bits */,
       AMS_OPT_OVERLAP_HEAD = 20 /* frozen inference: 1 = the image-pooling branch on a side stream beside the aspp0 GEMM; 0 (default): measured slower */,
       AMS_OPT_STREAM_MIN_ROWS = 21 /* frozen inference: rows (frames x pixels at the block's resolution) from which the streaming expand+depthwise
                                       kernels run (default 4096: from two 512x1024 frames per pass on; same bits either way) */,
       AMS_OPT_DUAL_AUTOTUNE = 12 /* with AMS_OPT_DUAL_STREAM = 1: 1 = pick the number of parts per batch size by TIMING the plans inside the first call
                                      with that batch size (median of three passes each; that call synchronises the host and its result then depends
                                      on which plan won); 0 (default) = the static rule: the same call always runs the same plan */,
       AMS_OPT_DUAL_PARTS = 13 /* parts (2 .. 4) of the forced split, AMS_OPT_DUAL_STREAM = n >= 2 */,
       AMS_OPT_EMULATE_BF16_STORAGE = 15 /* STUDY ONLY (tools/bf16_storage_study.py), default 0: frozen inference rounds the depthwise results and
                                            the block inputs of the output-stride-16 section to bf16 after they are written — the values bf16
                                            STORAGE of those tensors would hold; the arithmetic and every other tensor stay f32.  Costs a pass per
                                            tensor: an accuracy probe, not a fast path */,
       AMS_OPT_FUSE_DGRAD_BN = 16 /* fine-tune step, stride-1 blocks that keep their tensors (blocks 7-16): >= 1 the depthwise input gradient,
                                     the expand layer's activation derivative and BN-backward sums, and the depthwise weight gradient come out of
                                     ONE kernel (k_conv.hip: dw3x3_dgrad_bn_kernel); 2 (default) the forward too: the depthwise conv applies the
                                     expand layer's BN + activation on its tap loads and leaves the statistics of its result (dw3x3_fwd_bn_kernel) —
                                     the expand activation is never written; 3 (default) the depthwise layer's OWN apply pass (dz_d = A dy + B + C z_d) is folded into
                                     that backward kernel too, through an LDS ring (k_dw_train.hip); 0 separate passes.  Same mathematics, f32-level differences */,
       AMS_OPT_FUSE_GEMM_RED = 17 /* fine-tune step, BN column reductions in the epilogue of the 1x1 GEMM that holds the values in registers
                                     (pw_common.hpp pw_red_*): bit 0 the forward statistics of the GEMM's own result, bit 1 the BN-backward sums of the
                                     layer whose output gradient the dgrad GEMM produces.  Default 3; 0 = separate reduction passes.  Same mathematics,
                                     f32-level differences (partial sums per row strip instead of per column chunk) */,
       AMS_OPT_TRAIN_RECOMPUTE = 11 /* fine-tune step: >= 1 the early blocks (block input <= 32 channels) run without their 6x-expanded
                                       tensors — every consumer recomputes z_e = x . W_e from the block input (k_xdw_train.hip); 0 the
                                       layer-by-layer step (every tensor materialised); 2 (default) the expand layer's BN statistics additionally come from the
                                       Gram matrix of the block input (z_e is linear in x: sum z = g0 . w, sum z^2 = w^T XX w, XX accumulated in f64 in one
                                       cheap pass over x, k_xx_stats.hip) instead of a pass that recomputes z_e.  Same mathematics, f32-level differences. */,
       AMS_OPT_DUAL_STREAM = 10 /* frozen inference: a batch as two to four parts on as many streams (the caller's and up to three the student
                                   owns, created with the student; one fork and one join per call), each frame computed exactly as in a batch of the
                                   part's size.  0 never; 1 (default) a fixed function of the batch size (from 8 frames on two parts, three at 12, 24 and
                                   48 frames: 1-8 % at 512x1024, tools/sweep_parts.py) — nothing is timed, the call never
                                   synchronises; n >= 2 always AMS_OPT_DUAL_PARTS parts from n frames on (the caller decides). */,
       AMS_OPT_BLOCK_X6 = 8 /* whole-block kernels: 1 (default) the expand products of the blocks with 24 / 32 input channels, and the stem's
                               products in the one-kernel first block (operands from a 258-entry table of the normalised byte values), run as six bf16
                               MFMAs on three-part splits (f32-level, 96 instead of 256 matrix-pipe cycles per 16x16 tile); 0 exact f32 MFMA
                               (bit-identical to the layer-by-layer plan).  Always exact f32 under AMS_MATMUL_F32. */,
       AMS_OPT_LATE_SUBBATCH = 7 /* frozen inference: frames per pass of the output-stride-16 section (blocks 7-16 and the head); 0 = the whole
                                    batch.  Same results bit for bit; a pass whose largest tensor fits the 256 MB Infinity Cache keeps the
                                    writer / reader pairs of that section out of HBM */,
       AMS_OPT_FUSE_BLOCK = 6 /* frozen inference: 1 (default) every early inverted-residual block with Cin <= 32 (expand + depthwise +
                                 project [+ block input]) runs as ONE kernel: neither the 6x-expanded tensor nor the depthwise result reaches
                                 HBM; bit-identical to the layer-by-layer plan.  0: the per-layer / pairwise-fused kernels below */,
       AMS_OPT_FUSE_FIRST_BLOCK = 4 /* frozen inference, stem + depthwise + project of the first block: 0 three kernels, 1 one kernel
                                       with a tile per block (default), 2 one kernel with a tile per wave (measured slower); same bits */,
       AMS_OPT_FUSE_DW_PROJECT = 3 /* frozen inference: 1 = depthwise + project of the stride-16 blocks in one kernel (needs
                                      AMS_MATMUL_SPLIT_BF16), 0 (default) separate kernels: measured no faster */,
       AMS_OPT_FUSE_EXPAND_DW_STREAM = 5 /* frozen inference, split-bf16 modes: expand + depthwise of the stride-16 blocks in one
                                            streaming kernel, bit-identical to the two kernels it replaces: 0 never, 1
                                            (default) where measured faster (Cin 64 / 96, batches of >= 16384 pixels at
                                            that stride), 2 every supported block (Cin 160 too) */,
       AMS_OPT_MATMUL = 1, AMS_OPT_FUSE_EXPAND_DW = 2 /* 0 never, 1 (default) blocks where the fused kernel is faster, 2 every supported block */ };
enum { AMS_MATMUL_F32 = 0, AMS_MATMUL_SPLIT_BF16 = 1, AMS_MATMUL_SPLIT_BF16_X6 = 2,
       AMS_MATMUL_SPLIT_F16 = 4 /* frozen inference: every operand of those layers as TWO fp16 parts, x ~ hi + lo 2^-11 (22 significand bits),
                                   products hi hi + 2^-11 (hi lo + lo hi) on v_mfma_f32_16x16x32_f16 with the cross terms in an accumulator of
                                   their own: 3 MFMAs per 32 k instead of 6, and 4 bytes per value where parts are stored instead of 6 — the
                                   depthwise result of the stride-16 blocks is handed to the project GEMM as ready-made fp16 pairs at the bytes of
                                   f32.  Per product ~3 2^-22 against 2^-24: below the f32 accumulation error of these contractions (512x1024
                                   logits 4e-5 from the f64 oracle, as the three-part form).  Operands must lie within fp16's range (|x| <= 65504, and
                                   2^-14 or more for 22 bits: activations and weights of O(1); a layer's weights outside it move that layer to
                                   three bf16 parts at freeze, see ams_student_f16_fallback_layers); the fine-tune step keeps the three-part bf16 form (its gradients span a range
                                   fp16 cannot hold). */,
       AMS_MATMUL_BF16 = 3 /* opt-in bf16 inference variant (BASELINE.json configs[1] says "bf16"): the same late layers with ONE bf16 part per
                              operand = plain bf16 products, f32 accumulate, 1 MFMA per 32 k.  Storage stays f32 and the early blocks stay
                              exact f32.  NOT within the f32 tolerance: bench.py reports its label-mismatch fraction and mIoU delta against
                              the default plan beside its speed; frozen inference only (the fine-tune step ignores it). */ };
int ams_student_set_option(ams_student* s, int32_t option, int32_t value);

/* ---- measurement hook (bench.py roofline leg) -----------------------------------------------------------
 * With profiling enabled every kernel launch of the engine is bracketed by HIP events on the launch stream.
 * ams_student_profile_read synchronises and writes one line per launch: "kernel\tlayer\tms\talgorithmic_bytes\talgorithmic_flops\n"
 * (flops = 0 where the launch is priced by bytes only)
 * (kernel named as rocprofv3 prints it, without namespace and argument list).  `needed` receives the size. */
int ams_student_profile(ams_student* s, int32_t enable);
int ams_student_profile_read(ams_student* s, char* buf, size_t cap, size_t* needed);

/* Adam step counter (t of SURVEY.md Appendix C.10); exposed so host-side checkpoints can carry it. */
int ams_student_get_adam_step(const ams_student* s, int64_t* t);
int ams_student_set_adam_step(ams_student* s, int64_t t);

/* ---- model delta for the downlink: replaces the host loop of run.py:316-336 ------------------------------
 * Casts the masked parameters to fp16 in trainable order: out_half_dev receives sum(mask) halves, and
 * n_out_dev (int64) the count.  mask_dev NULL = all parameters. */
int ams_pack_masked_fp16(const float* params_dev, const uint8_t* mask_dev, int64_t n, uint16_t* out_half_dev,
                         int64_t* n_out_dev, int64_t* scratch_dev, size_t scratch_elems, void* stream);
/* int64 elements of caller-owned device scratch the call above needs (segment counts; nothing is allocated inside) */
size_t ams_pack_masked_fp16_scratch(int64_t n);

/* ---- the same delta applied on the edge: replaces reading the payload of run.py:316-328 and the model reload of run.py:401-411 -----------
 * One descriptor per variable of the payload's layout, in layout order: where its elements live (AMS_REGION_PARAMS or AMS_REGION_STATS,
 * element offset, element count) and where its packed mask bits start in the payload.  Masks are contiguous: mask_offset of the first
 * variable is 0 and each next one starts ceil(count / 8) bytes later; their sum is the mask section, the fp16 values follow it. */
typedef struct ams_delta_var {
    int32_t region;          /* AMS_REGION_PARAMS or AMS_REGION_STATS */
    int32_t reserved;        /* 0 */
    int64_t offset;          /* first element inside the region */
    int64_t count;           /* elements */
    int64_t mask_offset;     /* byte offset of the variable's mask bits in the payload */
} ams_delta_var;

#define AMS_DELTA_MAX_VARS 1024

/* status word written by ams_student_apply_delta, ams_student_apply_delta_q8 and ams_student_encode_delta_q8 */
enum {
    AMS_DELTA_OK = 0,
    AMS_DELTA_BAD_SIZE = 1,      /* payload bytes != mask bytes + 2 x set mask bits (truncated, over-long or a corrupted mask) */
    AMS_DELTA_BAD_PADDING = 2,   /* a padding bit after a variable's last element is set */
    AMS_DELTA_BAD_SCALE = 3,     /* q8 payload: a variable's scale is NaN, inf, negative, or nonzero below 2^-126 */
    AMS_DELTA_Q8_NONFINITE = 4   /* q8 encoder: a masked change (current - base) is NaN or +-inf; nothing was written */
};

/* Decodes payload_dev (payload_bytes device bytes, any alignment) into the student's unfolded variables: every masked element gets
 * float(its fp16 value), bit-exactly; every other element keeps its bits.  The payload is validated on the device first and a payload that
 * fails writes nothing: *status_dev (int32) = AMS_DELTA_*, *n_applied_dev (int64) = values written (0 unless AMS_DELTA_OK).  Neither is
 * read back here: the caller reads them once the stream has run.  The frozen snapshot is not touched: ams_student_freeze re-freezes.
 * vars_host (n_vars <= AMS_DELTA_MAX_VARS) is checked against the arena on the host; scratch_dev holds
 * ams_student_apply_delta_scratch(vars_host, n_vars) int64.  Three launches on `stream` (delta_count_kernel, delta_scan_kernel,
 * delta_apply_kernel) after a copy of the table; no allocation, no synchronisation. */
int ams_student_apply_delta(ams_student* s, const uint8_t* payload_dev, int64_t payload_bytes, const ams_delta_var* vars_host,
                            int32_t n_vars, int64_t* n_applied_dev, int32_t* status_dev, int64_t* scratch_dev, size_t scratch_elems,
                            void* stream);
/* int64 elements of device scratch ams_student_apply_delta needs for this table (0 if the table is malformed) */
size_t ams_student_apply_delta_scratch(const ams_delta_var* vars_host, int32_t n_vars);

/* ---- the server half of a model update: coordinates chosen by how far the first step moved them, the others rolled back, and the
 * delta encoded, all on the device.  Every result equals the host code it replaces bit for bit. --------------------------------------------
 *
 * The order statistics np.percentile interpolates between (replaces SemanticNetwork.py:267-271: the model fetched twice, 164
 * abs(after - before) arrays concatenated and partitioned).  change[i] = fabsf(after[i] - before[i]); *result_dev receives a = the change
 * of rank k (0-based, ascending), b = the change of rank k + 1 (a again when k + 1 == n) and the number of NaN changes (which sort last, as
 * in np.sort).  The threshold itself is formed on the host from these 16 bytes with NumPy's arithmetic (ams_amd/coord_masks.py:
 * percentile_rank, percentile_cut).  0 <= k < n < 2^31; result_dev 8-byte aligned; after / before any float alignment.  A memset and eight
 * launches on `stream` (three histogram + scan passes of a radix select, select_tail_kernel, select_finish_kernel); no allocation, no
 * synchronisation; scratch_dev holds ams_select_changed_scratch(n) int64. */
typedef struct ams_select_result {
    float a;
    float b;
    int64_t nan_count;
} ams_select_result;
int ams_select_changed(const float* after_dev, const float* before_dev, int64_t n, int64_t k, ams_select_result* result_dev,
                       int64_t* scratch_dev, size_t scratch_elems, void* stream);
size_t ams_select_changed_scratch(int64_t n);

/* The mask and the roll-back (replaces SemanticNetwork.py:276-287): mask_dev[i] = fabsf(params[i] - before[i]) > cut as uint8 0 / 1,
 * params_dev[i] keeps its value where the mask is set and becomes before_dev[i] elsewhere, *n_kept_dev (int64) = set mask entries.
 * cut = NaN keeps nothing and rolls everything back (np.percentile's answer when a change is NaN).  Adam moments and BN statistics are not
 * part of it.  One launch after a memset of the count; 16 bytes per lane when params / before are 16-byte and mask_dev 4-byte aligned. */
int ams_select_apply(float* params_dev, const float* before_dev, int64_t n, float cut, uint8_t* mask_dev, int64_t* n_kept_dev, void* stream);

/* The downlink delta written on the device (replaces the host loop of run.py:316-336; the inverse of ams_student_apply_delta, over the
 * same descriptor table): payload_dev receives, per variable, np.packbits of its mask, then the masked elements of every variable as
 * little-endian fp16 (round to nearest even, +-inf beyond 65504, as ams_pack_masked_fp16), read from the student's params / stats.
 * mask_dev: uint8 0 / non-0 per element in layout order (for the trainable layout: arena order), NULL = every element.
 * *payload_bytes_dev (int64) = the payload's size.  If that exceeds payload_cap nothing is written to payload_dev at all and the caller,
 * who reads the word once the stream has run, sees payload_bytes > payload_cap.  payload_cap below the mask section is refused at once.
 * Three launches (encode_kernel<false>, encode_scan_kernel, encode_kernel<true>) after a copy of the table; no allocation, no
 * synchronisation; scratch_dev holds ams_student_encode_delta_scratch(vars_host, n_vars) int64. */
int ams_student_encode_delta(ams_student* s, const uint8_t* mask_dev, const ams_delta_var* vars_host, int32_t n_vars, uint8_t* payload_dev,
                             int64_t payload_cap, int64_t* payload_bytes_dev, int64_t* scratch_dev, size_t scratch_elems, void* stream);
/* int64 elements of device scratch ams_student_encode_delta needs for this table (0 if the table is malformed) */
size_t ams_student_encode_delta_scratch(const ams_delta_var* vars_host, int32_t n_vars);

/* ---- the same delta in 8 bits (q8): both ends hold the model the update starts from, so the change travels, not the value --------------
 * Payload, over the same descriptor table, no header and no padding between sections:
 *   [mask section]   as above: per variable np.packbits(mask)
 *   [scale section]  n_vars little-endian f32, one per variable of the layout in layout order (unaligned: read and written as bytes)
 *   [code section]   one int8 per set mask bit, in mask order
 * so payload bytes = mask bytes + 4 x n_vars + set bits.
 *
 * Encoder, all f32, one rounding per operation: d = current - base; amax_v = max |d| over the masked elements of variable v (0 if none);
 * scale_v = amax_v / 127, set to 0 if below 2^-126; q = 0 if scale_v == 0, else clamp(rintf(d / scale_v), -127, 127) (ties to even).
 * The student's params / stats are the current values; base_params_dev / base_stats_dev hold the base in the same element order
 * (n_trainable / n_stats floats; base_stats_dev may be NULL only if no table entry lies in AMS_REGION_STATS).  mask_dev as above.
 * *status_dev (int32) = AMS_DELTA_OK, or AMS_DELTA_Q8_NONFINITE if a masked d is NaN or +-inf: then *payload_bytes_dev = 0 and neither
 * the payload nor the base is written.  Otherwise *payload_bytes_dev (int64) = the payload's size; beyond payload_cap nothing is written
 * either and the caller sees payload_bytes > payload_cap.  advance_base = 1: the write pass also stores f32(base + f32(scale_v * q)) —
 * what the decoder makes of the element — into the base of every masked element, so that the next payload is relative to the model the
 * edge really holds (continual training); 0 leaves the base alone.
 * Refused on the host with AMS_E_INVALID and nothing launched: a null pointer, advance_base outside 0 / 1, a malformed table, scratch
 * below ams_student_encode_delta_q8_scratch, payload_cap below mask section + scale section.
 * Three launches (q8_amax_kernel, q8_encode_scan_kernel, q8_encode_write_kernel) after a copy of the table, which also zeroes the
 * per-variable maxima; no allocation, no synchronisation. */
int ams_student_encode_delta_q8(ams_student* s, const uint8_t* mask_dev, const ams_delta_var* vars_host, int32_t n_vars,
                                float* base_params_dev, float* base_stats_dev, int32_t advance_base, uint8_t* payload_dev,
                                int64_t payload_cap, int64_t* payload_bytes_dev, int32_t* status_dev, int64_t* scratch_dev,
                                size_t scratch_elems, void* stream);
/* int64 elements of device scratch ams_student_encode_delta_q8 needs for this table (0 if the table is malformed) */
size_t ams_student_encode_delta_q8_scratch(const ams_delta_var* vars_host, int32_t n_vars);

/* Decodes a q8 payload in place: every masked element becomes f32(element + f32(scale_v * q)), two roundings (the element's current
 * value is the base: load the base first); every other element keeps its bits; a code of -128 (never produced) decodes as -128.
 * Validated on the device first, all or nothing: size (AMS_DELTA_BAD_SIZE), padding bits (AMS_DELTA_BAD_PADDING), then the scales
 * (AMS_DELTA_BAD_SCALE).  *status_dev / *n_applied_dev, the table and the scratch as for ams_student_apply_delta.  Three launches
 * (delta_count_kernel, q8_delta_scan_kernel, q8_delta_apply_kernel) after a copy of the table; no allocation, no synchronisation. */
int ams_student_apply_delta_q8(ams_student* s, const uint8_t* payload_dev, int64_t payload_bytes, const ams_delta_var* vars_host,
                               int32_t n_vars, int64_t* n_applied_dev, int32_t* status_dev, int64_t* scratch_dev, size_t scratch_elems,
                               void* stream);
/* int64 elements of device scratch ams_student_apply_delta_q8 needs for this table (0 if the table is malformed) */
size_t ams_student_apply_delta_q8_scratch(const ams_delta_var* vars_host, int32_t n_vars);

/* ---- the uplink frame codec (k_uplink.hip; run.py --compress_uplink): an intra-frame transform codec of the project's own, format AUC1.
 * It stands for the reference's H.264 leg (lossy frames at a byte budget, counted bytes); its byte counts are NOT H.264's.  All arithmetic
 * is integer (>> is an arithmetic shift), so tests/uplink_ref.py restates both ends byte for byte.
 *
 * Frame: RGB uint8 [H, W, 3], H and W multiples of 16 in 16 .. 4096.
 * Colour, JFIF full range in 16-bit fixed point, every result clamped to 0 .. 255:
 *   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16;  Cb = ((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128;
 *   Cr = ((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128;  chroma 4:2:0: (a + b + c + d + 2) >> 2 over each 2 x 2.
 *   Back, chroma replicated 2 x 2: R = Y + ((91881 (Cr - 128) + 32768) >> 16);  B = Y + ((116130 (Cb - 128) + 32768) >> 16);
 *   G = Y - ((22554 (Cb - 128) + 46802 (Cr - 128) + 32768) >> 16).
 * Transform: 8 x 8 blocks of pixel - 128; M = rint(2^13 C), C the orthonormal 8-point DCT-II matrix.  Forward: along the rows
 *   t = (M x + 512) >> 10, then along the columns c = (M t + 32768) >> 16.  Inverse: the same two shifts with M transposed, columns
 *   first, then + 128 and the clamp; the decoder clamps every dequantised coefficient to [-2047, 2047] first.
 * Quantisation: the JPEG Annex K luminance / chrominance tables with libjpeg's quality scaling, q in 1 .. 100: s = q < 50 ? 5000 / q :
 *   200 - 2 q;  qt = clamp((base s + 50) / 100, 1, 255);  level = sign(c) ((|c| + qt / 2) / qt);  dequantised level x qt.
 * Entropy code: Exp-Golomb of order 0, bits MSB first: ue(v) = floor(log2(v + 1)) zero bits, then v + 1 in binary; se(v) = ue(v > 0 ?
 *   2 v - 1 : -2 v).  A block in JPEG zig-zag order: se(dc - pred); per non-zero AC ue(run + 1), se(level), run = the zeros since the
 *   previous coded coefficient; ue(0) ends every block.
 * Slices: planes in the order Y, Cb, Cr, blocks in raster order within a plane; every 32 consecutive blocks of a plane are a slice (a
 *   plane's last may be shorter); pred = the previous block's quantised DC within the slice, 0 for its first; zero bits pad a slice to a byte.
 * Payload, little-endian, no alignment assumed: 16-byte header "AUC1", u16 H, u16 W, u8 q, three zero bytes, u32 total payload bytes;
 *   one u16 byte length per slice; the slices. */
enum {
    AMS_UPLINK_OK = 0,
    AMS_UPLINK_BAD_HEADER = 1,      /* magic, H or W (against the call's), q, the reserved bytes or the total (against the bytes handed in) */
    AMS_UPLINK_BAD_TABLE = 2,       /* header + table + the table's lengths != the total */
    AMS_UPLINK_BAD_SLICE_END = 3,   /* a slice's last block ends before the slice's last byte, or a padding bit is set */
    AMS_UPLINK_BAD_POSITION = 4,    /* a run leads past coefficient 63 */
    AMS_UPLINK_BAD_ZERO_LEVEL = 5,  /* an AC level of 0 */
    AMS_UPLINK_BAD_LEVEL = 6,       /* |level| > 2047 (an Exp-Golomb prefix of more than 16 zero bits counts as one) */
    AMS_UPLINK_BAD_OVERRUN = 7,     /* a code runs past the end of its slice */
    AMS_UPLINK_NO_ROOM = 8,         /* encoder: the payload is larger than payload_cap; nothing was written */
    AMS_UPLINK_BAD_VECTOR = 9,      /* AUP1: a vector component beyond +-15, or a 16 x 16 luma window that leaves the frame */
    AMS_UPLINK_BAD_ZERO_SLICE = 10  /* AUP1: a slice of nothing but zero levels (a motion slice: zero vectors) sent with bytes */
};
/* Every ams_uplink_* entry refuses on the host, AMS_E_INVALID and nothing launched, in this order: H or W <= 0; H or W no multiple of 16
 * in 16 .. 4096 (the encoder: or q outside 1 .. 100); scratch NULL or below the entry's _scratch bytes; a null pointer; scratch
 * not 16-byte aligned; a negative payload_cap / payload_bytes.  No handle, no allocation, no synchronisation. */
/* the largest payload of an H x W frame: header + table + 208 bytes per block; 0 for a size the entries refuse */
int64_t ams_uplink_max_bytes(int32_t H, int32_t W);
/* BYTES of device scratch of the encoder entries (transform, size_table, encode share one block) and of the decoder; 0 for a refused size */
size_t ams_uplink_encode_scratch(int32_t H, int32_t W);
size_t ams_uplink_decode_scratch(int32_t H, int32_t W);
/* Colour, 4:2:0 and the forward transform of frame_dev: int16 coefficients, zig-zag order per block, into the scratch (one launch). */
int ams_uplink_transform(const uint8_t* frame_dev, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes, void* stream);
/* From the coefficients ams_uplink_transform left in the scratch: sizes_dev[q - 1] (int64 x 100) = the exact payload bytes at quality q
 * (two launches: per (quality, slice) byte counts, then the 100 totals). */
int ams_uplink_size_table(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int64_t* sizes_dev, void* stream);
/* Writes the payload at quality q from the coefficients in the scratch.  *bytes_dev (int64) = the payload's size; *status_dev (int32) =
 * AMS_UPLINK_OK, or AMS_UPLINK_NO_ROOM if that size exceeds payload_cap: then no byte of payload_dev is written.  Three launches: slice
 * lengths, their scan with header and table, the slices' bits. */
int ams_uplink_encode(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int32_t q, uint8_t* payload_dev, int64_t payload_cap,
                      int64_t* bytes_dev, int32_t* status_dev, void* stream);
/* Decodes payload_dev[0, payload_bytes) to RGB uint8 [H, W, 3].  Validated on the device, all or nothing: *status_dev (int32) = AMS_UPLINK_*
 * (several malformed slices: the largest of their codes), and frame_out_dev is written only under AMS_UPLINK_OK.  No byte outside
 * [0, payload_bytes) is read.  Three launches: header, table and scan; one slice per thread into int16 levels; reconstruction. */
int ams_uplink_decode(const uint8_t* payload_dev, int64_t payload_bytes, int32_t H, int32_t W, uint8_t* frame_out_dev, int32_t* status_dev,
                      void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- the predicted frame of the uplink codec (k_uplink_inter.hip; run.py --uplink_gop), format AUP1: a frame coded as a prediction from a
 * reference frame plus a residual.  Everything not stated here is AUC1's, above; tests/uplink_inter_ref.py restates both ends byte for byte.
 *
 * Reference: RGB uint8 [H, W, 3] of the frame's size, what the decoder produced for the previous frame (closed loop).  Both ends take it to
 *   Y and 4:2:0 Cb, Cr with the AUC1 colour equations.
 * Motion: one vector (dy, dx) per 16 x 16 macroblock (my, mx), full luma pels, each component in -15 .. 15.  Legal are the vectors whose
 *   luma window lies in the frame: 0 <= y0 = 16 my + dy <= H - 16 and 0 <= x0 = 16 mx + dx <= W - 16.  Luma prediction: that window.
 *   Chroma prediction: the 8 x 8 window of the reference's chroma plane at (8 my + (dy >> 1), 8 mx + (dx >> 1)) = (y0 >> 1, x0 >> 1); an odd
 *   component averages each sample with its successor along that axis, (a + b + 1) >> 1; two odd components average the four,
 *   (a + b + c + d + 2) >> 2.
 *   Those reads stay in the plane for every legal luma vector: along y (x alike) the first row read is y0 >> 1 >= 0.  For an even y0 the
 *   last is y0 / 2 + 7 <= (H - 16) / 2 + 7 = H / 2 - 1.  For an odd y0 it is (y0 - 1) / 2 + 8, and H - 16 is even, so y0 <= H - 17 and
 *   the row is at most (H - 18) / 2 + 8 = H / 2 - 1.
 * Residual: current - prediction per 8 x 8 block, without the - 128, through the AUC1 forward transform, tables, quality scale, level rule,
 *   zig-zag and block code, DC prediction within a slice included.  |coefficient| <= 2047 holds for residuals in +-255: with A = the largest
 *   row sum of |C| = 8 / sqrt(8) (row 0 and row 4; the others are smaller), the real coefficient is at most 255 A^2 = 2040, and the two
 *   rounded passes add less than FWD_BOUND's terms at twice the range: 1/2 + A e_t / 8 + R1 (2048 A + e_t) / 65536 with e_t = 1/2 + 255 R1 /
 *   1024, about 1.1 (tests/test_uplink_inter_ref_cpu.py computes it and runs the extremes).  So the level rule's numerator stays below 4096
 *   and the coefficients fit int16.  The decoder adds the inverse transform, without the + 128, to the prediction and clamps to 0 .. 255.
 * Slices: the motion slices come first, each 32 consecutive raster macroblocks (the last may be shorter): per macroblock se(dy - pdy)
 *   se(dx - pdx) against the previous macroblock's vector in the slice, (0, 0) for its first, zero bits to a whole byte.  The Y, Cb, Cr
 *   residual slices follow as AUC1 cuts them.  A table length of 0 means: every level of the slice is zero (a motion slice: every vector),
 *   and no byte follows.  A slice of that content MUST be written so: the long form is refused, one frame has one payload.
 * Payload: "AUP1", u16 H, u16 W, u8 q, three zero bytes, u32 total payload bytes; one u16 byte length per slice; the slices.
 * Each decoder refuses the other kind's payload with AMS_UPLINK_BAD_HEADER.
 *
 * The encoder's choices (not the format's: the decoder takes any legal vector): an exhaustive search over the legal vectors for the least
 *   SAD_luma + 128 [vector != 0]; ties go to the smaller |dy| + |dx|, then the smaller dy, then the smaller dx.
 *
 * The entries refuse on the host as the ams_uplink_* entries above do, in the same order; ref_dev is one of the pointers. */
/* the largest payload: header + table + 208 bytes per block + 3 bytes per macroblock; 0 for a size the entries refuse */
int64_t ams_uplink_inter_max_bytes(int32_t H, int32_t W);
/* BYTES of device scratch of the encoder entries (transform, size_table, encode share one block) and of the decoder; 0 for a refused size */
size_t ams_uplink_inter_encode_scratch(int32_t H, int32_t W);
size_t ams_uplink_inter_decode_scratch(int32_t H, int32_t W);
/* The motion search of frame_dev in ref_dev, then prediction and the residual's forward transform: vectors and int16 coefficients, zig-zag
 * order per block, into the scratch (two launches). */
int ams_uplink_inter_transform(const uint8_t* frame_dev, const uint8_t* ref_dev, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes,
                               void* stream);
/* From what ams_uplink_inter_transform left in the scratch: sizes_dev[q - 1] (int64 x 100) = the exact AUP1 payload bytes at quality q; the
 * (quality, slice) count of an all-zero slice is 0 (two launches). */
int ams_uplink_inter_size_table(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int64_t* sizes_dev, void* stream);
/* Writes the AUP1 payload at quality q from the scratch; *bytes_dev, *status_dev and payload_cap as in ams_uplink_encode (three launches). */
int ams_uplink_inter_encode(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int32_t q, uint8_t* payload_dev, int64_t payload_cap,
                            int64_t* bytes_dev, int32_t* status_dev, void* stream);
/* Decodes an AUP1 payload against ref_dev (RGB uint8 [H, W, 3]) to RGB uint8 [H, W, 3].  Validated on the device, all or nothing, as
 * ams_uplink_decode: the largest status of the malformed slices stands, frame_out_dev is written only under AMS_UPLINK_OK, and no byte outside
 * the payload or the reference is read: the vectors are validated before the reconstruction reads through them (three launches). */
int ams_uplink_inter_decode(const uint8_t* payload_dev, int64_t payload_bytes, const uint8_t* ref_dev, int32_t H, int32_t W, uint8_t* frame_out_dev,
                            int32_t* status_dev, void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- the server's replay memory on the device (replaces run.py:136-137 frame_memory / label_memory, two host deques, and the sampling of
 * utils/utils.py:129-185 mini_batch from them).  The memory is a ring of `capacity` slots the caller owns: slot p of the frames is uint8
 * [src_h, src_w, 3] at frame_slots_dev + p * frame_slot_stride, of the labels uint8 [src_h, src_w] at label_slots_dev + p * label_slot_stride
 * (strides in bytes; multiples of 16 with 16-byte aligned bases and src_w, W multiples of 16 let the copy case move 16 bytes per lane).
 *
 * One descriptor per batch entry, drawn on the host with the host generators (ams_amd/replay.py: draw_samples): the entry is the crop
 * [top, top + H) x [left, left + W) of cv2.resize(frame, (tw, th)) [INTER_LINEAR, OpenCV's 8-bit fixed-point arithmetic as in
 * ams_ingest_resize_u8] and of cv2.resize(label, (tw, th), INTER_NEAREST), with the columns mirrored when flip != 0 (np.flip(axis=1)):
 * utils/utils.py:165-183, bit for bit, without forming the rescaled frame. */
typedef struct ams_replay_sample {
    int32_t slot;        /* physical slot in the ring */
    int32_t th, tw;      /* size of the rescaled image the crop is cut from: int(src_h*factor), int(src_w*factor) */
    int32_t top, left;   /* crop origin inside it */
    int32_t flip;        /* mirror the columns (np.flip(axis=1)) */
} ams_replay_sample;

/* A mini-batch in one launch (replaces utils/utils.py:129-185 and the pinned staging + upload of the batch): frames_out_dev uint8
 * [batch, H, W, 3], labels_out_dev uint8 [batch, H, W].  samples_dev is the table the kernel reads; samples_host is the same table on the
 * host, checked before the launch: a slot outside the capacity, negative slack (th < H or tw < W) or a crop outside (th, tw) is refused
 * with AMS_E_INVALID and nothing is launched.  One launch (replay_gather_kernel); no allocation, no synchronisation. */
int ams_replay_gather(const uint8_t* frame_slots_dev, int64_t frame_slot_stride, const uint8_t* label_slots_dev, int64_t label_slot_stride,
                      int32_t capacity, int32_t src_h, int32_t src_w, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host,
                      int32_t batch, int32_t H, int32_t W, uint8_t* frames_out_dev, uint8_t* labels_out_dev, void* stream);

/* The cached teacher logits of the frames a batch drew (replaces the np.stack + pin_memory + upload of the soft-teacher batch; the reference
 * feeds teacher_labels_logits_pl per batch, utils/graph_utils.py:359): slot p is f32 [th, tw, channels] at slots_dev + p * slot_stride
 * (stride in elements), out_dev f32 [batch, th, tw, channels].  Whole slots only: a descriptor with a crop origin or a flip is refused
 * (ams_replay_gather_logits rescales, crops and mirrors logits cached at the frame size, ams_replay_gather_logits_lowres logits cached on
 * a smaller grid).  One launch (replay_gather_rows_kernel); no allocation, no synchronisation. */
int ams_replay_gather_f32(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t th, int32_t tw, int32_t channels,
                          const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int32_t batch, float* out_dev, void* stream);

/* The teacher logits of a rescaled, cropped and mirrored batch: what the descriptors of ams_replay_gather do to a frame, done to the logits
 * cached for it AT THE FRAME SIZE.  Slot p is f32 [src_h, src_w, channels] at slots_dev + p * slot_stride (stride in elements); out_dev is
 * f32 [batch, H, W, channels], the label size, which ams_student_feed_teacher_logits(th = H, tw = W) reads as it is.
 *
 * The rule is this project's own (the reference's mini_batch never sees logits): the geometry of cv2.resize's float INTER_LINEAR, so that
 * the logits are resampled where their frame is.  Output (y, x) of a descriptor (slot, th, tw, top, left, flip) samples the rescaled
 * logits at cy = top + y, cx = left + (flip ? W - 1 - x : x).  Per axis (x shown), in double: f = (cx + 0.5) * ((double)src_w / (double)tw)
 * - 0.5, s = floor(f), w = (float)(f - s); s < 0 gives s = 0, w = 0; s >= src_w - 1 gives s = src_w - 1, w = 0; the second tap is
 * min(s + 1, src_w - 1).  Per channel, in f32, every operation rounded once (no fused multiply-add):
 *
 *     r0  = t[sy ][sx] * (1 - wx) + t[sy ][sx1] * wx
 *     r1  = t[sy1][sx] * (1 - wx) + t[sy1][sx1] * wx
 *     out = r0 * (1 - wy) + r1 * wy
 *
 * th == src_h && tw == src_w (per sample) is a plain copy of the crop window, mirrored when flip: an inf or NaN of a neighbouring pixel
 * does not enter.  An exact 2x down-scale lands on w = 0.5, the 2 x 2 mean.  Logits cached on a smaller grid than the frame are served by
 * ams_replay_gather_logits_lowres (this rule applied to their align-corners upsample); whole frames go through ams_replay_gather_f32.
 *
 * The descriptors are checked as by ams_replay_gather, on the host before the launch (AMS_E_INVALID, nothing launched) and again in the
 * kernel.  16-byte aligned bases, slot_stride, src_w * channels and W * channels multiples of 4 let the unmirrored copy case with
 * left * channels a multiple of 4 move 16 bytes per lane; with channels a multiple of 4 (slots in the selected layout, K = 4, 8, ...) that
 * holds for every left, and the mirrored copy moves 16 bytes per lane too.  One launch (replay_gather_logits_kernel); no allocation, no synchronisation. */
int ams_replay_gather_logits(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t src_h, int32_t src_w, int32_t channels,
                             const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int32_t batch, int32_t H, int32_t W,
                             float* out_dev, void* stream);

/* The same for teacher logits cached on a grid NO LARGER THAN THE FRAME (e.g. 33 x 65 for 512 x 1024 frames: what a teacher of output stride
 * 16 produces; 163 KB per slot at 19 classes instead of 40 MB).  Slot p is f32 [lh, lw, channels] at slots_dev + p * slot_stride, 1 <= lh <=
 * src_h, 1 <= lw <= src_w; channels is every class or the K selected ones; out_dev is f32 [batch, H, W, channels] as above.
 *
 * The rule: a low-resolution slot behaves, bit for bit, as a frame-size slot that holds its own align-corners upsample.  Two stages, both
 * already defined, evaluated in one kernel (the frame-size tensor U is never stored):
 *
 *   Stage U, the virtual logits f32 [src_h, src_w, channels], by the arithmetic of the soft loss kernel (what ams_student_feed_teacher_logits
 *   does to a teacher grid smaller than the labels): sy = src_h > 1 ? (float)(lh - 1) / (float)(src_h - 1) : 0, sx likewise, in f32.  Per axis
 *   (y shown), in f32: src = (float)Y * sy, lo = floor(src), hi = min(lo + 1, lh - 1), ty = src - floor(src).  On a grid point, ty == 0 &&
 *   tx == 0, U(Y, X, c) is the cached sample t[lo_y][lo_x][c] itself (the sign of a zero survives).  Otherwise, every operation rounded once:
 *
 *       top = tl + (tr - tl) * tx,  bot = bl + (br - bl) * tx,  U(Y, X, c) = top + (bot - top) * ty
 *
 *   with tl = t[lo_y][lo_x][c], tr = t[lo_y][hi_x][c], bl = t[hi_y][lo_x][c], br = t[hi_y][hi_x][c].
 *
 *   Stage G, the rule of ams_replay_gather_logits applied to U: cy = top + y, cx = left + (flip ? W - 1 - x : x); th == src_h && tw == src_w
 *   copies U's window; otherwise the taps in double per axis with their two clamps, r0 = U[sy][sx] * (1 - wx) + U[sy][sx1] * wx, r1 likewise
 *   on row sy1, out = r0 * (1 - wy) + r1 * wy in f32.
 *
 * lh == src_h && lw == src_w makes every point a grid point: the result is ams_replay_gather_logits' (that entry's copy case moves 16 bytes
 * per lane; prefer it there).  A whole-frame batch needs no gather at this size at all: ams_replay_gather_f32 copies the cached grids and the
 * loss kernel's own upsample gives the bits of U.  The contract is for finite logits: a non-finite cached value spreads to the pixels between
 * it and its neighbours through the interpolation, as it does in the loss kernel, and no bit pattern is promised for those.
 *
 * Checked on the host before the launch (AMS_E_INVALID, nothing launched, nothing written) and again in the kernel: the descriptors as by
 * ams_replay_gather_logits, 1 <= lh <= src_h, 1 <= lw <= src_w, slot_stride >= lh * lw * channels, no NULL pointer.  One launch
 * (replay_gather_logits_lowres_kernel); no allocation, no synchronisation. */
int ams_replay_gather_logits_lowres(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t lh, int32_t lw, int32_t channels,
                                    int32_t src_h, int32_t src_w, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host,
                                    int32_t batch, int32_t H, int32_t W, float* out_dev, void* stream);

/* A frame's teacher logits into a replay slot (the append of logits that are already on the device; the reference keeps what it feeds to
 * teacher_labels_logits_pl on the host, utils/graph_utils.py:359, and its loss reads the class_weights channels alone, :375-376):
 * logits_dev f32 [th, tw, num_classes] -> slot_dev.  AMS_TLOGITS_SELECTED writes f32 [th, tw, K], channel k = input channel
 * class_idx_host[k] (a HOST array, checked here, passed by value): copies, every bit pattern survives.  AMS_TLOGITS_FULL copies the input
 * as it is (class_idx_host and K are not read).  One launch (replay_pack_logits_kernel: a block stages a run of pixels of one row in LDS;
 * 16-byte loads when logits_dev is 16-byte aligned and tw * num_classes a multiple of 4, 16-byte stores when slot_dev is and tw * K is).
 * AMS_E_INVALID, nothing launched, nothing written: a layout other than the two, a NULL pointer, K outside 1..32, an index outside
 * 0..num_classes - 1, num_classes > 256, th > 65535. */
int ams_replay_pack_logits(const float* logits_dev, int32_t th, int32_t tw, int32_t num_classes, const int32_t* class_idx_host, int32_t K,
                           int32_t layout, float* slot_dev, void* stream);

/* The hard teacher labels of cached teacher logits (what a replay slot stores beside the logits; the reference's teacher derives its
 * `predictions` the same way, argmax of its bilinearly upsampled logits, utils/graph_utils.py:143-152, and extract_labels.py writes them to
 * gt_*.png): item i is f32 [lh, lw, num_classes] at logits_dev + i * slot_stride (stride in elements), the FULL layout, 1 <= lh <= Hs,
 * 1 <= lw <= Ws; labels_out_dev + i * out_stride (stride in bytes) receives uint8 [Hs, Ws] of class ids 0 .. num_classes - 1:
 *
 *     label(Y, X) = argmax_c U(Y, X, c)
 *
 * U is Stage U of ams_replay_gather_logits_lowres above, bit for bit (sy = Hs > 1 ? (float)(lh - 1) / (float)(Hs - 1) : 0, the f32 taps, the
 * cached sample itself on a grid point, every f32 operation rounded once), over all num_classes channels; lh == Hs && lw == Ws makes every
 * position a grid point.  The argmax is tf.argmax's: the first maximum wins (a strict > scan from class 0), so a tie takes the lowest index,
 * and -0.0 and +0.0 tie.  The contract is for finite logits, as for Stage U: no label is promised at a pixel whose interpolation a NaN or an
 * infinity enters.  Bytes past Hs * Ws of an item's out_stride are not written.
 *
 * Checked on the host before the launch (AMS_E_INVALID, nothing launched, nothing written) and again in the kernel: no NULL pointer,
 * 1 <= n <= 65535, Hs <= 65535, 1 <= lh <= Hs, 1 <= lw <= Ws, 1 <= num_classes <= 255 (id 255 stays "unlabelled"), slot_stride >= lh * lw *
 * num_classes, out_stride >= Hs * Ws.  One launch (teacher_labels_kernel: a block stages the cached columns under a segment of an output row
 * in LDS, each lane scans the classes of one pixel; labels_out_dev and out_stride multiples of 4 with Ws a multiple of 4 make the stores
 * 4 bytes wide); no allocation, no synchronisation. */
int ams_teacher_labels_from_logits(const float* logits_dev, int64_t slot_stride, int32_t n, int32_t lh, int32_t lw, int32_t num_classes, int32_t Hs,
                                   int32_t Ws, uint8_t* labels_out_dev, int64_t out_stride, void* stream);

/* The phi-score confusion matrices of n_pairs pairs of label slots at once (replaces the loop of run.py:287-291 over calc_cross_miou,
 * SemanticNetwork.py:124-139: one upload and one synchronising read per pair): pair i is (pairs[2i], pairs[2i + 1]) = (before, after)
 * physical slots, conf_mats_dev int64 [n_pairs][K][K] overwritten with the integers ams_cross_confusion gives pair by pair.  pairs_host
 * is checked against the capacity before the launch.  A memset and one launch (cross_confusion_pairs_kernel); no allocation, no
 * synchronisation. */
int ams_cross_confusion_pairs(const ams_student* s, const uint8_t* label_slots_dev, int64_t label_slot_stride, int32_t capacity, int64_t n_pixels,
                              const int32_t* pairs_dev, const int32_t* pairs_host, int32_t n_pairs, int64_t* conf_mats_dev, void* stream);

/* ---- the edge's pictures on the device (replaces the NumPy bodies of SemanticNetwork.py:719-755 colorize / colorize_teacher / cross_ignore
 * for callers whose frame and labels are on the device already, and feeds run.py:441-454 --save_pic).  Six RGB uint8 views [batch, H, W, 3]:
 *
 *   colour_student    reduced palette [student]                     (student: index into the K-class subset)
 *   overlay_student   the 50/50 blend of the frame and colour_student
 *   colour_teacher    full palette [teacher]                        (teacher: dataset class id; all 256 rows exist, rows >= 19 are black)
 *   overlay_teacher   the 50/50 blend of the frame and colour_teacher
 *   ignore_mask       white where take[teacher] == 0, black elsewhere (as in the reference, subset index 0 doubles as "ignored")
 *   cross_mask        reduced palette [take[teacher]] where not ignored and take[teacher] != student, black elsewhere
 *
 * The blend is integer: t = f + c; h = t >> 1; h += (t & 1) & (h & 1) (half to even, what cv2.addWeighted gives on the float sum).
 *
 * The table block (AMS_RENDER_TABLE_BYTES bytes on the device; ams_amd/render.py: build_tables makes it once per network): the full palette
 * uint8 [256][3], the reduced palette uint8 [32][3] (rows from K on zero), the take table uint8 [256] (teacher id -> subset index, zero for
 * an id outside the subset and from the dataset's class count on).
 *
 * Labels out of range give defined output: a student label outside [0, K) paints black; a teacher id from the dataset's class count on counts
 * as ignored (white in ignore_mask, black in cross_mask, black in colour_teacher), where the host helper raises IndexError.  The metric of
 * ams_student_predict_with_metric ignores such an id as well (its class table maps every id outside the subset to "ignored"). */
#define AMS_RENDER_TABLE_BYTES 1120

typedef struct ams_render_out {          /* device pointers, uint8 [batch, H, W, 3]; NULL = the view is not wanted and costs nothing */
    uint8_t* colour_student;
    uint8_t* overlay_student;
    uint8_t* colour_teacher;
    uint8_t* overlay_teacher;
    uint8_t* ignore_mask;
    uint8_t* cross_mask;
} ams_render_out;

/* AMS_RENDER_TABLE_BYTES of the library that is loaded */
size_t ams_render_table_bytes(void);

/* frames_dev uint8 [batch, H, W, 3]; student_dev uint8 or int32 [batch, H, W] (student_dtype AMS_DT_U8 / AMS_DT_I32); teacher_dev uint8
 * [batch, H, W].  An input that no requested view reads may be NULL.  Stateless; one launch (render_views_kernel), no allocation, no
 * synchronisation.  With W a multiple of 16 and every pointer 16-byte aligned a lane moves 16 pixels with 16-byte accesses.
 * Refused with AMS_E_INVALID before anything is launched (no output is touched): batch, H or W <= 0 (or batch, H above 65535), K outside
 * [1, 32], another student_dtype, tables_dev NULL, no view requested, a requested view whose input is NULL. */
int ams_render_views(const uint8_t* frames_dev, const void* student_dev, int32_t student_dtype, const uint8_t* teacher_dev, int32_t batch, int32_t H,
                     int32_t W, int32_t K, const uint8_t* tables_dev, const ams_render_out* out, void* stream);

/* =====================================================================================================
 * Kernel-level entry points.  Same kernels the engine launches, exposed one by one so that tests/ can
 * check each against the oracle (SURVEY.md §4 test pyramid level 1).  x/y/... are device pointers.
 * ===================================================================================================== */

/* The entries of the GEMM family (ams_k_pointwise, _split, _split3, _split_f16, _wgrad, _wgrad_split, _red, _xform, _wgrad_xform,
 * ams_k_pack_h2i), of the depthwise and stem family (ams_k_depthwise3x3, _dgrad, _wgrad, _fwd_bn, _dgrad_bn, _fwd_bn_tiles, _dgrad_bn_apply,
 * ams_k_stem_conv) and of the recompute family (ams_k_xdw_fwd_stats, _bwd_reduce, _bwd_dx, _bwd_reduce_stem, _dwe, ams_k_xx_gram,
 * ams_k_expand_stats) refuse with AMS_E_INVALID, in this order and in front of their first launch (a weight split is a launch); the message
 * starts with the entry's name without its prefix ("depthwise3x3_wgrad: ..."):
 *   1. no pixels or rows — B, H, W, M, K, N, C, Cin, Cexp, cout or n <= 0                                  "empty problem"
 *   2. the entry's shape rule, stated as "Accepts:" at its prototype                                        "unsupported shape"
 *   3. scratch or panels NULL, or fewer elements than the entry states                                      "too small (need N)"
 *   4. scale without shift                                                                                  "scale without shift"
 *   5. NULL among the pointers the entry reads or writes ("Reads:"; what is not listed may be NULL)         "null pointer"
 * The *_scratch() functions of these entries return 0 for sizes <= 0 and for a shape their entry refuses at 1 or 2.  The launchers behind the
 * entries keep their own conditions (alignment, grid and LDS limits), which follow. */

/* K1+K2: pad(127.5) -> x/127.5-1 -> dense 3x3 stride 2 SAME (3 -> cout) -> y*scale+shift -> act.
 * scale/shift NULL: raw conv output.
 * Accepts: B, H, W, cout > 0; cout % 8 == 0 and <= 256, frames_dtype AMS_DT_U8 | AMS_DT_F32 (cout == 32 runs the MFMA form, every other width the
 * generic kernel).  Reads: frames, w, y. */
int ams_k_stem_conv(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, const float* w /*[3,3,3,cout]*/,
                    int32_t cout, const float* scale, const float* shift, int32_t act, float pixel_scale,
                    float* y /*[B,Ho,Wo,cout]*/, void* stream);

/* K3: depthwise 3x3, NHWC, SAME, stride 1|2, rate 1|2 -> y*scale+shift -> act (scale NULL: raw).
 * Accepts (every ams_k_depthwise3x3* entry): B, H, W, C > 0; C % 4 == 0 and 4 <= C <= 1024; stride 1 | 2, rate 1 | 2, not both 2 (the four
 * one-kernel fine-tune forms have stride 1).  Reads: x, w, y. */
int ams_k_depthwise3x3(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* w /*[3,3,C,1]*/,
                       int32_t stride, int32_t rate, const float* scale, const float* shift, int32_t act,
                       float* y, void* stream);

/* K4: 1x1 conv as GEMM: y[M,N] = act((x[M,K] @ w[K,N] + img_bias[row/rows_per_img]) * scale + shift) + res.
 * Any of img_bias/scale/shift/res may be NULL.  trans_w != 0: w is given as [N,K] (dgrad).
 * M <= 16 runs a kernel of its own (one row per block row, k summed in another order than the tiled and streaming kernels): wherever an entry
 * below is called bit-identical to ams_k_pointwise, that holds for M > 16 rows; up to 16 rows the two agree to f32 rounding.
 * Accepts: M, K, N > 0; K % 4 == 0 (any N >= 1).  Reads: x, w, y. */
int ams_k_pointwise(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w,
                    const float* img_bias, int64_t rows_per_img, const float* scale, const float* shift,
                    int32_t act, const float* res, float* y, void* stream);

/* K4, split-bf16 form (see AMS_MATMUL_SPLIT_BF16): y = act((x @ w) * scale + shift) + res with w [K,N] f32 split on the
 * fly into bf16 hi/lo panels held in `panels` (uint16, >= 2*N*roundup(K,32) elements).  K % 8 == 0.
 * Scratch and panels of every ams_k_* entry: the caller need not zero them — an entry writes every element it later reads, the pad columns
 * K .. roundup(K,32) of a weight panel included — and an entry refuses (AMS_E_INVALID, nothing launched) a size below the minimum it states.
 * Accepts (this entry and ams_k_pointwise_split3): M, K, N > 0; K % 8 == 0 (any N >= 1); panels as stated.  Reads: x, w, y. */
int ams_k_pointwise_split(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale,
                          const float* shift, int32_t act, const float* res, float* y, uint16_t* panels,
                          size_t panel_elems, void* stream);

/* The same with the three-part split (hi, mid, lo: all 24 significand bits, 6 bf16 MFMAs per 32 k; AMS_MATMUL_SPLIT_BF16_X6);
 * panels >= 3*N*roundup(K,32) uint16. */
int ams_k_pointwise_split3(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale,
                           const float* shift, int32_t act, const float* res, float* y, uint16_t* panels,
                           size_t panel_elems, void* stream);

/* The frozen-block entries (ams_k_expand_dw, ams_k_block_fused[_f16], ams_k_expand_dw_stream[_f16], ams_k_dw_project, ams_k_first_block[_tiles])
 * refuse with AMS_E_INVALID, in this order and in front of their first launch: (first block) frames that are not uint8 / float32; B, H or W <= 0;
 * an unsupported shape, unknown form or number of parts; panels == NULL or panel_elems below what the call needs in all ("need N"); a NULL
 * tensor, weight or BN vector (res may be NULL: no residual). */
/* K4+K3 fused (frozen inference): y = relu6(bn_d(dw3x3(relu6(bn_e(x @ w_exp))))) for an inverted-residual block whose
 * input has Cin <= 64 channels; the expanded tensor never reaches HBM.  x [B,H,W,Cin], w_exp [Cin,Cexp], w_dw [3,3,Cexp,1],
 * y [B,Ho,Wo,Cexp] (SAME, stride 1|2, rate 1).  Cexp % 32 == 0 or % 48 == 0. */
int ams_k_expand_dw(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                    const float* shift_e, int32_t Cexp, const float* w_dw, int32_t stride, int32_t rate, const float* scale_d,
                    const float* shift_d, float* y, void* stream);

/* A whole early block in one kernel (k_block.hip): y = bn_p(relu6(bn_d(dw3x3(relu6(bn_e(x @ w_exp))))) @ w_proj) (+ x when residual != 0:
 * stride 1 and Cout == Cin only).  Cin % 4 == 0 and <= 32, Cexp % 16 == 0 and <= 384, Cout % 4 == 0 and <= 64, stride 1|2, rate 1
 * (the launcher picks the largest measured tile that fits 64 KB of LDS; AMS_E_INVALID for any other shape).
 * panels == NULL: exact f32 products in the k order of ams_k_pointwise — the same bits as ams_k_expand_dw followed by ams_k_pointwise.
 * panels != NULL (scratch of >= 3*Cexp*32 uint16) and Cin > 16: the EXPAND products as six bf16 MFMAs on three-part splits (all 24
 * significand bits, f32-level: what the engine does by default, AMS_OPT_BLOCK_X6); depthwise and project stay exact f32. */
int ams_k_block_fused(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e, const float* shift_e,
                      int32_t Cexp, const float* w_dw, int32_t stride, const float* scale_d, const float* shift_d, const float* w_proj, int32_t Cout,
                      const float* scale_p, const float* shift_p, int32_t residual, float* y, uint16_t* panels, size_t panel_elems, void* stream);

/* K4+K3 fused, streaming form for the stride-16 blocks (Cin in {64, 96, 160}, stride 1, rate 1|2, Cexp % 32 == 0): the same
 * result as ams_k_pointwise_split (parts = 2) / the three-part split (parts = 3) followed by ams_k_depthwise3x3, bit for bit,
 * without writing the expanded tensor.  panels: scratch of >= 3*Cexp*Cin uint16 (w_exp [Cin,Cexp] is split into it; three planes
 * whatever `parts` is).  In all: ns * Cexp*Cin + (presplit ? ns * B*H*W*Cin : 0) with ns = 3 here and 2 for ams_k_expand_dw_stream_f16.
 * Cin in {16, 24, 32}: exact-f32 products instead (bit-identical to ams_k_pointwise + ams_k_depthwise3x3; parts / presplit /
 * panels unused), and rate = -2 selects the stride-2 depthwise conv (y [B,Ho,Wo,Cexp], SAME).
 * presplit != 0: x is first written as bf16 parts (what the project GEMM of the previous block leaves behind in the engine) and
 * the kernel loads its operand from them; panels then needs 3*B*H*W*Cin more elements.  Same result, bit for bit. */
int ams_k_expand_dw_stream(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                           const float* shift_e, int32_t Cexp, const float* w_dw, int32_t rate, const float* scale_d,
                           const float* shift_d, float* y, uint16_t* panels, size_t panel_elems, int32_t parts, int32_t presplit,
                           void* stream);

/* The two-fp16-part forms (AMS_MATMUL_SPLIT_F16; k_pw_f16.hip, split_bf16.hpp): every operand x ~ hi + lo 2^-11 with hi = f16(x),
 * lo = f16((x - hi) 2^11); products hi hi + 2^-11 (hi lo + lo hi), 3 MFMAs per 32 k, f32 accumulate.
 * ams_k_pack_h2i: f32 [M][C] (C % 8 == 0) -> "H2I": per 8 channels 16 bytes of hi then 16 bytes of lo, 4 C bytes per row (what the streaming
 *   kernels write with y_h2i and the GEMM reads with x_h2i).  Accepts: M, C > 0; C % 8 == 0.  Reads: x, out.
 * ams_k_pointwise_split_f16: as ams_k_pointwise_split3 (K4; replaces the Conv2D nodes of model.meta `expanded_conv_N/project`, `aspp0`, ...);
 *   panels >= 2*N*Kp uint16; x_h2i (optional, M*K floats of scratch): x is first packed into H2I and the GEMM loads its operand from there —
 *   same result, bit for bit (x_h2i == x: x is taken as packed already); y_parts (optional, 2*M*N uint16): the result also as two fp16 part planes.
 *   Accepts: M, K, N > 0; K % 8 == 0 and K >= 32 (any N >= 1); with y_parts, N % 4 == 0 (the vector epilogue writes the planes); panels as
 *   stated.  Reads: x, w, y.
 * ams_k_expand_dw_stream_f16: as ams_k_expand_dw_stream with the fp16 parts (Cin 64 / 96 / 160); presplit 1 | 2 as there (2 = the
 *   weight-register form; panels then needs 2*B*H*W*Cin more elements); y_h2i != 0: y is written in H2I instead of f32.  Bit-identical to
 *   ams_k_pointwise_split_f16 followed by ams_k_depthwise3x3. */
int ams_k_pack_h2i(const float* x, int64_t M, int32_t C, float* out, void* stream);
/* ams_k_block_fused with the expand AND the project products on two fp16 parts (3 MFMAs each; K = 16 included); panels: scratch of
 * >= 2*Cexp*32 + 2*Cout*roundup(Cexp, 32) uint16 */
int ams_k_block_fused_f16(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                          const float* shift_e, int32_t Cexp, const float* w_dw, int32_t stride, const float* scale_d, const float* shift_d,
                          const float* w_proj, int32_t Cout, const float* scale_p, const float* shift_p, int32_t residual, float* y,
                          uint16_t* panels, size_t panel_elems, void* stream);
int ams_k_pointwise_split_f16(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale, const float* shift,
                              int32_t act, const float* res, float* y, uint16_t* panels, size_t panel_elems, float* x_h2i, uint16_t* y_parts,
                              void* stream);
int ams_k_expand_dw_stream_f16(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                               const float* shift_e, int32_t Cexp, const float* w_dw, int32_t rate, const float* scale_d,
                               const float* shift_d, float* y, uint16_t* panels, size_t panel_elems, int32_t presplit, int32_t y_h2i,
                               void* stream);

/* K3+K4 fused (frozen inference): y = bn_p(relu6(bn_d(dw3x3(e))) @ w_proj) (+ res) — the depthwise output never reaches
 * HBM; the product uses the two-part bf16 split of ams_k_pointwise_split.  e [B,H,W,C] (C % 32 == 0), w_dw [3,3,C,1],
 * stride 1, rate 1|2, w_proj [C,N] with N % 16 == 0 and N/16 in {1..6, 8, 10} or a multiple of 10 or 8 of those; res/y
 * [B,H,W,N]; panels: scratch of >= 2*N*C uint16. */
int ams_k_dw_project(const float* e, int32_t B, int32_t H, int32_t W, int32_t C, const float* w_dw, int32_t rate,
                     const float* scale_d, const float* shift_d, const float* w_proj, int32_t N, const float* scale_p,
                     const float* shift_p, const float* res, float* y, uint16_t* panels, size_t panel_elems, void* stream);

/* The first block of the frozen path in one kernel (k_first_block.hip): frames [B,H,W,3] (frames_dtype AMS_DT_U8 | AMS_DT_F32) -> one row and one
 * column of 127.5 -> x * pixel_scale - 1 -> stem 3x3 s2 (w_stem [3,3,3,32]) + BN + ReLU6 -> depthwise 3x3 (w_dw [3,3,32,1]) + BN + ReLU6 -> project
 * 1x1 (w_proj [32,16]) + BN = y [B, ceil((H+1)/2), ceil((W+1)/2), 16].  form 0: exact f32 products, the same bits as ams_k_stem_conv ->
 * ams_k_depthwise3x3 -> ams_k_pointwise; 1: the stem's products on three bf16 parts (six MFMAs); 2: the stem's and the project layer's on two fp16
 * parts (three MFMAs each; what the engine runs by default: uint8 frames walk the interior tiles, see ams_first_block_plan).  panels: scratch of
 * >= ams_k_first_block_scratch(form) uint16, into which the entry splits the weights as ams_student_freeze does (unused, may be NULL, for form 0).
 * plan_out (optional): what was launched.  Refused with AMS_E_INVALID before any launch, in this order: a frames_dtype other than the two; B, H or W
 * below 1; an unknown form; panels too small; a null pointer. */
typedef struct ams_first_block_plan {
    int32_t out_h, out_w, pad_top, pad_left;   /* y's grid; the stem's SAME padding in front of the (H+1) x (W+1) padded frame */
    int32_t tiles_y, tiles_x;                  /* 8 x 16 output tiles per frame */
    int32_t ity0, itx0, niy, nix;              /* interior tiles (every stem position of the tile + 1-pixel halo exists, every tap and every byte the
                                                  walking kernel loads for it lies inside the unpadded frame): rows [ity0, ity0 + niy), columns
                                                  [itx0, itx0 + nix); niy * nix = 0: none */
    int32_t interior_tiles, interior_grid;     /* the walking launch: tiles over the batch, blocks (0, 0: not launched) */
    int32_t border_tiles, border_grid;         /* the launch of all other tiles (with interior_tiles = 0: every tile, one per block) */
    int32_t border_walks;                      /* 1: that launch is the walking border kernel, 0: the one-tile kernel */
} ams_first_block_plan;
size_t ams_k_first_block_scratch(int32_t form);
int ams_k_first_block(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, float pixel_scale, const float* w_stem,
                      const float* scale_s, const float* shift_s, const float* w_dw, const float* scale_d, const float* shift_d, const float* w_proj,
                      const float* scale_p, const float* shift_p, float* y, int32_t form, uint16_t* panels, size_t panel_elems,
                      ams_first_block_plan* plan_out, void* stream);
/* The same block as one tile per wave (k_block.hip; exact f32, the same bits as form 0; AMS_OPT_FUSE_FIRST_BLOCK = 2). */
int ams_k_first_block_tiles(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, float pixel_scale, const float* w_stem,
                            const float* scale_s, const float* shift_s, const float* w_dw, const float* scale_d, const float* shift_d,
                            const float* w_proj, const float* scale_p, const float* shift_p, float* y, void* stream);
/* The plan ams_k_first_block would hand back, without a launch.  occupancy NULL: the blocks per CU of the two walking kernels and the CU count are
 * asked of the current device; else {interior blocks per CU, border blocks per CU, CUs}: pure host arithmetic, no GPU needed. */
int ams_k_first_block_plan(int32_t frames_dtype, int32_t B, int32_t H, int32_t W, int32_t form, const int32_t* occupancy, ams_first_block_plan* plan_out);
/* The steps that ams_k_expand_dw_stream (f16 == 0; Cin > 32: counted with three parts) or ams_k_expand_dw_stream_f16 (f16 != 0) would run for
 * these arguments (presplit 2: the weight-register form; rate -2 as there), without a launch: the launchers' own geometry (AMS_XDS_FORCE /
 * AMS_XWR_FORCE honoured) walked with the kernels' own step rule (csrc/xdw_steps.hpp).  Host arithmetic, no GPU needed.  A work item is a
 * segment of a sub-image; its roles walk it in steps of STEP positions: the E-waves expand, the D-waves run the depthwise conv one row behind.
 * out[0 .. 4]: STEP, Wp (row pitch of a segment), SH (its rows), T (steps of a whole segment: what every item ran before steps were
 *   skipped), items per channel chunk.
 * out[5 .. 9], summed over the items: steps executed, E-steps that compute, E-steps that only write zeros, D-steps with a stored centre,
 *   loop steps in which the E-step computes and the D-step is active.
 * n >= 10 + 5 * items: out[10 + 5 i ..] the same five figures of item i (the first is its T_item).
 * n >= 10 + (5 + T) * items: out[10 + 5 items + T i + t] = E class of step t of item i (0 idle, 1 zero, 2 compute) + 4 (D-step t active)
 *   + 8 (t < T_item: the step is executed). */
int ams_k_expand_dw_steps(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cexp, int32_t rate, int32_t f16, int32_t presplit, int32_t* out,
                          size_t n);

/* Frame ingest (reference run.py:179-183, :415-421: cv2.resize of the decoded frame to [H, 2H] + BGR->RGB; INTER_NEAREST for
 * the teacher label map).  src [Hs,Ws,C] uint8 -> dst [H,W,C] uint8, both device memory.  mode AMS_RESIZE_NEAREST |
 * AMS_RESIZE_LINEAR (OpenCV's 8-bit fixed-point INTER_LINEAR: 11-bit weights, integer passes, the 2x box-average shortcut; bit-identical
 * to the restatement in oracle/cv_resize.py, which hand-derived vectors pin); swap_rb != 0 reverses the 3 channels. */
enum { AMS_RESIZE_NEAREST = 0, AMS_RESIZE_LINEAR = 1 };
int ams_ingest_resize_u8(const uint8_t* src, int32_t Hs, int32_t Ws, int32_t C, int32_t mode, int32_t swap_rb, uint8_t* dst,
                         int32_t H, int32_t W, void* stream);

/* K7: global average pool [B,HW,C] -> [B,C] (two-stage, deterministic); scratch >= ams_k_global_mean_scratch floats. */
int ams_k_global_mean(const float* x, int32_t B, int64_t HW, int32_t C, float* y, float* scratch, size_t scratch_floats,
                      void* stream);
size_t ams_k_global_mean_scratch(int32_t B, int32_t C);

/* K9-K12: bilinear(align_corners) upsample of low-res logits to HxW fused with class gather, argmax and
 * (when teacher != NULL) confusion matrix + CE loss sums.  Full-resolution logits are never written.
 * conf_mat int64 [K*K] and loss double[2] are accumulators: the call zeroes both itself (on `stream`, in front of its kernel) — the caller
 * need not, and whatever they held is gone.  teacher == NULL: neither is touched.
 * The argmax is a strict `>` scan from class 0 in the order of class_idx_host over the K interpolated values: ties, and -0.0 against +0.0, take
 * the lower index; a NaN wins only in class 0 (a NaN there keeps label 0, a NaN elsewhere is never the label).  ams_k_upsample_confidence and
 * ams_k_upsample_soft_metric derive the same label, bit for bit.  A pixel whose teacher label is ignored (outside the subset) contributes
 * nothing to conf_mat and loss, whatever its logits hold.  A valid pixel whose loss is not finite (a NaN or an infinite logit among its taps,
 * a tap of weight 0 included) makes loss[0] non-finite; it is still counted in loss[1] and in conf_mat, under the label of the rule.  Frames
 * do not affect each other's labels or counts.  The loss of a pixel enters loss[0] rounded to a multiple of 2^-20. */
int ams_k_upsample_argmax(const float* logits /*[B,h,w,NC]*/, int32_t B, int32_t h, int32_t w, int32_t NC,
                          const int32_t* class_idx_host, int32_t K, int32_t H, int32_t W, const uint8_t* teacher,
                          int32_t* labels_out, int64_t* conf_mat, double* loss, void* stream);

/* The student's own certainty (create_student_v3's probabilities_reduced and loss_sel, utils/graph_utils.py:388-389, 410-418): the same walk
 * over the full-resolution pixels as ams_k_upsample_argmax (same interpolation, same argmax), per pixel p = max_k softmax_k = 1 / sum_k
 * exp(z_k - z_max).  Every output may be NULL (nothing is written there):
 *   conf_u8  uint8 [B,H,W]   rint(p * 255)
 *   conf_f32 float [B,H,W]   p
 *   stats    int64 [B][ams_confidence_stats_len()], one row per frame, overwritten:
 *            hist[NB] | hist_valid[NB] | hist_hit[NB] | bin_sum[NB] | sel_cnt[32] | sel_sum[32] | sum_all,  NB = AMS_CONFIDENCE_BINS
 *            bin = min(NB - 1, (int)(p * NB)); hist counts every pixel and sum_all adds their rint(p * 2^20).  The other fields need `teacher`
 *            (uint8 [B,H,W], NULL = none) and cover its valid pixels (label in the subset): hist_valid their number per bin, hist_hit those
 *            whose argmax is the teacher's class, bin_sum their summed rint(p * 2^20); sel_cnt[k] the valid pixels whose teacher class OR
 *            argmax is k (once when both are), sel_sum[k] their summed rint(CE * 2^20).  All integers: a frame's row does not depend on the
 *            batch it is computed in.  A pixel whose logits hold a NaN is counted in bin 0 and adds 0 to bin_sum and sum_all; a pixel
 *            loss that is not finite is counted in sel_cnt and adds 0 to sel_sum.  Such a pixel's conf_f32 is a NaN and its conf_u8 is 0.
 *            p == 1 (every other class underflows) is counted in the last bin.  A pixel the teacher ignores enters hist and sum_all alone. */
#define AMS_CONFIDENCE_BINS 32
int ams_k_upsample_confidence(const float* logits /*[B,h,w,NC]*/, int32_t B, int32_t h, int32_t w, int32_t NC,
                              const int32_t* class_idx_host, int32_t K, int32_t H, int32_t W, const uint8_t* teacher,
                              uint8_t* conf_u8, float* conf_f32, int64_t* stats, void* stream);
size_t ams_confidence_stats_len(void);

/* Evaluation of the soft-teacher objective (create_student_v3 with soft_teacher=True; prob_confmat / prob_confmat_star, utils/graph_utils.py:265-317,
 * and the soft loss, :375-376, 397, 403-408): the same walk over the full-resolution pixels as ams_k_upsample_argmax (same interpolation, same
 * argmax).  teacher_logits f32 [B,th,tw,NC] with th <= H, tw <= W: at the label size they are read as they are, a smaller grid is interpolated
 * as in ams_k_ce_loss_grad_soft.  Per pixel z = the K gathered student logits, t = the K gathered teacher logits, p = softmax(t),
 * ce = sum_k p_k (logsumexp(z) - z_k), in f32.  teacher uint8 [B,H,W]: a pixel is valid when its id is in the subset; NULL: every pixel is
 * valid (prob_confmat's unmasked form).  Every output may be NULL (nothing is written there):
 *   p_f32  float [B,H,W,K]  p          ce_f32  float [B,H,W]  ce          (every pixel, valid or not)
 *   stats  int64 [B][ams_soft_metric_stats_len(K)] = [B][2 + 2 K K], one row per frame, overwritten:
 *          valid_cnt | ce_sum | M_stu[K*K] | M_star[K*K]
 *          ce_sum = sum over the valid pixels of rint(ce * 2^20); M_stu[c*K + i] = sum over the valid pixels whose argmax is i of
 *          rint(p_c * 2^20); M_star[c*K + i] the same over those whose reduced teacher label is i (zeros when teacher == NULL): rows are the
 *          probability class, columns the label.  All integers: a frame's row does not depend on the batch it is computed in.  A valid pixel
 *          with a NaN in either logit vector, or whose ce is not finite, is counted in valid_cnt and adds 0 everywhere else.
 * AMS_E_INVALID, nothing written: B < 1, K outside 1..32, a teacher grid larger than H x W, more than 2047 rows per band of the launch grid
 * (H > 65504: a thread's 32-bit column sums). */
int ams_k_upsample_soft_metric(const float* logits /*[B,h,w,NC]*/, int32_t B, int32_t h, int32_t w, int32_t NC,
                               const int32_t* class_idx_host, int32_t K, int32_t H, int32_t W, const uint8_t* teacher,
                               const float* teacher_logits /*[B,th,tw,NC]*/, int32_t th, int32_t tw, int64_t* stats, float* p_f32,
                               float* ce_f32, void* stream);
/* The same for teacher logits in either layout (AMS_TLOGITS_*; utils/graph_utils.py:359, 375-376): AMS_TLOGITS_SELECTED reads teacher_logits as
 * f32 [B,th,tw,K], channel k = class class_idx_host[k].  ld >= NC: the row stride of `logits` (the engine's logits block has 32).  Also
 * AMS_E_INVALID, nothing launched, nothing written: a layout other than the two, class_idx_host == NULL. */
int ams_k_upsample_soft_metric_layout(const float* logits /*[B,h,w,ld]*/, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC,
                                      const int32_t* class_idx_host, int32_t K, int32_t H, int32_t W, const uint8_t* teacher,
                                      const float* teacher_logits, int32_t th, int32_t tw, int32_t layout, int64_t* stats, float* p_f32,
                                      float* ce_f32, void* stream);
size_t ams_soft_metric_stats_len(int32_t K);    /* 2 + 2 K K; 0 for K outside 1..32 */

/* K11 backward: d loss / d low-res logits (zeros for unselected classes); loss_and_count_dev: the double[2]
 * written by ams_k_upsample_argmax ([1] = number of valid pixels, the mean's denominator).
 * class_idx_host (here and above): HOST array of the K selected class ids; it travels by value.
 * A pixel whose teacher label is ignored contributes nothing, whatever its logits hold (it is skipped, not multiplied by 0).  A valid pixel
 * with a non-finite logit among its taps makes non-finite only the cells it is interpolated from: every other cell, every other frame
 * among them, holds the bits it holds without that pixel. */
int ams_k_ce_grad(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host,
                  int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const double* loss_and_count_dev,
                  float* dlogits, void* stream);

/* K11 forward + backward in ONE pass over the pixels (what the fine-tune step runs; replaces graph_utils.py:403-408 and its
 * gradient): loss_dev[0] = CE sum over valid pixels, loss_dev[1] = their number, dlogits [B*h*w, NC] = d(mean CE) / d low-res
 * logits (zeros for unselected classes).  Every pixel's softmax is evaluated once; no atomics touch the gradient (run-to-run
 * identical).  scratch: >= ams_k_ce_loss_grad_scratch floats.  AMS_E_INVALID when one source column spans more than ~20 output
 * columns (callers then use ams_k_upsample_argmax + ams_k_ce_grad).
 * Here and in the _soft, _kd, _weighted and _mined forms: a pixel whose teacher label is ignored contributes nothing to loss_dev or dlogits,
 * whatever its logits hold (it is skipped, not multiplied by 0).  A valid pixel whose loss is not finite (a NaN or an infinite logit among its
 * taps, a tap of weight 0 included) makes loss_dev[0] non-finite and is still counted in loss_dev[1]; it makes non-finite only the cells of
 * dlogits that one of its four taps names: every other cell, every other frame among them, holds the bits it holds without that pixel.
 * The loss of a pixel enters loss_dev[0] rounded to a multiple of 2^-20: a pixel loss below 2^-21 (a saturated, correct student) adds 0. */
int ams_k_ce_loss_grad(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host,
                       int32_t K, int32_t H, int32_t W, const uint8_t* teacher, double* loss_dev, float* dlogits,
                       float* scratch, size_t scratch_floats, void* stream);
size_t ams_k_ce_loss_grad_scratch(int32_t B, int32_t h, int32_t w, int32_t K);
/* The same with soft-teacher targets: teacher_logits f32 [B, th, tw, NC] (ams_student_feed_teacher_logits); `teacher` still masks the pixels. */
int ams_k_ce_loss_grad_soft(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host,
                            int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                            double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream);
/* The same for teacher logits in either layout (AMS_TLOGITS_*; utils/graph_utils.py:359, 375-376): AMS_TLOGITS_SELECTED reads teacher_logits as
 * f32 [B, th, tw, K], channel k = class class_idx_host[k].  ld (NC <= ld <= 256): the row stride of `logits` and of `dlogits`, whose pad
 * columns get 0 (the engine's logits block has 32).  AMS_E_INVALID, nothing launched, nothing written: a layout other than the two,
 * class_idx_host == NULL, K outside 1..32. */
int ams_k_ce_loss_grad_soft_layout(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                                   int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                                   int32_t layout, double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream);
/* The same under a temperature and a soft : hard mix (ams_student_set_kd has the objective).  temperature and alpha are checked first, before any
 * pointer is looked at: AMS_E_INVALID, nothing launched, nothing written, ams_last_error naming the argument.  (1, 1) is
 * ams_k_ce_loss_grad_soft_layout and alpha = 0 is ams_k_ce_loss_grad, bit for bit: the launcher sends them to those kernels. */
int ams_k_ce_loss_grad_kd(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                          int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                          int32_t layout, double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream,
                          float temperature, float alpha);
/* The same under per-class weights and the teacher-confidence weight (ams_student_set_loss_weights has the objective): loss_dev[1] = sum of the
 * quantised weights.  class_weights_host: K floats or NULL = ones.  temperature, alpha, then class_weights_host's entries and conf_gamma are checked
 * before any other pointer is looked at: AMS_E_INVALID, nothing launched, nothing written.  teacher_logits may be NULL when conf_gamma = 0 and
 * alpha = 0.  conf_gamma > 0 with alpha = 0 runs the mix form, which has the teacher's distribution.  All ones with conf_gamma = 0 is
 * ams_k_ce_loss_grad_kd, bit for bit. */
int ams_k_ce_loss_grad_weighted(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                                int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                                int32_t layout, double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream,
                                float temperature, float alpha, const float* class_weights_host, float conf_gamma);
/* The same over the hardest pixels alone (ams_student_set_loss_mining has the semantics): the key pass, the select and the relabel, then the two
 * launches of ams_k_ce_loss_grad_weighted on labels_out_dev.  labels_out_dev: uint8 [B, H, W], the mined map (a dropped pixel reads 255);
 * key_out_dev: f32 [B, H, W] or NULL (the keys then stay in the mining scratch), -1 at a pixel that is not valid; result_dev: 8-byte aligned;
 * mining_scratch_dev: 16-byte aligned, ams_k_loss_mining_scratch(B, H, W) bytes.  top_k = 1: the unmined entry, labels_out_dev a copy of
 * `teacher`, key_out_dev and result_dev untouched.  AMS_E_INVALID, nothing launched, nothing written: whatever ams_k_ce_loss_grad_weighted
 * refuses, in its order; then top_k outside (0, 1] or not finite; the mining scratch NULL, misaligned or too small; a NULL output. */
int ams_k_ce_loss_grad_mined(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                             int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                             int32_t layout, double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream,
                             float temperature, float alpha, const float* class_weights_host, float conf_gamma, float top_k,
                             uint8_t* labels_out_dev, float* key_out_dev, ams_mining_result* result_dev, void* mining_scratch_dev,
                             size_t mining_scratch_bytes);

/* K13: weight gradient of a 1x1 conv: dw[K,N] = x[M,K]^T @ dy[M,N]; x and dy are packed (row strides K and N).
 * scratch: the partial products of the row splits, written before they are summed (nothing to zero): splits * K * N floats, where
 *   ams_k_pointwise_wgrad (exact f32):  splits = max(min(ceil(1024 / tiles), ceil(M / 256)), 1), tiles = ceil(K / 64) * ceil(N / 64);
 *   ams_k_pointwise_wgrad_split (K13b): splits = max(min(ceil(512 / tiles), ceil(M / 256), 32), 1), tiles = ceil(K / (16 kt)) * ceil(N / (16 nw)),
 *     kt = 8 for K > 64 and 4 up to there; with n16 = ceil(N / 16): nw = 4 | 5 | 6 | 8 | 10 for n16 <= 4 | 5 | 6 | 8 | 10, above that
 *     10, 8 or 6 where it divides n16 (tried in that order) and 8 otherwise.
 * Each entry refuses (AMS_E_INVALID) fewer floats than ITS formula gives; ams_k_pointwise_wgrad_scratch returns the larger of the two, which
 * serves either entry and ams_k_pointwise_wgrad_xform with either value of split.
 * Accepts (ams_k_pointwise_wgrad): M, K, N > 0, any K and N (the launcher picks one of nine vector-width pairs <VA, VB>: 1 up to 16 channels, at
 * most 2 up to 32, else the widest of 4 / 2 / 1 that divides the count).  Reads: x, dy, dw. */
int ams_k_pointwise_wgrad(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, float* dw,
                          float* scratch, size_t scratch_floats, void* stream);
size_t ams_k_pointwise_wgrad_scratch(int64_t M, int32_t K, int32_t N);
/* K13b: the same on the bf16 matrix pipe with both operands split into three bf16 parts (six products, f32-level
 * accuracy): the kernel the fine-tune step uses for its late layers (few pixels, many channel pairs).
 * Accepts: M, K, N > 0; 1024 <= M <= 32768, K and N multiples of 4, K*N >= 4096.  Reads: x, dy, dw. */
int ams_k_pointwise_wgrad_split(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, float* dw,
                                float* scratch, size_t scratch_floats, void* stream);

/* K13: depthwise backward: dx (input gradient) and dw[3,3,C,1].  ams_k_depthwise3x3_wgrad's scratch holds one 9 x C partial per block, each written
 * whole before the second stage sums them (nothing to zero): scratch_floats >= blocks * 9 * C with items = B * ceil(Ho / 4) * Wo,
 * slots = max(256 / (C / 4), 1), blocks = min(ceil(items / (2 * slots)), max(items * 2 / 9, 1), 1024); AMS_E_INVALID below that.
 * Accepts: as ams_k_depthwise3x3.  Reads: dy, w, dx (dgrad); x, dy, dw (wgrad). */
int ams_k_depthwise3x3_dgrad(const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, const float* w,
                             int32_t stride, int32_t rate, float* dx, void* stream);
int ams_k_depthwise3x3_wgrad(const float* x, const float* dy, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t stride, int32_t rate, float* dw, float* scratch, size_t scratch_floats,
                             void* stream);

/* A 1x1 conv of the fine-tune step with a BN column reduction in its epilogue (pw_common.hpp pw_red_*; what FusedBatchNormV3 /
 * FusedBatchNormGradV3's reductions are to the reference's graph).  y [M,N] = x [M,K] . w [K,N] (trans_w: w is [N,K], the dgrad orientation).
 *   mode 1: partial rows [rows][2][N] of sum(y - center), sum((y - center)^2)            (forward statistics; center may be NULL)
 *   mode 2: y is the gradient wrt the ACTIVATED output of a BN layer with raw output z [M,N]: y (+ res [M,N] first, if given) is multiplied by
 *           act'(z scale + shift) BEFORE it is stored; partial rows of sum(y), sum(y (z - mean) rstd)   (first half of that layer's BN backward)
 * split 1: the three-part bf16 kernel (panels: >= 3 N Kp bf16 scratch); split 2: the two-fp16-part kernel (mode 1 only: what the fine-tune step's
 * forward runs under AMS_MATMUL_SPLIT_F16; panels >= 2 N Kp); 0: the exact-f32 streaming kernel.  *rows_out = 0 means the kernel
 * chosen for this shape cannot fuse the reduction (y is then the plain product, + res): the caller runs the separate pass.
 * part_floats >= (M / 64 + 8 or 2048, whichever is larger) * 2 N; rows that would not fit make the launch run unfused (*rows_out = 0), no
 * refusal.  The *rows_out rows are written whole; the rest of `part` is left alone.  Nothing in `part` or `panels` needs zeroing.
 * Accepts: M, K, N > 0; mode 1 | 2; split 0: K % 4 == 0; split 1: K % 8 == 0; split 2: mode 1, K % 8 == 0 and K >= 32; panels as stated.
 * Reads: x, w, y, part, rows_out, and with mode 2 z, scale, shift, mean, rstd. */
int ams_k_pointwise_red(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w, int32_t split, int32_t mode,
                        const float* center, const float* z, const float* scale, const float* shift, const float* mean, const float* rstd,
                        int32_t act, const float* res, float* y, float* part, size_t part_floats, int32_t* rows_out, uint16_t* panels,
                        size_t panel_elems, void* stream);

/* The 1x1 kernels of the fine-tune step with an elementwise BN pass applied on their OPERAND loads instead of being written first
 * (PwArgs / WgArgs x_mode, dy_mode; AMS_OPT_FUSE_OPERAND_BN): same IEEE operations in the same order as the pass, so the result is
 * bit-identical to running the pass and then the plain kernel.
 *   ams_k_pointwise_xform: y [M,N] = x' . w with x' = act(x * v0[k] + v1[k]) (x_mode 1: BN + activation, what FusedBatchNormV3 + Relu6 are to
 *     the reference's graph) or x' = v0[k] * x + v1[k] + v2[k] * x2 (x_mode 2: the second half of FusedBatchNormGradV3, (v0, v1, v2) = (A, B, C),
 *     x2 = the BN layer's raw output).  split 1: the three-part bf16 kernel (panels >= 3 N Kp), split 2 (x_mode 1 only): the two-fp16-part kernel, else the exact-f32 kernels.  A kernel that
 *     cannot transform on load writes x' into x_tmp [M,K] first (may be NULL: then such shapes fail with AMS_E_INVALID).
 *   ams_k_pointwise_wgrad_xform: dw [K,N] = x'^T . dy' with x' as x_mode 1 (x_mode 0: x' = x) and dy' = d0[n] * dy + d1[n] + d2[n] * dy2
 *     (dy_mode 2; dy_mode 0: dy' = dy); split != 0 the six-product bf16 kernel (shapes as ams_k_pointwise_wgrad_split).
 * Accepts (xform): M, K, N > 0; x_mode 1 | 2; split 0: K % 4 == 0; split 1: K % 8 == 0; split 2: x_mode 1, K % 8 == 0, 32 <= K <= 1024, N % 4 == 0;
 *   panels as stated.  Reads: x, w, y, v0, v1, and with x_mode 2 v2, x2.
 * Accepts (wgrad_xform): M, K, N > 0; x_mode 0 | 1, dy_mode 0 | 2; split != 0: the shapes of ams_k_pointwise_wgrad_split; scratch as the entry of
 *   the same split.  Reads: x, dy, dw, with x_mode 1 v0, v1, with dy_mode 2 d0, d1, d2, dy2. */
int ams_k_pointwise_xform(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w, int32_t split, int32_t x_mode,
                          int32_t x_act, const float* v0, const float* v1, const float* v2, const float* x2, float* y, float* x_tmp,
                          uint16_t* panels, size_t panel_elems, void* stream);
int ams_k_pointwise_wgrad_xform(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, int32_t split, int32_t x_mode, int32_t x_act,
                                const float* v0, const float* v1, int32_t dy_mode, const float* d0, const float* d1, const float* d2,
                                const float* dy2, float* dw, float* scratch, size_t scratch_floats, void* stream);

/* The fine-tune step's one-kernel forms of a stride-1 depthwise layer inside a block that keeps its tensors (what tf.gradients spreads over
 * FusedBatchNormV3 / Relu6 / DepthwiseConv2dNative and their Grad ops, SemanticNetwork.py:253-260 via utils/graph_utils.py:457-496):
 *   forward: zd [B,H,W,C] = dwconv3x3(act(ze * scale + shift), w) (rate 1 | 2, SAME: the ACTIVATION is zero-padded), and partial rows
 *            [rows][2][C] of sum(zd - center), sum((zd - center)^2) (center may be NULL) in scratch; *rows_out = rows;
 *   backward: out [B,H,W,C] = dwconv3x3^T(dz, w) * act'(z_prev * scale + shift), and partial rows [rows][11][C] of sum(out),
 *            sum(out * (z_prev - mean) * rstd) and the nine taps of the depthwise weight gradient sum(act(z_prev * scale + shift) . dz).
 * scratch_floats must be at least the matching *_scratch().
 * Accepts (all four, and the two tile forms below): as ams_k_depthwise3x3 with stride 1; ams_k_depthwise3x3_fwd_bn_tiles: H * W * C < 2^31.
 * Reads: every tensor and vector but center (NULL: sums about zero), and rows_out. */
size_t ams_k_depthwise3x3_fwd_bn_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate);
int ams_k_depthwise3x3_fwd_bn(const float* ze, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate,
                              const float* scale, const float* shift, int32_t act, const float* center, float* zd, float* scratch,
                              size_t scratch_floats, int32_t* rows_out, void* stream);
size_t ams_k_depthwise3x3_dgrad_bn_scratch(int32_t B, int32_t H, int32_t W, int32_t C);
int ams_k_depthwise3x3_dgrad_bn(const float* dz, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate,
                                const float* z_prev, const float* scale, const float* shift, int32_t act, const float* mean,
                                const float* rstd, float* out, float* scratch, size_t scratch_floats, int32_t* rows_out, void* stream);
/* ... with the depthwise layer's own BN-backward apply pass folded in (AMS_OPT_FUSE_DGRAD_BN = 3, k_dw_train.hip): the gradient entering the
 * transposed conv is dz_d = cA dy + cB + cC zd, formed once per element on the way into an LDS ring (the unfused operations of the apply pass:
 * `out` is bit-identical to ams_k_depthwise3x3_dgrad_bn on the materialised dz_d); partial rows [rows][11][C] as above, split differently. */
size_t ams_k_depthwise3x3_dgrad_bn_apply_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate);
/* the forward in the same LDS-tile form (act(ze scale + shift) formed once per element; zd bit-identical to ams_k_depthwise3x3_fwd_bn) */
size_t ams_k_depthwise3x3_fwd_bn_tiles_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate);
int ams_k_depthwise3x3_fwd_bn_tiles(const float* ze, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate, const float* scale,
                                    const float* shift, int32_t act, const float* center, float* zd, float* scratch, size_t scratch_floats,
                                    int32_t* rows_out, void* stream);
int ams_k_depthwise3x3_dgrad_bn_apply(const float* dy, const float* zd, const float* cA, const float* cB, const float* cC, int32_t B, int32_t H, int32_t W,
                                      int32_t C, const float* w, int32_t rate, const float* z_prev, const float* scale, const float* shift, int32_t act,
                                      const float* mean, const float* rstd, float* out, float* scratch, size_t scratch_floats, int32_t* rows_out,
                                      void* stream);

/* The fine-tune step of an early inverted-residual block WITHOUT its 6x-expanded tensors (k_xdw_train.hip; Cin 8..32, Cexp 32..192 in 16s,
 * depthwise stride 1 | 2, rate 1): every pass recomputes z_e = x . w_exp from the block input x [B,H,W,Cin].  KP = Cin rounded up to 16.
 *   fwd_stats : partial rows  S [2][Cexp] = sum(z_e - center), sum((z_e - center)^2) | XX [KP][KP] = x^T x | g0 [KP] = sum x
 *   bwd_reduce: with dz_d = gradient wrt the depthwise layer's raw output [B,Ho,Wo,Cexp]: dy_e = dwconv^T(dz_d) . act'(z_e sc + sh);
 *               partial rows  S [2][Cexp] = sum dy_e, sum dy_e xhat_e | dWd [9][Cexp] (depthwise weight gradient) | G1 [KP][Cexp] = x^T dy_e
 *   bwd_dx    : dx [B,H,W,Cin] = (cA dy_e + cB + cC z_e) . w_exp^T (+ res)
 *   dwe       : dw_exp [Cin][Cexp] = cA G1 + g0^T cB + cC (XX . w_exp) from the REDUCED rows (G1; XX | g0 contiguous)
 * rows of *stride_out floats, *rows_out of them, in scratch (>= ams_k_xdw_train_scratch floats).
 * Accepts (fwd_stats, bwd_reduce, bwd_dx): B, H, W, Cin, Cexp > 0; Cin % 4 == 0 in 8 .. 32, Cexp % 16 == 0 in 32 .. 192, stride 1 | 2 (fwd_stats has
 *   none), H * W * max(Cin, Cexp) < 2^31.  Reads: every tensor and vector but center and res (NULL: none), rows_out, stride_out.
 * Accepts (bwd_reduce_stem): B, fH, fW > 0; frames_dtype AMS_DT_U8 | AMS_DT_F32, fH * fW * 3 < 2^31.  Reads: all its pointers.
 * Accepts (dwe): Cin, Cexp > 0; Cin <= 32 (the stem's 27 taps included: rows of KP = Cin rounded up to 16), Cexp % 16 == 0 in 32 .. 192.
 *   Reads: all its pointers. */
/* BN statistics of an early block's expand layer from the Gram matrix of the block input (AMS_OPT_TRAIN_RECOMPUTE = 2, k_xx_stats.hip; what
 * FusedBatchNormV3's reduction over z_e = x . W_e is to the reference's graph): ams_k_xx_gram forms XX = x^T x [KP][KP] and g0 = sum x [KP]
 * (KP = Cin rounded up to 16, Cin <= 32) over the M rows of x [M, Cin] on the f64 matrix pipe — xx64: KP KP + KP doubles, xx32 (may be NULL) the
 * same as floats; ams_k_expand_stats turns them into scale / shift / saved mean / rstd (and the moving averages, sums [2][Cexp] about
 * `center`, both optional) of the BN over n pixels: sum z = g0 . w, sum z^2 = w^T XX w per channel, in f64.
 * Accepts (xx_gram): M, Cin > 0; 4 <= Cin <= 32.  Reads: x, xx64 (xx32 optional); scratch >= ams_k_xx_gram_scratch doubles.
 * Accepts (expand_stats): Cin, Cexp, n > 0; 4 <= Cin <= 32.  Reads: xx64, w_exp, gamma, beta, scale, shift; save_mean and save_rstd, and
 *   moving_mean and moving_var, each as a pair or both NULL; center and sums optional. */
size_t ams_k_xx_gram_scratch(int64_t M, int32_t Cin);
int ams_k_xx_gram(const float* x, int64_t M, int32_t Cin, double* scratch, size_t scratch_doubles, double* xx64, float* xx32, void* stream);
int ams_k_expand_stats(const double* xx64, int32_t Cin, const float* w_exp, int32_t Cexp, double n, const float* center, const float* gamma,
                       const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale, float* shift,
                       float* save_mean, float* save_rstd, double* sums, void* stream);

size_t ams_k_xdw_train_scratch(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cexp);
int ams_k_xdw_fwd_stats(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* center,
                        float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream);
int ams_k_xdw_bwd_reduce(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* sc_e,
                         const float* sh_e, const float* mean_e, const float* rstd_e, int32_t act_e, const float* w_dw, int32_t stride,
                         const float* dz_d, float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream);
int ams_k_xdw_bwd_dx(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* sc_e,
                     const float* sh_e, int32_t act_e, const float* w_dw, int32_t stride, const float* dz_d, const float* cA, const float* cB,
                     const float* cC, const float* res, float* dx, void* stream);
/* the first block of the network in the same form: the stem conv (3x3 stride 2 over the normalised, 127.5-padded frame, 3 -> 32) is the
 * "expand" layer over its 27-tap patch (k = tap * 3 + channel), followed by the first depthwise conv.  One pass over dz_d [B,H1,W1,32] and
 * the frames: partial rows  S [2][32] | dWd [9][32] | G1 [32][32] (27 rows used) | XX [32][32] | g0 [32]. */
size_t ams_k_xdw_stem_scratch(int32_t B, int32_t fH, int32_t fW);
int ams_k_xdw_bwd_reduce_stem(const void* frames, int32_t frames_dtype, int32_t B, int32_t fH, int32_t fW, float pixel_scale, const float* w_stem,
                              const float* sc_e, const float* sh_e, const float* mean_e, const float* rstd_e, int32_t act_e, const float* w_dw,
                              const float* dz_d, float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream);
int ams_k_xdw_dwe(const float* G1, const float* xx_g0, int32_t Cin, int32_t Cexp, const float* w_exp, const float* cA, const float* cB,
                  const float* cC, float* dw_exp, void* stream);

/* ---- The BN pieces of the fine-tune step (k_elementwise.hip), each alone.  What FusedBatchNormV3(is_training=True), its gradient, Relu6 / Relu6Grad
 * and the reductions behind them are to the reference's graph.  All tensors f32, [M, C] dense unless an ld is given; sums are f64 [2][C].
 *
 * The column reductions run in two stages.  ams_k_col_plan gives the geometry of the first: CG = C / 4 lanes along the channels, slots = max(1, 256 / CG)
 * rows per block step, chunks = min(1024, ceil(M / (16 * slots))) blocks per group, rows_per_chunk = ceil(M / chunks) rows each (chunk k owns rows
 * [k * rows_per_chunk, min(M, (k + 1) * rows_per_chunk)); with the cap in force trailing chunks can be empty).  out = {CG, slots, chunks, rows_per_chunk}.
 * Host arithmetic: no GPU call.  C must be a multiple of 4, at most 1024.
 * Scratch sizes (floats), independent of M: the first stage leaves one row of NQ * C partial sums per chunk, and at most 1024 chunks run:
 *   ams_k_colstats_scratch(M, C)       = 1024 * 2 * C    (ams_k_colstats, ams_k_colstats_bn, ams_k_bn_bwd_reduce, ams_k_bn_bwd_reduce_coef: NQ = 2)
 *   ams_k_colsum_scratch(C)            = 1024 * C        (NQ = 1)
 *   ams_k_image_colsum_scratch(B, C)   = B * 1024 * C    (one group per image; the same as ams_k_global_mean_scratch)
 * The second stage adds the chunks' rows in f64 in a fixed order: results are the same bits from run to run. */
int ams_k_col_plan(int64_t M, int32_t groups, int32_t C, int32_t* out /* [4] */);
/* sums[0][c] = sum_m (z[m,c] - center[c]), sums[1][c] = sum_m (z[m,c] - center[c])^2; center == NULL: 0.  The differences, squares and the sums within
 * a chunk are f32 (ams_k_colstats), or everything is f64 with one thread per channel (ams_k_colstats_f64: layers of a few rows). */
size_t ams_k_colstats_scratch(int64_t M, int32_t C);
int ams_k_colstats(const float* z, int64_t M, int32_t C, const float* center, double* sums, float* scratch, size_t scratch_floats, void* stream);
int ams_k_colstats_f64(const float* z, int64_t M, int32_t C, const float* center, double* sums, void* stream);
/* the per-channel arithmetic from such sums over n elements: d1 = sums[0] / n, var = max(0, sums[1] / n - d1^2) (f64); mean = f32(center + d1),
 * rstd = 1 / sqrtf(f32(var) + eps), scale = gamma * rstd, shift = beta - mean * scale (f32).  With moving_mean != NULL (then moving_var too):
 * moving -= (moving - stat) * one_minus_decay in f32, stat = mean and the UNBIASED variance f32(var * n / (n - 1)) (n = 1: var).  save_mean / save_rstd
 * may be NULL together. */
int ams_k_bn_finalize(const double* sums, double n, int32_t C, const float* center, const float* gamma, const float* beta, float eps,
                      float one_minus_decay, float* moving_mean, float* moving_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                      void* stream);
/* ams_k_colstats + ams_k_bn_finalize in two launches (the single-process step): the second stage does the per-channel arithmetic.  Also writes sums. */
int ams_k_colstats_bn(const float* z, int64_t M, int32_t C, const float* center, double* sums, float* scratch, size_t scratch_floats, double n,
                      const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale,
                      float* shift, float* save_mean, float* save_rstd, void* stream);
/* The second stages alone, over partial rows part [rows][2][C] that a fused kernel left (ams_k_pointwise_red, ams_k_depthwise3x3_*_bn*, ams_k_xdw_*),
 * row_stride floats apart (0: dense = 2 * C): sums[q][c] = sum_r part[r * row_stride + q * C + c] in f64, then the arithmetic of ams_k_bn_finalize
 * (ams_k_bn_fwd_partials), of ams_k_bn_bwd_coef with dgamma and dbeta (ams_k_bn_bwd_partials), or none (ams_k_partials_to_sums: the data-parallel
 * step all-reduces the sums first).  Nothing but those rows * 2 * C floats is read. */
int ams_k_bn_fwd_partials(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, double n, const float* center,
                          const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale,
                          float* shift, float* save_mean, float* save_rstd, void* stream);
int ams_k_bn_bwd_partials(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, double n, const float* gamma, const float* mean,
                          const float* rstd, float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, void* stream);
int ams_k_partials_to_sums(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, void* stream);
/* backward sums: dy = da * mask, mask = act'(y) of y = f32(f32(z * scale) + shift) (RELU6: 0 < y < 6, RELU: y > 0, NONE: 1);
 * sums[0][c] = sum_m dy, sums[1][c] = sum_m (dy * (z - mean)) * rstd, terms in f32.  Scratch: ams_k_colstats_scratch. */
int ams_k_bn_bwd_reduce(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* mean,
                        const float* rstd, double* sums, float* scratch, size_t scratch_floats, void* stream);
/* from those sums over n elements, in f64 rounded once: A = gamma * rstd, k = A * (sums[1] / n) * rstd, coefA = A, coefC = -k,
 * coefB = -A * (sums[0] / n) + k * mean, so that dz = A dy + B + C z; dgamma = sums[1], dbeta = sums[0] (may be NULL together in ams_k_bn_bwd_coef;
 * ams_k_bn_param_grads writes only these two: a data-parallel rank's own share). */
int ams_k_bn_bwd_coef(const double* sums, double n, int32_t C, const float* gamma, const float* mean, const float* rstd, float* coefA, float* coefB,
                      float* coefC, float* dgamma, float* dbeta, void* stream);
int ams_k_bn_param_grads(const double* sums, int32_t C, float* dgamma, float* dbeta, void* stream);
/* ams_k_bn_bwd_reduce + ams_k_bn_bwd_coef in two launches (the single-process step). */
int ams_k_bn_bwd_reduce_coef(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act,
                             const float* mean, const float* rstd, double* sums, float* scratch, size_t scratch_floats, double n, const float* gamma,
                             float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, void* stream);
/* apply passes, one IEEE f32 operation at a time (nothing fused): a = act(f32(f32(z * scale) + shift)) (+ res when res != NULL);
 * dz = ((coefA * (da * mask)) + coefB) + (coefC * z), mask as in ams_k_bn_bwd_reduce; dz may be da (in place).  C a multiple of 4. */
int ams_k_bn_act(const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* res, float* a, void* stream);
int ams_k_bn_bwd_apply(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* coefA,
                       const float* coefB, const float* coefC, float* dz, void* stream);
/* frozen coefficients: scale = gamma * (1 / sqrtf(var + eps)), shift = beta - mean * scale (f32) */
int ams_k_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int32_t C, float* scale, float* shift,
                  void* stream);
/* plain folds: out[i] = f32(sum_k part[k * stride + i]) for i < n, k < splits, in f64 in a fixed order (stride >= n).  ams_k_reduce_batch does up to 32
 * such folds in one launch (arrays of n_jobs entries, host memory); more jobs are refused before anything is launched.  No scratch. */
int ams_k_reduce_splits(const float* part, int32_t splits, int64_t n, int64_t stride, float* out, void* stream);
int ams_k_reduce_batch(const float* const* part, const int32_t* splits, const int64_t* count, const int64_t* stride, float* const* out, int32_t n_jobs,
                       void* stream);
/* column sums of x [M, ldx] (the first C columns): out[c] = sum_m x[m, c]; per image: x [B, HW, ldx], out [B, C].  ldx a multiple of 4. */
size_t ams_k_colsum_scratch(int32_t C);
int ams_k_colsum(const float* x, int64_t M, int32_t C, int32_t ldx, float* out, float* scratch, size_t scratch_floats, void* stream);
size_t ams_k_image_colsum_scratch(int32_t B, int32_t C);
int ams_k_image_colsum(const float* x, int32_t B, int64_t HW, int32_t C, int32_t ldx, float* out, float* scratch, size_t scratch_floats, void* stream);

/* regularize=True over a flat arena with a byte mask of the regularised entries: grads[i] = grads[i] + (coef / n_vars) * params[i] where mask[i] != 0
 * (f32, two operations; the others untouched), and loss[0] += 0.5 * coef / n_vars * sum_mask params^2 * loss[1] with the sum and the update in f64
 * (loss = {CE sum, valid pixels}, as the loss kernels leave it).  Scratch: 256 doubles (one per block). */
int ams_k_l2_regularizer(const float* params, float* grads, const uint8_t* mask, int64_t n, int32_t n_vars, float coef, double* scratch,
                         size_t scratch_doubles, double* loss, void* stream);

/* K14-K16: fused Adam + coordinate-descent mask over a flat arena (TF1 Adam, Appendix C.10). */
int ams_k_adam(float* params, const float* grads, float* m, float* v, const uint8_t* mask, int64_t n, float lr_t,
               float beta1, float beta2, float eps, void* stream);

/* Test hook (no GPU needed): the per-DEVICE bookkeeping behind the one-time kernel attributes (dynamic LDS limits).  Returns 1
 * when (device, kernel_key) has not yet been granted `lds` bytes — i.e. the launcher would call hipFuncSetAttribute now — and
 * records the grant; 0 otherwise.  Two students on two GPUs of one process each get their attributes set. */
int ams_debug_launch_table_needs_attr(int32_t device, uint64_t kernel_key, size_t lds);
/* Tests and tools/ only.  The tuning knobs (environment variables AMS_BLK_TILE, AMS_BLK_HP, AMS_PW_FORCE, AMS_PW_PERCU, AMS_PWX_NO_TAIL, AMS_PWX_FORCE,
 * AMS_PWH_VARIANT, AMS_XDS_FORCE, AMS_XWR_FORCE, AMS_WG6_SPLITS, AMS_WG6_EIGHT_WAVES, AMS_FB_WALK (first block: 0 one tile per block, -2 only the border
 * tiles so, n at most n tiles per walking block): tile / grid / form overrides of single kernels, same results; AMS_BLK_TIMED, AMS_XWR_TIMED: the kernels' phase clocks
 * (ams_debug_phase_cycles; correct results).  AMS_PWH_ABL, AMS_XWR_ABL, AMS_FB_ABL (kernels with loads / MFMAs / stores removed: WRONG results by design; AMS_FB_ABL=32
 * and AMS_XWR_TIMED on the weight-register kernel: clocked forms) exist ONLY in the measurement build libams_hip_measure.so (`make -C ams_amd/csrc measure`, compiled with
 * -DAMS_MEASURE, selected by tools/ through AMS_HIP_LIB): this library has no such kernels, names the variables on stderr and ignores them.  AMS_SIDE_CU_MASK=<hex>: the
 * fine-tune step's side stream confined to the CUs whose bit is set; AMS_EVENT_FLAGS=<hex>: hipEventCreateWithFlags flags of the
 * stream-ordering events — these two change stream semantics and exist for measurements only) are read ONCE, at first use; this re-reads
 * them.  Not thread-safe against launches in flight. */
int ams_debug_reload_knobs(void);
/* tools/ only.  Shader-clock cycles per wave and phase, summed over the launches since the last call, copied to out[0..n) (n <= 8) and cleared.
 * (which = 0 and 2 need the measurement build, see ams_debug_reload_knobs.)
 * which = 0: the walking first block with AMS_FB_ABL=32 ([0] tile decode, [1] stem, [2] wait at the barrier, [3] depthwise + project, [6] wave-tiles);
 * which = 1: the whole-block kernels with AMS_BLK_TIMED=1 ([0] prologue, [1] expand phases, [2] depthwise + project phases, [3] epilogue, [6] waves);
 * which = 2 / 3: the weight-register / the LDS-weight streaming kernel with AMS_XWR_TIMED=1 ([0] E-waves between the step barriers, [1] E-waves at the barrier, [2] / [3]
 * the same for the D-waves, [6] E-wave steps, [7] D-wave steps). */
int ams_debug_phase_cycles(int32_t which, uint64_t* out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* AMS_HIP_H */
