// The student engine, part 4 of 4: the C ABI of include/ams_hip.h — student lifetime, the calls behind SemanticNetwork's methods, options,
// the profiler read-out, and the kernel-level entry points (ams_k_*) the parity tests drive.
#include "engine.hpp"
#include "head_common.hpp"
#include "entry_check.hpp"

using namespace ams;

// =========================================================================================================
// C ABI
// =========================================================================================================
extern "C" {

const char* ams_last_error(void) { return ams::last_error(); }
int ams_abi_version(void) { return AMS_ABI_VERSION; }

int ams_device_info(char* name_out, size_t name_cap, int32_t* n_cu, int64_t* hbm_bytes) {
    int dev = 0;
    AMS_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    AMS_CHECK_HIP(hipGetDeviceProperties(&p, dev));
    if (name_out && name_cap) { snprintf(name_out, name_cap, "%s (%s)", p.name, p.gcnArchName); }
    if (n_cu) *n_cu = p.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)p.totalGlobalMem;
    return AMS_OK;
}

int ams_student_arena_bytes(const ams_student_config* cfg, const ams_layer_desc* layers, size_t* bytes_out) {
    AMS_REQUIRE(bytes_out, "arena_bytes: null output");
    ams_student tmp;
    int rc = student_build(&tmp, cfg, layers);
    if (rc) return rc;
    return student_layout(&tmp, nullptr, bytes_out);
}

int ams_student_create(const ams_student_config* cfg, const ams_layer_desc* layers, void* arena_dev, size_t arena_bytes,
                       ams_student** out) {
    AMS_REQUIRE(out && arena_dev, "create: null pointer");
    AMS_REQUIRE(((uintptr_t)arena_dev & 255) == 0, "create: arena must be 256-byte aligned");
    ams_student* s = new ams_student();
    int rc = student_build(s, cfg, layers);
    size_t need = 0;
    if (!rc) rc = student_layout(s, arena_dev, &need);
    if (!rc && need > arena_bytes) { set_error("create: arena too small (%zu < %zu)", arena_bytes, need); rc = AMS_E_NOMEM; }
    if (rc) { delete s; return rc; }
    s->arena = (char*)arena_dev;
    s->arena_bytes = arena_bytes;
    {   // events are free; STREAMS are not: the runtime multiplexes them onto a handful of hardware queues (GPU_MAX_HW_QUEUES, 4 by
        // default), and two streams that land on one queue serialise.  A student therefore owns only the streams it uses: the part
        // streams appear with the first multi-part call (never inside a graph capture: ensure_part_streams).
        int e = create_sync_event(&s->ev_fork_dual);
        for (int k = 0; k < 3 && e == AMS_OK; ++k) e = create_sync_event(&s->part_done[k]);
        if (e != AMS_OK) { delete s; return e; }
    }
    if (s->vec_ones) {
        std::vector<float> ones(1024, 1.0f), zeros(1024, 0.0f);
        hipError_t e = hipMemcpy(s->vec_ones, ones.data(), 1024 * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s->vec_zeros, zeros.data(), 1024 * sizeof(float), hipMemcpyHostToDevice);
        std::vector<float> inv(1024, (float)(1.0 / ((double)s->h * s->w)));
        if (e == hipSuccess) e = hipMemcpy(s->vec_inv_hw, inv.data(), 1024 * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("create: uploading constants -> %s", hipGetErrorString(e)); delete s; return AMS_E_HIP; }
    }
    if (!s->tp_jobs.empty()) {
        for (size_t k = 0; k < s->tp_jobs.size(); ++k) {
            SplitJob& j = s->tp_jobs[k];
            j.w = s->params + (int64_t)(uintptr_t)j.w;
            j.p0 = s->tp_panels + (size_t)(uintptr_t)j.p0;
            s->tp_index[{j.w, j.sk == 1 ? 1 : 0}] = (int)k;
        }
        const hipError_t e = hipMemcpy(s->tp_jobs_dev, s->tp_jobs.data(), s->tp_jobs.size() * sizeof(SplitJob), hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error("create: uploading the panel table -> %s", hipGetErrorString(e)); delete s; return AMS_E_HIP; }
    }
    *out = s;
    return AMS_OK;
}

void ams_student_destroy(ams_student* s) { delete s; }

int ams_student_region(const ams_student* s, int32_t region, size_t* offset_bytes, size_t* n_elems) {
    AMS_REQUIRE(s && offset_bytes && n_elems, "region: null pointer");
    const void* p = nullptr;
    size_t n = 0;
    switch (region) {
        case AMS_REGION_PARAMS: p = s->params; n = s->cfg.n_trainable; break;
        case AMS_REGION_STATS: p = s->stats; n = s->cfg.n_stats; break;
        case AMS_REGION_GRADS: p = s->grads; n = s->cfg.n_trainable; break;
        case AMS_REGION_ADAM_M: p = s->adam_m; n = s->cfg.n_trainable; break;
        case AMS_REGION_ADAM_V: p = s->adam_v; n = s->cfg.n_trainable; break;
        case AMS_REGION_FROZEN: p = s->fparams; n = s->cfg.n_trainable; break;
        case AMS_REGION_BN_SYNC: p = s->bn_sync; n = s->bn_sync_doubles; break;
        case AMS_REGION_LOGITS: p = s->logits; n = (size_t)s->cfg.max_batch * s->h * s->w * 32; break;
        default: set_error("region: unknown region %d", region); return AMS_E_INVALID;
    }
    if (!p) { set_error("region %d is not allocated for this student (trainable=%d)", region, s->cfg.trainable); return AMS_E_STATE; }
    *offset_bytes = (size_t)((const char*)p - s->arena);
    *n_elems = n;
    return AMS_OK;
}

int ams_student_lowres_size(const ams_student* s, int32_t* h, int32_t* w) {
    AMS_REQUIRE(s && h && w, "lowres_size: null pointer");
    *h = s->h; *w = s->w;
    return AMS_OK;
}

int ams_student_layer_tensor(const ams_student* s, int32_t layer, int32_t which, size_t* offset_bytes, size_t* n_elems) {
    AMS_REQUIRE(s && offset_bytes && n_elems, "layer_tensor: null pointer");
    AMS_REQUIRE(layer >= 1 && layer <= s->cfg.n_layers && which >= 0 && which <= 3, "layer_tensor: layer %d / which %d out of range", layer, which);
    const LayerRt& l = s->L[layer];
    const float* p = which == 0 ? l.z : which == 1 ? l.a : which == 2 ? l.da : (l.dzp ? l.dzp : l.da);
    if (!p) { set_error("layer_tensor: layer %d has no such tensor (trainable=%d)", layer, s->cfg.trainable); return AMS_E_STATE; }
    *offset_bytes = (size_t)((const char*)p - s->arena);
    *n_elems = (size_t)s->cfg.max_batch * l.px_out * l.d.cout;
    return AMS_OK;
}

int ams_student_freeze(ams_student* s, void* stream) {
    AMS_REQUIRE(s, "freeze: null student");
    hipStream_t st = (hipStream_t)stream;
    RUN(launch_copy(s->fparams, s->params, s->cfg.n_trainable, st));
    RUN(launch_copy(s->fstats, s->stats, s->cfg.n_stats, st));
    for (int i = 1; i <= s->cfg.n_layers; ++i) {
        LayerRt& l = s->L[i];
        if (l.d.bn_eps < 0) continue;
        RUN(launch_bn_fold(s->fparams + l.d.gamma_off, s->fparams + l.d.beta_off, s->fstats + l.d.mean_off, s->fstats + l.d.var_off,
                           s->cfg.bn_eps_frozen, l.d.cout, l.fscale, l.fshift, st));
    }
    for (int i = 1; i + 1 <= s->n_backbone; ++i) {
        LayerRt& l = s->L[i];
        LayerRt& ld = s->L[i + 1];
        if (l.blk_vecs) RUN(launch_block_pack(l.fscale, l.fshift, ld.fscale, ld.fshift, s->fparams + ld.d.w_off, l.d.cout, l.blk_vecs, st));
    }
    if (s->L[1].whi)        // stem: [27][32] -> parts [32][32], k = tap * 3 + channel
        RUN(launch_split_weights3(s->fparams + s->L[1].d.w_off, 32, 1, 27, 32, 32, s->L[1].whi, s->L[1].wlo, s->L[1].wlo3, st));
    if (s->L[1].whf_mem) RUN(launch_split_weights_f16(s->fparams + s->L[1].d.w_off, 32, 1, 27, 32, 32, s->L[1].whf_mem, s->L[1].whf_mem + 32 * 32, st));
    for (int i = 2; i <= s->cfg.n_layers; ++i) {
        LayerRt& l = s->L[i];
        if (!l.whi) continue;
        const int K = l.d.cin - l.split_k0;
        RUN(launch_split_weights3(s->fparams + l.d.w_off + (int64_t)l.split_k0 * l.d.cout, l.d.cout, 1, K, l.d.cout, l.Kp, l.whi, l.wlo,
                                  l.wlo3, st));
        if (l.whf_mem)
            RUN(launch_split_weights_f16(s->fparams + l.d.w_off + (int64_t)l.split_k0 * l.d.cout, l.d.cout, 1, K, l.d.cout, l.Kp, l.whf_mem,
                                         l.whf_mem + (size_t)l.d.cout * l.Kp, st));
    }
    // fp16's range: a weight of 65520 or more has hi = inf, lo = -inf -> NaN logits.  At the other end split1_f16 keeps 22 bits only
    // while hi and lo are normal fp16 numbers (|w| >= 2^-14); below that every part is a multiple of 2^-24 and the pair's error is up to 2^-36
    // absolute, so a layer whose weights ALL lie far below 1 (a legal checkpoint: its BN can scale them back up) would multiply at far worse than
    // f32 level relative to its own scale.  A layer whose largest |w| is below 2^-10 has that floor at <= 2^-26 of its largest weight: below it
    // the layer leaves the fp16 form too (tests/test_f16_split_cpu.py derives the bounds).  Every freeze checks the frozen weights of the
    // layers that hold fp16 panels (one small launch, one 4-byte-per-layer copy, one wait on `stream`: freeze is a phase boundary, not the hot
    // path) and a layer outside the range loses its fp16 form until a later freeze finds it inside again: it runs on three bf16 parts (f32's
    // range) like the fine-tune step.  Activations are not checked: see INTEGRATION.md "Range of the fp16 product form".
    {
        std::vector<WeightRange> jobs;
        std::vector<int> which;
        for (int i = 1; i <= s->cfg.n_layers; ++i) {
            LayerRt& l = s->L[i];
            l.whf = l.whf_mem;
            if (!l.whf_mem) continue;
            // the weights the fp16 panels hold (concat_projection: not the image-pooling rows, which stay f32)
            const int64_t n = i == 1 ? 27 * 32 : (int64_t)(l.d.cin - l.split_k0) * l.d.cout;
            jobs.push_back(WeightRange{s->fparams + l.d.w_off + (int64_t)l.split_k0 * l.d.cout, n});
            which.push_back(i);
        }
        if (!jobs.empty()) {
            std::vector<int> over(jobs.size(), 0);
            RUN(weights_beyond(jobs, 65504.f, 0x1p-10f, reinterpret_cast<int*>(s->tmp_c), over.data(), st));
            s->f16_fallback_layers = 0;
            for (size_t k = 0; k < jobs.size(); ++k)
                if (over[k]) { s->L[which[k]].whf = nullptr; ++s->f16_fallback_layers; }
        }
    }
    s->frozen_ready = true;
    return AMS_OK;
}

// The one body of the four predict entries.  metric: 0 none, 1 when teacher labels come, 2 required; labels: int32, or uint8 when labels_u8
static int student_predict(const char* who, ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode, const uint8_t* teacher_dev,
                           int metric, void* labels_out_dev, int64_t* conf_dev, double* loss_dev, void* stream, int per_frame, int labels_u8) {
    RUN(check_call(s, frames_dev, frames_dtype, batch));
    if (metric == 2) AMS_REQUIRE(teacher_dev && labels_out_dev && conf_dev && loss_dev, "%s: null pointer", who);
    AMS_REQUIRE(labels_out_dev, "%s: null output", who);
    AMS_REQUIRE(teacher_dev == nullptr || (conf_dev && loss_dev), "%s: metrics need conf and loss buffers", who);
    hipStream_t st = (hipStream_t)stream;
    RUN(run_forward(s, frames_dev, frames_dtype, batch, mode, st));
    return launch_upsample_argmax(student_head_call(s, batch, teacher_dev), static_cast<int32_t*>(labels_out_dev), conf_dev, loss_dev, st, per_frame, labels_u8);
}

int ams_student_predict(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode,
                        int32_t* labels_out_dev, void* stream) {
    return student_predict("predict", s, frames_dev, frames_dtype, batch, mode, nullptr, 0, labels_out_dev, nullptr, nullptr, stream, 0, 0);
}

int ams_student_predict_with_metric(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode,
                                    const uint8_t* teacher_dev, int32_t* labels_out_dev, int64_t* conf_mat_dev, double* loss_dev,
                                    void* stream) {
    return student_predict("predict_with_metric", s, frames_dev, frames_dtype, batch, mode, teacher_dev, 2, labels_out_dev, conf_mat_dev, loss_dev, stream, 0, 0);
}

int ams_student_predict_frames(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode, const uint8_t* teacher_dev,
                               int32_t* labels_out_dev, int64_t* conf_mats_dev, double* losses_dev, void* stream) {
    return student_predict("predict_frames", s, frames_dev, frames_dtype, batch, mode, teacher_dev, 1, labels_out_dev, conf_mats_dev, losses_dev, stream, 1, 0);
}

int ams_student_predict_frames_u8(ams_student* s, const void* frames_dev, int32_t frames_dtype, int32_t batch, int32_t mode, const uint8_t* teacher_dev,
                                  uint8_t* labels_out_dev, int64_t* conf_mats_dev, double* losses_dev, void* stream) {
    return student_predict("predict_frames_u8", s, frames_dev, frames_dtype, batch, mode, teacher_dev, 1, labels_out_dev, conf_mats_dev, losses_dev, stream, 1, 1);
}

int ams_student_confidence(ams_student* s, int32_t batch, const uint8_t* teacher_dev, uint8_t* conf_u8, float* conf_f32, int64_t* stats, void* stream) {
    AMS_REQUIRE(s, "confidence: null student");
    AMS_REQUIRE(batch >= 1 && batch <= s->cfg.max_batch, "confidence: batch %d outside 1..%d", batch, s->cfg.max_batch);
    return launch_upsample_confidence(student_head_call(s, batch, teacher_dev), conf_u8, conf_f32, stats, (hipStream_t)stream);
}

int ams_student_soft_metric_layout(ams_student* s, int32_t batch, const uint8_t* teacher_dev, const float* teacher_logits_dev, int32_t th, int32_t tw,
                                   int64_t* stats, float* p_f32, float* ce_f32, void* stream, int32_t layout) {
    AMS_REQUIRE(s, "soft_metric: null student");
    AMS_REQUIRE(batch >= 1 && batch <= s->cfg.max_batch, "soft_metric: batch %d outside 1..%d", batch, s->cfg.max_batch);
    return launch_upsample_soft_metric(student_head_call(s, batch, teacher_dev), LossObjective{teacher_logits_dev, th, tw, layout}, stats, p_f32, ce_f32,
                                       (hipStream_t)stream);
}

int ams_student_soft_metric(ams_student* s, int32_t batch, const uint8_t* teacher_dev, const float* teacher_logits_dev, int32_t th, int32_t tw,
                            int64_t* stats, float* p_f32, float* ce_f32, void* stream) {
    return ams_student_soft_metric_layout(s, batch, teacher_dev, teacher_logits_dev, th, tw, stats, p_f32, ce_f32, stream, AMS_TLOGITS_FULL);
}

// teacher id -> the student's subset index, -1 = ignored
struct StudentLut {
    int32_t lut[256];
    explicit StudentLut(const ams_student* s) {
        for (int i = 0; i < 256; ++i) lut[i] = -1;
        for (int k = 0; k < s->cfg.n_selected; ++k) lut[s->cfg.class_indices[k]] = k;
    }
};

int ams_cross_confusion(const ams_student* s, const uint8_t* labels_dev, int64_t n_pixels, int64_t* conf_mat_dev, void* stream) {
    AMS_REQUIRE(s && labels_dev && conf_mat_dev && n_pixels > 0, "cross_confusion: bad argument");
    return launch_cross_confusion(labels_dev, labels_dev + n_pixels, n_pixels, StudentLut(s).lut, s->cfg.n_selected, conf_mat_dev,
                                  (hipStream_t)stream);
}

int ams_cross_confusion_pairs(const ams_student* s, const uint8_t* label_slots_dev, int64_t label_slot_stride, int32_t capacity, int64_t n_pixels,
                              const int32_t* pairs_dev, const int32_t* pairs_host, int32_t n_pairs, int64_t* conf_mats_dev, void* stream) {
    AMS_REQUIRE(s, "cross_confusion_pairs: null student");
    return launch_cross_confusion_pairs(label_slots_dev, label_slot_stride, capacity, n_pixels, pairs_dev, pairs_host, n_pairs, StudentLut(s).lut,
                                        s->cfg.n_selected, conf_mats_dev, (hipStream_t)stream);
}

int ams_replay_gather(const uint8_t* frame_slots_dev, int64_t frame_slot_stride, const uint8_t* label_slots_dev, int64_t label_slot_stride,
                      int32_t capacity, int32_t src_h, int32_t src_w, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host,
                      int32_t batch, int32_t H, int32_t W, uint8_t* frames_out_dev, uint8_t* labels_out_dev, void* stream) {
    return launch_replay_gather(frame_slots_dev, frame_slot_stride, label_slots_dev, label_slot_stride, capacity, src_h, src_w, samples_dev,
                                samples_host, batch, H, W, frames_out_dev, labels_out_dev, (hipStream_t)stream);
}

int ams_replay_gather_f32(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t th, int32_t tw, int32_t channels,
                          const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int32_t batch, float* out_dev, void* stream) {
    return launch_replay_gather_rows(slots_dev, slot_stride, capacity, th, tw, channels, samples_dev, samples_host, batch, out_dev,
                                     (hipStream_t)stream);
}

int ams_replay_gather_logits(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t src_h, int32_t src_w, int32_t channels,
                             const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int32_t batch, int32_t H, int32_t W,
                             float* out_dev, void* stream) {
    return launch_replay_gather_logits(slots_dev, slot_stride, capacity, src_h, src_w, channels, samples_dev, samples_host, batch, H, W, out_dev,
                                       (hipStream_t)stream);
}

int ams_replay_gather_logits_lowres(const float* slots_dev, int64_t slot_stride, int32_t capacity, int32_t lh, int32_t lw, int32_t channels, int32_t src_h,
                                    int32_t src_w, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int32_t batch, int32_t H,
                                    int32_t W, float* out_dev, void* stream) {
    return launch_replay_gather_logits_lowres(slots_dev, slot_stride, capacity, lh, lw, channels, src_h, src_w, samples_dev, samples_host, batch, H, W,
                                              out_dev, (hipStream_t)stream);
}

int ams_replay_pack_logits(const float* logits_dev, int32_t th, int32_t tw, int32_t num_classes, const int32_t* class_idx_host, int32_t K,
                           int32_t layout, float* slot_dev, void* stream) {
    AMS_REQUIRE(layout == AMS_TLOGITS_FULL || layout == AMS_TLOGITS_SELECTED, "replay_pack_logits: unknown teacher-logit layout %d", layout);
    if (layout == AMS_TLOGITS_FULL) {                              // a full slot is the input itself
        AMS_REQUIRE(logits_dev && slot_dev && th > 0 && tw > 0 && num_classes > 0, "replay_pack_logits: bad argument (%d x %d x %d)", th, tw, num_classes);
        AMS_CHECK_HIP(hipMemcpyAsync(slot_dev, logits_dev, sizeof(float) * (size_t)th * tw * num_classes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return AMS_OK;
    }
    return launch_replay_pack_logits(logits_dev, th, tw, num_classes, class_idx_host, K, slot_dev, (hipStream_t)stream);
}

int ams_teacher_labels_from_logits(const float* logits_dev, int64_t slot_stride, int32_t n, int32_t lh, int32_t lw, int32_t num_classes, int32_t Hs,
                                   int32_t Ws, uint8_t* labels_out_dev, int64_t out_stride, void* stream) {
    return launch_teacher_labels_from_logits(logits_dev, slot_stride, n, lh, lw, num_classes, Hs, Ws, labels_out_dev, out_stride, (hipStream_t)stream);
}

size_t ams_render_table_bytes(void) { return AMS_RENDER_TABLE_BYTES; }

int ams_render_views(const uint8_t* frames_dev, const void* student_dev, int32_t student_dtype, const uint8_t* teacher_dev, int32_t batch, int32_t H,
                     int32_t W, int32_t K, const uint8_t* tables_dev, const ams_render_out* out, void* stream) {
    return launch_render_views(frames_dev, student_dev, student_dtype, teacher_dev, batch, H, W, K, tables_dev, out, (hipStream_t)stream);
}

int ams_student_train_step_dp(ams_student* s, const void* frames_dev, int32_t frames_dtype, const uint8_t* teacher_dev,
                              int32_t batch, int32_t global_batch, float lr, const uint8_t* mask_dev, double* loss_dev,
                              ams_allreduce_cb cb, void* user, void* stream) {
    return train_step_impl(s, frames_dev, frames_dtype, teacher_dev, batch, global_batch, lr, mask_dev, loss_dev, cb, user, nullptr, stream);
}

int ams_student_train_step_rccl(ams_student* s, const void* frames_dev, int32_t frames_dtype, const uint8_t* teacher_dev,
                                int32_t batch, int32_t global_batch, float lr, const uint8_t* mask_dev, double* loss_dev,
                                ams_comm* comm, void* stream) {
    AMS_REQUIRE(comm, "train_step_rccl: null communicator");
    return train_step_impl(s, frames_dev, frames_dtype, teacher_dev, batch, global_batch, lr, mask_dev, loss_dev, nullptr, nullptr, comm, stream);
}

int ams_student_train_step(ams_student* s, const void* frames_dev, int32_t frames_dtype, const uint8_t* teacher_dev, int32_t batch,
                           float lr, const uint8_t* mask_dev, double* loss_dev, void* stream) {
    return train_step_impl(s, frames_dev, frames_dtype, teacher_dev, batch, batch, lr, mask_dev, loss_dev, nullptr, nullptr, nullptr, stream);
}

int ams_student_f16_fallback_layers(const ams_student* s, int32_t* n_layers) {
    AMS_REQUIRE(s && n_layers, "f16_fallback_layers: null pointer");
    *n_layers = s->f16_fallback_layers;
    return AMS_OK;
}

int ams_student_feed_teacher_logits_layout(ams_student* s, const float* teacher_logits_dev, int32_t th, int32_t tw, int32_t layout) {
    AMS_REQUIRE(s, "feed_teacher_logits: null student");
    AMS_REQUIRE(tlogits_layout_ok(layout), "feed_teacher_logits: unknown teacher-logit layout %d", layout);
    LossObjective& o = s->loss_objective;
    if (!teacher_logits_dev) { o.teacher_logits = nullptr; o.th = o.tw = 0; o.layout = AMS_TLOGITS_FULL; return AMS_OK; }
    AMS_REQUIRE(th >= 1 && tw >= 1 && th <= s->cfg.height && tw <= s->cfg.width, "feed_teacher_logits: %d x %d teacher logits for %d x %d labels", th, tw,
                s->cfg.height, s->cfg.width);
    o.teacher_logits = teacher_logits_dev; o.th = th; o.tw = tw; o.layout = layout;
    return AMS_OK;
}

int ams_student_feed_teacher_logits(ams_student* s, const float* teacher_logits_dev, int32_t th, int32_t tw) {
    return ams_student_feed_teacher_logits_layout(s, teacher_logits_dev, th, tw, AMS_TLOGITS_FULL);
}

int ams_student_set_regularizer(ams_student* s, const uint8_t* reg_mask_dev, int32_t n_vars, float coef) {
    AMS_REQUIRE(s, "set_regularizer: null student");
    if (!reg_mask_dev) { s->reg_mask = nullptr; s->reg_nvars = 0; s->reg_coef = 0.f; return AMS_OK; }
    AMS_REQUIRE(s->cfg.trainable, "set_regularizer: this student was created frozen");
    AMS_REQUIRE(n_vars > 0 && coef >= 0.f, "set_regularizer: n_vars=%d coef=%g", n_vars, (double)coef);
    s->reg_mask = reg_mask_dev; s->reg_nvars = n_vars; s->reg_coef = coef;
    return AMS_OK;
}

int ams_student_set_kd(ams_student* s, float temperature, float alpha) {
    AMS_REQUIRE(s, "set_kd: null student");
    AMS_REQUIRE(s->cfg.trainable, "set_kd: this student was created frozen");
    RUN(kd_params_check("set_kd", temperature, alpha));
    s->loss_objective.temperature = temperature; s->loss_objective.alpha = alpha;
    return AMS_OK;
}

int ams_student_set_loss_weights(ams_student* s, const float* class_weights_host, int32_t n, float conf_gamma) {
    AMS_REQUIRE(s, "set_loss_weights: null student");
    AMS_REQUIRE(s->cfg.trainable, "set_loss_weights: this student was created frozen");
    AMS_REQUIRE(!class_weights_host || n == s->cfg.n_selected, "set_loss_weights: %d class weights for %d selected classes", n, s->cfg.n_selected);
    RUN(loss_weights_check("set_loss_weights", class_weights_host, n, s->cfg.n_selected, conf_gamma));
    for (int k = 0; k < n && class_weights_host; ++k) s->loss_cw[k] = class_weights_host[k];
    s->loss_objective.class_weights = class_weights_host ? s->loss_cw : nullptr;
    s->loss_objective.conf_gamma = conf_gamma;
    return AMS_OK;
}

int ams_student_set_loss_mining(ams_student* s, float top_k, void* scratch_dev, size_t scratch_bytes) {
    AMS_REQUIRE(s, "set_loss_mining: null student");
    AMS_REQUIRE(s->cfg.trainable, "set_loss_mining: this student was created frozen");
    RUN(mining_top_k_check("set_loss_mining", top_k));
    if (top_k < 1.f) {
        const ams_student_config& c = s->cfg;
        AMS_REQUIRE(ce_loss_grad_supported(s->w, c.width), "set_loss_mining: %d output columns on %d logit columns is outside the one-pass loss kernel", c.width, s->w);
        const size_t need = loss_mining_scratch(c.max_batch, c.height, c.width);
        AMS_REQUIRE(scratch_dev && ((uintptr_t)scratch_dev & 15) == 0 && scratch_bytes >= need,
                    "set_loss_mining: scratch NULL, misaligned or too small (need %zu bytes, 16-byte aligned)", need);
    }
    s->mining_top_k = top_k;
    if (scratch_dev != s->mining_scratch) s->mining_ran = false;       // another block: nothing of a mined step in it yet
    s->mining_scratch = scratch_dev;
    return AMS_OK;
}

int ams_student_mining_result(ams_student* s, ams_mining_result* out_host, void* stream) {
    AMS_REQUIRE(s && out_host, "mining_result: null pointer");
    if (!s->mining_ran || !s->mining_scratch) { set_error("mining_result: no mined step has run (ams_student_set_loss_mining with top_k < 1)"); return AMS_E_STATE; }
    const MiningBuffers m = loss_mining_buffers(s->mining_scratch, s->cfg.max_batch, s->cfg.height, s->cfg.width);
    AMS_CHECK_HIP(hipMemcpyAsync(out_host, m.result, sizeof(ams_mining_result), hipMemcpyDeviceToHost, (hipStream_t)stream));
    AMS_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return AMS_OK;
}

int ams_student_set_option(ams_student* s, int32_t option, int32_t value) {
    AMS_REQUIRE(s, "set_option: null student");
    s->dual_choice.clear();                            // any option may change the plans the autotune compared
    if (option == AMS_OPT_MATMUL) {
        AMS_REQUIRE(value == AMS_MATMUL_F32 || value == AMS_MATMUL_SPLIT_BF16 || value == AMS_MATMUL_SPLIT_BF16_X6 || value == AMS_MATMUL_BF16 ||
                        value == AMS_MATMUL_SPLIT_F16,
                    "set_option: unknown matmul mode %d", value);
        s->matmul_mode = value;
        return AMS_OK;
    }
    if (option == AMS_OPT_DUAL_AUTOTUNE) {
        s->dual_autotune = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_DUAL_PARTS) {
        AMS_REQUIRE(value >= 2 && value <= 4, "set_option: AMS_OPT_DUAL_PARTS must be 2 .. 4");
        s->dual_parts = value;
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_FIRST_BLOCK) {
        s->fuse_first_block = value < 0 ? 0 : (value > 2 ? 2 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_DW_PROJECT) {
        s->fuse_dw_project = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_EXPAND_DW_STREAM) {
        s->fuse_expand_dw_stream = value < 0 ? 0 : (value > 2 ? 2 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_BLOCK_X6) {
        s->block_x6 = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_LATE_SUBBATCH) {
        s->late_subbatch = value < 0 ? 0 : value;
        return AMS_OK;
    }
    if (option == AMS_OPT_DUAL_STREAM) {
        s->dual_stream = value < 0 ? 0 : value;
        s->dual_choice.clear();
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_BLOCK) {
        s->fuse_block = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_EXPAND_DW) {
        s->fuse_expand_dw = value < 0 ? 0 : (value > 2 ? 2 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_EMULATE_BF16_STORAGE) {
        s->emulate_bf16_storage = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_DGRAD_BN) {
        s->fuse_dgrad_bn = value < 0 ? 0 : (value > 3 ? 3 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_GEMM_RED) {
        s->fuse_gemm_red = value & 3;
        return AMS_OK;
    }
    if (option == AMS_OPT_TRAIN_RECOMPUTE) {
        s->train_recompute = value < 0 ? 0 : (value > 2 ? 2 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_OPERAND_BN) {
        s->fuse_operand_bn = value & 1;
        return AMS_OK;
    }
    if (option == AMS_OPT_WGRAD_FORK_EVERY) {
        AMS_REQUIRE(value >= 1 && value <= 64, "set_option: AMS_OPT_WGRAD_FORK_EVERY must be in 1 .. 64");
        s->wgrad_fork_every = value;
        return AMS_OK;
    }
    if (option == AMS_OPT_TRAIN_FWD_F16) {
        s->train_fwd_f16 = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_SOFT_TEACHER) {
        s->loss_objective.soft_teacher = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_NAN_GRADS) {
        s->nan_grads = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_OVERLAP_WGRAD) {
        s->overlap_wgrad = value < 0 ? 0 : (value > 3 ? 3 : value);
        return AMS_OK;
    }
    if (option == AMS_OPT_OVERLAP_HEAD) {
        s->overlap_head = value != 0;
        return AMS_OK;
    }
    if (option == AMS_OPT_FUSE_HEAD) {
        s->fuse_head = value < 0 ? 0 : value & 3;
        return AMS_OK;
    }
    if (option == AMS_OPT_STREAM_MIN_ROWS) {
        AMS_REQUIRE(value >= 0, "set_option: AMS_OPT_STREAM_MIN_ROWS must be >= 0");
        s->stream_min_rows = value;
        return AMS_OK;
    }
    set_error("set_option: unknown option %d", option);
    return AMS_E_INVALID;
}

int ams_student_profile(ams_student* s, int32_t enable) {
    AMS_REQUIRE(s, "profile: null student");
    AMS_CHECK_HIP(hipDeviceSynchronize());
    s->prof.clear();
    s->prof.on = enable != 0;
    return AMS_OK;
}

int ams_student_profile_read(ams_student* s, char* buf, size_t cap, size_t* needed) {
    AMS_REQUIRE(s && needed, "profile_read: null pointer");
    AMS_CHECK_HIP(hipDeviceSynchronize());
    std::string out;
    char line[256];
    for (auto& r : s->prof.recs) {
        float ms = 0.f;
        AMS_CHECK_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        snprintf(line, sizeof(line), "%s\t%d\t%.6f\t%.0f\t%.0f\t%.0f\n", r.name.c_str(), r.layer, ms, r.bytes, r.flops, r.flops_x6);
        out += line;
    }
    *needed = out.size() + 1;
    if (buf && cap >= out.size() + 1) memcpy(buf, out.c_str(), out.size() + 1);
    return AMS_OK;
}

int ams_student_get_adam_step(const ams_student* s, int64_t* t) {
    AMS_REQUIRE(s && t, "get_adam_step: null pointer");
    *t = s->adam_t;
    return AMS_OK;
}
int ams_student_set_adam_step(ams_student* s, int64_t t) {
    AMS_REQUIRE(s && t >= 0, "set_adam_step: bad argument");
    s->adam_t = t;
    return AMS_OK;
}

size_t ams_pack_masked_fp16_scratch(int64_t n) { return n > 0 ? pack_fp16_scratch(n) : 0; }

int ams_pack_masked_fp16(const float* params_dev, const uint8_t* mask_dev, int64_t n, uint16_t* out_half_dev, int64_t* n_out_dev,
                         int64_t* scratch_dev, size_t scratch_elems, void* stream) {
    AMS_REQUIRE(params_dev && out_half_dev && n_out_dev && n > 0, "pack_masked_fp16: bad argument");
    AMS_REQUIRE(scratch_dev && scratch_elems >= pack_fp16_scratch(n), "pack_masked_fp16: scratch too small (need %zu int64)",
                pack_fp16_scratch(n));
    return launch_pack_fp16(params_dev, mask_dev, n, out_half_dev, n_out_dev, scratch_dev, (hipStream_t)stream);
}

// mask section of a descriptor table, or -1 if the table does not describe contiguous masks inside the arena (reason in the error)
static int64_t delta_mask_bytes(const ams_student* s, const ams_delta_var* vars, int32_t n_vars, const char* what = "apply_delta") {
    if (!vars || n_vars < 1 || n_vars > AMS_DELTA_MAX_VARS) { set_error("%s: %d variables (1 .. %d)", what, n_vars, AMS_DELTA_MAX_VARS); return -1; }
    int64_t mask = 0;
    for (int32_t i = 0; i < n_vars; ++i) {
        const ams_delta_var& d = vars[i];
        const int64_t n_region = d.region == AMS_REGION_PARAMS ? (int64_t)s->cfg.n_trainable : d.region == AMS_REGION_STATS ? (int64_t)s->cfg.n_stats : -1;
        if (n_region < 0) { set_error("%s: variable %d: region %d is neither params nor stats", what, i, d.region); return -1; }
        if (d.offset < 0 || d.count < 0 || d.offset > n_region - d.count) {
            set_error("%s: variable %d: elements [%lld, +%lld) outside its region of %lld", what, i, (long long)d.offset, (long long)d.count,
                      (long long)n_region);
            return -1;
        }
        if (d.mask_offset != mask) {
            set_error("%s: variable %d: mask at byte %lld, the masks before it end at %lld", what, i, (long long)d.mask_offset, (long long)mask);
            return -1;
        }
        mask += (d.count + 7) / 8;
    }
    return mask;
}

// the mask section of a delta over these variables, in bytes: one bit per element, each variable on a byte of its own; -1: no such table
static int64_t delta_mask_sum(const ams_delta_var* vars_host, int32_t n_vars) {
    if (!vars_host || n_vars < 1 || n_vars > AMS_DELTA_MAX_VARS) return -1;
    int64_t mask = 0;
    for (int32_t i = 0; i < n_vars; ++i) mask += vars_host[i].count > 0 ? (vars_host[i].count + 7) / 8 : 0;
    return mask;
}

size_t ams_student_apply_delta_scratch(const ams_delta_var* vars_host, int32_t n_vars) {
    const int64_t mask = delta_mask_sum(vars_host, n_vars);
    return mask < 0 ? 0 : (size_t)(4 * (int64_t)n_vars + delta_segments(mask));
}

int ams_student_apply_delta(ams_student* s, const uint8_t* payload_dev, int64_t payload_bytes, const ams_delta_var* vars_host,
                            int32_t n_vars, int64_t* n_applied_dev, int32_t* status_dev, int64_t* scratch_dev, size_t scratch_elems,
                            void* stream) {
    AMS_REQUIRE(s && n_applied_dev && status_dev && scratch_dev, "apply_delta: null pointer");
    AMS_REQUIRE(payload_bytes >= 0 && (payload_dev || payload_bytes == 0), "apply_delta: %lld payload bytes at %p", (long long)payload_bytes,
                (const void*)payload_dev);
    static_assert(sizeof(ams_delta_var) == 4 * sizeof(int64_t), "ams_delta_var: four int64 words");
    const int64_t mask_bytes = delta_mask_bytes(s, vars_host, n_vars);
    if (mask_bytes < 0) return AMS_E_INVALID;
    const size_t need = 4 * (size_t)n_vars + (size_t)delta_segments(mask_bytes);
    AMS_REQUIRE(scratch_elems >= need, "apply_delta: scratch too small (need %zu int64)", need);
    hipStream_t st = (hipStream_t)stream;
    // the table travels from a host copy the handle keeps until the upload has read it (no synchronisation on the stream's earlier work)
    if (s->ev_delta) AMS_CHECK_HIP(hipEventSynchronize(s->ev_delta));
    else RUN(create_sync_event(&s->ev_delta));
    s->delta_vars.assign(vars_host, vars_host + n_vars);
    ams_delta_var* vars_dev = reinterpret_cast<ams_delta_var*>(scratch_dev);
    AMS_CHECK_HIP(hipMemcpyAsync(vars_dev, s->delta_vars.data(), n_vars * sizeof(ams_delta_var), hipMemcpyHostToDevice, st));
    AMS_CHECK_HIP(hipEventRecord(s->ev_delta, st));
    return launch_apply_delta(payload_dev, payload_bytes, vars_dev, n_vars, mask_bytes, s->params, (int64_t)s->cfg.n_trainable, s->stats,
                              (int64_t)s->cfg.n_stats, scratch_dev + 4 * n_vars, n_applied_dev, status_dev, st);
}

size_t ams_select_changed_scratch(int64_t n) { return n > 0 ? select_scratch() : 0; }

int ams_select_changed(const float* after_dev, const float* before_dev, int64_t n, int64_t k, ams_select_result* result_dev,
                       int64_t* scratch_dev, size_t scratch_elems, void* stream) {
    AMS_REQUIRE(after_dev && before_dev && result_dev && scratch_dev, "select_changed: null pointer");
    AMS_REQUIRE(n > 0 && n < ((int64_t)1 << 31) && k >= 0 && k < n, "select_changed: rank %lld of %lld elements (0 <= k < n < 2^31)", (long long)k,
                (long long)n);
    AMS_REQUIRE(((uintptr_t)result_dev & 7) == 0 && ((uintptr_t)after_dev & 3) == 0 && ((uintptr_t)before_dev & 3) == 0, "select_changed: misaligned pointer");
    AMS_REQUIRE(scratch_elems >= select_scratch(), "select_changed: scratch too small (need %zu int64)", select_scratch());
    return launch_select_changed(after_dev, before_dev, n, k, result_dev, scratch_dev, (hipStream_t)stream);
}

int ams_select_apply(float* params_dev, const float* before_dev, int64_t n, float cut, uint8_t* mask_dev, int64_t* n_kept_dev, void* stream) {
    AMS_REQUIRE(params_dev && before_dev && mask_dev && n_kept_dev && n > 0, "select_apply: bad argument");
    AMS_REQUIRE(((uintptr_t)n_kept_dev & 7) == 0 && ((uintptr_t)params_dev & 3) == 0 && ((uintptr_t)before_dev & 3) == 0, "select_apply: misaligned pointer");
    return launch_select_apply(params_dev, before_dev, n, cut, mask_dev, n_kept_dev, (hipStream_t)stream);
}

size_t ams_student_encode_delta_scratch(const ams_delta_var* vars_host, int32_t n_vars) {
    const int64_t mask = delta_mask_sum(vars_host, n_vars);
    return mask < 0 ? 0 : (size_t)(5 * (int64_t)n_vars + 2 + encode_segments(mask));
}

int ams_student_encode_delta(ams_student* s, const uint8_t* mask_dev, const ams_delta_var* vars_host, int32_t n_vars, uint8_t* payload_dev,
                             int64_t payload_cap, int64_t* payload_bytes_dev, int64_t* scratch_dev, size_t scratch_elems, void* stream) {
    AMS_REQUIRE(s && payload_dev && payload_bytes_dev && scratch_dev, "encode_delta: null pointer");
    const int64_t mask_bytes = delta_mask_bytes(s, vars_host, n_vars, "encode_delta");
    if (mask_bytes < 0) return AMS_E_INVALID;
    AMS_REQUIRE(payload_cap >= mask_bytes, "encode_delta: room for %lld bytes, the mask section alone has %lld", (long long)payload_cap,
                (long long)mask_bytes);
    const size_t table = 5 * (size_t)n_vars + 1;
    const size_t need = table + 1 + (size_t)encode_segments(mask_bytes);
    AMS_REQUIRE(scratch_elems >= need, "encode_delta: scratch too small (need %zu int64)", need);
    hipStream_t st = (hipStream_t)stream;
    // as in apply_delta: the table (descriptors, then each variable's first element in layout order) travels from a host copy the handle keeps
    if (s->ev_encode) AMS_CHECK_HIP(hipEventSynchronize(s->ev_encode));
    else RUN(create_sync_event(&s->ev_encode));
    s->encode_table.resize(table);
    memcpy(s->encode_table.data(), vars_host, n_vars * sizeof(ams_delta_var));
    int64_t first = 0;
    for (int32_t i = 0; i < n_vars; ++i) { s->encode_table[4 * (size_t)n_vars + i] = first; first += vars_host[i].count; }
    s->encode_table[table - 1] = first;
    AMS_CHECK_HIP(hipMemcpyAsync(scratch_dev, s->encode_table.data(), table * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AMS_CHECK_HIP(hipEventRecord(s->ev_encode, st));
    return launch_encode_delta(mask_dev, scratch_dev, n_vars, mask_bytes, s->params, s->stats, scratch_dev + table, payload_dev, payload_cap,
                               payload_bytes_dev, st);
}

// ---- the q8 delta (k_delta_q8.hip) ---------------------------------------------------------------------------
// What a q8 call can tell about its table without the handle: the variable count, the regions, the signs and the contiguous masks.
// -> the mask section in bytes (has_stats: an entry lies in AMS_REGION_STATS), or -1 with the reason in the error.  The bounds inside
// the arena are delta_mask_bytes' business, once the handle is known to be there.
static int64_t delta_table_shape(const ams_delta_var* vars, int32_t n_vars, const char* what, bool* has_stats) {
    if (!vars || n_vars < 1 || n_vars > AMS_DELTA_MAX_VARS) { set_error("%s: malformed table: %d variables (1 .. %d)", what, n_vars, AMS_DELTA_MAX_VARS); return -1; }
    int64_t mask = 0;
    *has_stats = false;
    for (int32_t i = 0; i < n_vars; ++i) {
        const ams_delta_var& d = vars[i];
        if (d.region != AMS_REGION_PARAMS && d.region != AMS_REGION_STATS) {
            set_error("%s: malformed table: variable %d: region %d is neither params nor stats", what, i, d.region);
            return -1;
        }
        if (d.offset < 0 || d.count < 0 || d.count > ((int64_t)1 << 40)) {
            set_error("%s: malformed table: variable %d: elements [%lld, +%lld)", what, i, (long long)d.offset, (long long)d.count);
            return -1;
        }
        if (d.mask_offset != mask) {
            set_error("%s: malformed table: variable %d: mask at byte %lld, the masks before it end at %lld", what, i, (long long)d.mask_offset,
                      (long long)mask);
            return -1;
        }
        *has_stats = *has_stats || d.region == AMS_REGION_STATS;
        mask += (d.count + 7) / 8;
    }
    return mask;
}

size_t ams_student_encode_delta_q8_scratch(const ams_delta_var* vars_host, int32_t n_vars) {
    const int64_t mask = delta_mask_sum(vars_host, n_vars);
    return mask < 0 ? 0 : q8_encode_table_words(n_vars) + 1 + (size_t)delta_segments(mask);
}

// Order of refusal: null pointers; advance_base; the table's shape; the statistics' base; the scratch; the room; and only then the handle and
// the table against its arena — so everything before it can be asked without a student.
int ams_student_encode_delta_q8(ams_student* s, const uint8_t* mask_dev, const ams_delta_var* vars_host, int32_t n_vars, float* base_params_dev,
                                float* base_stats_dev, int32_t advance_base, uint8_t* payload_dev, int64_t payload_cap, int64_t* payload_bytes_dev,
                                int32_t* status_dev, int64_t* scratch_dev, size_t scratch_elems, void* stream) {
    AMS_REQUIRE(base_params_dev && payload_dev && payload_bytes_dev && status_dev && scratch_dev, "encode_delta_q8: null pointer");
    AMS_REQUIRE(advance_base == 0 || advance_base == 1, "encode_delta_q8: advance_base %d (0 or 1)", advance_base);
    bool has_stats = false;
    const int64_t shape = delta_table_shape(vars_host, n_vars, "encode_delta_q8", &has_stats);
    if (shape < 0) return AMS_E_INVALID;
    AMS_REQUIRE(base_stats_dev || !has_stats, "encode_delta_q8: null statistics base, and the table has variables in AMS_REGION_STATS");
    const size_t table = q8_encode_table_words(n_vars);
    const size_t need = table + 1 + (size_t)delta_segments(shape);
    AMS_REQUIRE(scratch_elems >= need, "encode_delta_q8: scratch too small (need %zu int64)", need);
    AMS_REQUIRE(payload_cap >= shape + 4 * (int64_t)n_vars, "encode_delta_q8: room for %lld bytes, the mask and scale sections alone have %lld",
                (long long)payload_cap, (long long)(shape + 4 * (int64_t)n_vars));
    AMS_REQUIRE(s, "encode_delta_q8: null handle");
    const int64_t mask_bytes = delta_mask_bytes(s, vars_host, n_vars, "encode_delta_q8");
    if (mask_bytes < 0) return AMS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    // as in encode_delta: the table travels from a host copy the handle keeps; its tail, the per-variable maxima, travels as zeros
    if (s->ev_encode) AMS_CHECK_HIP(hipEventSynchronize(s->ev_encode));
    else RUN(create_sync_event(&s->ev_encode));
    s->encode_table.assign(table, 0);
    memcpy(s->encode_table.data(), vars_host, n_vars * sizeof(ams_delta_var));
    int64_t first = 0;
    for (int32_t i = 0; i < n_vars; ++i) { s->encode_table[4 * (size_t)n_vars + i] = first; first += vars_host[i].count; }
    s->encode_table[5 * (size_t)n_vars] = first;
    AMS_CHECK_HIP(hipMemcpyAsync(scratch_dev, s->encode_table.data(), table * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AMS_CHECK_HIP(hipEventRecord(s->ev_encode, st));
    return launch_encode_delta_q8(mask_dev, scratch_dev, n_vars, mask_bytes, s->params, s->stats, base_params_dev, base_stats_dev, advance_base,
                                  scratch_dev + table, payload_dev, payload_cap, payload_bytes_dev, status_dev, st);
}

size_t ams_student_apply_delta_q8_scratch(const ams_delta_var* vars_host, int32_t n_vars) {
    return ams_student_apply_delta_scratch(vars_host, n_vars);
}

int ams_student_apply_delta_q8(ams_student* s, const uint8_t* payload_dev, int64_t payload_bytes, const ams_delta_var* vars_host, int32_t n_vars,
                               int64_t* n_applied_dev, int32_t* status_dev, int64_t* scratch_dev, size_t scratch_elems, void* stream) {
    AMS_REQUIRE(n_applied_dev && status_dev && scratch_dev, "apply_delta_q8: null pointer");
    AMS_REQUIRE(payload_bytes >= 0 && (payload_dev || payload_bytes == 0), "apply_delta_q8: %lld payload bytes at %p", (long long)payload_bytes,
                (const void*)payload_dev);
    bool has_stats = false;
    const int64_t shape = delta_table_shape(vars_host, n_vars, "apply_delta_q8", &has_stats);
    if (shape < 0) return AMS_E_INVALID;
    const size_t need = 4 * (size_t)n_vars + (size_t)delta_segments(shape);
    AMS_REQUIRE(scratch_elems >= need, "apply_delta_q8: scratch too small (need %zu int64)", need);
    AMS_REQUIRE(s, "apply_delta_q8: null handle");
    const int64_t mask_bytes = delta_mask_bytes(s, vars_host, n_vars, "apply_delta_q8");
    if (mask_bytes < 0) return AMS_E_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (s->ev_delta) AMS_CHECK_HIP(hipEventSynchronize(s->ev_delta));
    else RUN(create_sync_event(&s->ev_delta));
    s->delta_vars.assign(vars_host, vars_host + n_vars);
    ams_delta_var* vars_dev = reinterpret_cast<ams_delta_var*>(scratch_dev);
    AMS_CHECK_HIP(hipMemcpyAsync(vars_dev, s->delta_vars.data(), n_vars * sizeof(ams_delta_var), hipMemcpyHostToDevice, st));
    AMS_CHECK_HIP(hipEventRecord(s->ev_delta, st));
    return launch_apply_delta_q8(payload_dev, payload_bytes, vars_dev, n_vars, mask_bytes, s->params, (int64_t)s->cfg.n_trainable, s->stats,
                                 (int64_t)s->cfg.n_stats, scratch_dev + 4 * n_vars, n_applied_dev, status_dev, st);
}

// ---- the uplink frame codec (k_uplink.hip) ------------------------------------------------------------------
// One description for the entries of both payload kinds, refused in entry_check's order; then what only some of them take (a negative byte
// count).  need = the entry's scratch bytes for a size the shape rule accepts.
static int uplink_entry(const char* who, int32_t H, int32_t W, bool q_ok, int32_t q, const void* scratch, size_t have, size_t (*need)(int, int),
                        bool ptrs) {
    EntryCall c;
    c.who = who;
    c.describe("%d x %d, q=%d", H, W, q);
    c.sizes = H > 0 && W > 0;
    c.shape = uplink_shape_ok(H, W) && q_ok;
    c.scratch_what = "scratch";
    c.scratch = scratch;
    c.have = have;
    if (c.shaped()) c.need = need(H, W);
    c.ptrs = ptrs;
    RUN_RC(entry_check(c));
    AMS_REQUIRE(((uintptr_t)scratch & 15) == 0, "%s: scratch at %p is not 16-byte aligned", who, scratch);
    return AMS_OK;
}

int64_t ams_uplink_max_bytes(int32_t H, int32_t W) { return uplink_shape_ok(H, W) ? uplink_max_bytes(H, W) : 0; }
size_t ams_uplink_encode_scratch(int32_t H, int32_t W) { return AMS_ENTRY_SCRATCH(uplink_shape_ok(H, W), uplink_encode_scratch_bytes(H, W)); }
size_t ams_uplink_decode_scratch(int32_t H, int32_t W) { return AMS_ENTRY_SCRATCH(uplink_shape_ok(H, W), uplink_decode_scratch_bytes(H, W)); }

int ams_uplink_transform(const uint8_t* frame_dev, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes, void* stream) {
    RUN_RC(uplink_entry("uplink_transform", H, W, true, 0, scratch_dev, scratch_bytes, uplink_encode_scratch_bytes, frame_dev != nullptr));
    return launch_uplink_transform(frame_dev, H, W, scratch_dev, (hipStream_t)stream);
}

int ams_uplink_size_table(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int64_t* sizes_dev, void* stream) {
    RUN_RC(uplink_entry("uplink_size_table", H, W, true, 0, scratch_dev, scratch_bytes, uplink_encode_scratch_bytes, sizes_dev != nullptr));
    return launch_uplink_size_table(scratch_dev, H, W, sizes_dev, (hipStream_t)stream);
}

int ams_uplink_encode(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int32_t q, uint8_t* payload_dev, int64_t payload_cap,
                      int64_t* bytes_dev, int32_t* status_dev, void* stream) {
    RUN_RC(uplink_entry("uplink_encode", H, W, q >= 1 && q <= 100, q, scratch_dev, scratch_bytes, uplink_encode_scratch_bytes,
                        payload_dev && bytes_dev && status_dev));
    AMS_REQUIRE(payload_cap >= 0, "uplink_encode: room for %lld bytes", (long long)payload_cap);
    return launch_uplink_encode(scratch_dev, H, W, q, payload_dev, payload_cap, bytes_dev, status_dev, (hipStream_t)stream);
}

int ams_uplink_decode(const uint8_t* payload_dev, int64_t payload_bytes, int32_t H, int32_t W, uint8_t* frame_out_dev, int32_t* status_dev,
                      void* scratch_dev, size_t scratch_bytes, void* stream) {
    RUN_RC(uplink_entry("uplink_decode", H, W, true, 0, scratch_dev, scratch_bytes, uplink_decode_scratch_bytes,
                        frame_out_dev && status_dev && (payload_dev || payload_bytes <= 0)));
    AMS_REQUIRE(payload_bytes >= 0, "uplink_decode: %lld payload bytes", (long long)payload_bytes);
    return launch_uplink_decode(payload_dev, payload_bytes, H, W, frame_out_dev, status_dev, scratch_dev, (hipStream_t)stream);
}

// ---- the predicted frame AUP1 (k_uplink_inter.hip): the same description; the reference stands with the other pointers
int64_t ams_uplink_inter_max_bytes(int32_t H, int32_t W) { return uplink_shape_ok(H, W) ? uplink_inter_max_bytes(H, W) : 0; }
size_t ams_uplink_inter_encode_scratch(int32_t H, int32_t W) {
    return AMS_ENTRY_SCRATCH(uplink_shape_ok(H, W), uplink_inter_encode_scratch_bytes(H, W));
}
size_t ams_uplink_inter_decode_scratch(int32_t H, int32_t W) {
    return AMS_ENTRY_SCRATCH(uplink_shape_ok(H, W), uplink_inter_decode_scratch_bytes(H, W));
}

int ams_uplink_inter_transform(const uint8_t* frame_dev, const uint8_t* ref_dev, int32_t H, int32_t W, void* scratch_dev, size_t scratch_bytes,
                               void* stream) {
    RUN_RC(uplink_entry("uplink_inter_transform", H, W, true, 0, scratch_dev, scratch_bytes, uplink_inter_encode_scratch_bytes, frame_dev && ref_dev));
    return launch_uplink_inter_transform(frame_dev, ref_dev, H, W, scratch_dev, (hipStream_t)stream);
}

int ams_uplink_inter_size_table(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int64_t* sizes_dev, void* stream) {
    RUN_RC(uplink_entry("uplink_inter_size_table", H, W, true, 0, scratch_dev, scratch_bytes, uplink_inter_encode_scratch_bytes, sizes_dev != nullptr));
    return launch_uplink_inter_size_table(scratch_dev, H, W, sizes_dev, (hipStream_t)stream);
}

int ams_uplink_inter_encode(void* scratch_dev, size_t scratch_bytes, int32_t H, int32_t W, int32_t q, uint8_t* payload_dev, int64_t payload_cap,
                            int64_t* bytes_dev, int32_t* status_dev, void* stream) {
    RUN_RC(uplink_entry("uplink_inter_encode", H, W, q >= 1 && q <= 100, q, scratch_dev, scratch_bytes, uplink_inter_encode_scratch_bytes,
                        payload_dev && bytes_dev && status_dev));
    AMS_REQUIRE(payload_cap >= 0, "uplink_inter_encode: room for %lld bytes", (long long)payload_cap);
    return launch_uplink_inter_encode(scratch_dev, H, W, q, payload_dev, payload_cap, bytes_dev, status_dev, (hipStream_t)stream);
}

int ams_uplink_inter_decode(const uint8_t* payload_dev, int64_t payload_bytes, const uint8_t* ref_dev, int32_t H, int32_t W, uint8_t* frame_out_dev,
                            int32_t* status_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    RUN_RC(uplink_entry("uplink_inter_decode", H, W, true, 0, scratch_dev, scratch_bytes, uplink_inter_decode_scratch_bytes,
                        ref_dev && frame_out_dev && status_dev && (payload_dev || payload_bytes <= 0)));
    AMS_REQUIRE(payload_bytes >= 0, "uplink_inter_decode: %lld payload bytes", (long long)payload_bytes);
    return launch_uplink_inter_decode(payload_dev, payload_bytes, ref_dev, H, W, frame_out_dev, status_dev, scratch_dev, (hipStream_t)stream);
}

// ---- kernel-level entry points -----------------------------------------------------------------------------
// The GEMM, depthwise / stem and recompute entries describe their call to entry_check (entry_check.hpp) and launch nothing before it has
// passed: no pixels or rows; the shape rule; scratch or panels; scale without shift; null pointers.  The launchers keep their own checks.
static bool sizes3(int B, int H, int W) { return B > 0 && H > 0 && W > 0; }

int ams_k_stem_conv(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, const float* w, int32_t cout,
                    const float* scale, const float* shift, int32_t act, float pixel_scale, float* y, void* stream) {
    EntryCall c;
    c.who = "stem_conv";
    c.describe("B=%d, %d x %d, cout=%d, dtype=%d", B, H, W, cout, frames_dtype);
    c.sizes = sizes3(B, H, W) && cout > 0;
    c.shape = cout % 8 == 0 && cout <= 256 && frame_dtype_ok(frames_dtype);
    c.scale_without_shift = scale && !shift;
    c.ptrs = frames && w && y;
    RUN(entry_check(c));
    return launch_stem(frames, frames_dtype, B, H, W, w, cout, scale, shift, act, pixel_scale, y, (hipStream_t)stream);
}

// the depthwise entries: B, H, W, C > 0; C % 4 == 0 and <= 1024, stride 1 | 2, rate 1 | 2, not both 2
static EntryCall dw_entry(const char* who, int B, int H, int W, int C, int stride, int rate) {
    EntryCall c;
    c.who = who;
    c.describe("B=%d, %d x %d, C=%d, stride=%d, rate=%d", B, H, W, C, stride, rate);
    c.sizes = sizes3(B, H, W) && C > 0;
    c.shape = dw_entry_shape(C, stride, rate);
    return c;
}

int ams_k_depthwise3x3(const float* x, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t stride, int32_t rate,
                       const float* scale, const float* shift, int32_t act, float* y, void* stream) {
    EntryCall c = dw_entry("depthwise3x3", B, H, W, C, stride, rate);
    c.scale_without_shift = scale && !shift;
    c.ptrs = x && w && y;
    RUN(entry_check(c));
    return launch_depthwise(x, B, H, W, C, w, stride, rate, scale, shift, act, y, (hipStream_t)stream);
}

// the forward GEMM entries: M, K, N > 0; k_mult divides K (4: exact f32, 8: the part kernels)
static EntryCall pw_entry(const char* who, int64_t M, int K, int N, int k_mult) {
    EntryCall c;
    c.who = who;
    c.describe("M=%lld K=%d N=%d", (long long)M, K, N);
    c.sizes = M > 0 && K > 0 && N > 0;
    c.shape = K % k_mult == 0;
    return c;
}
static void pw_entry_panels(EntryCall* c, const uint16_t* panels, size_t panel_elems, int planes, int K, int N) {
    c->scratch_what = "panel scratch"; c->scratch = panels; c->have = panel_elems;
    if (c->shaped()) c->need = (size_t)planes * N * ((K + 31) / 32 * 32);
}

int ams_k_pointwise(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w, const float* img_bias,
                    int64_t rows_per_img, const float* scale, const float* shift, int32_t act, const float* res, float* y,
                    void* stream) {
    EntryCall c = pw_entry("pointwise", M, K, N, 4);
    c.scale_without_shift = scale && !shift;
    c.ptrs = x && w && y;
    RUN(entry_check(c));
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    if (trans_w) { a.w_sk = 1; a.w_sn = K; }
    a.img_bias = img_bias; a.rows_per_img = rows_per_img > 0 ? rows_per_img : 1;
    a.scale = scale; a.shift = shift; a.act = act; a.res = res; a.ldr = N;
    return launch_pointwise(a, (hipStream_t)stream);
}

int ams_k_pointwise_split(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale, const float* shift,
                          int32_t act, const float* res, float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    EntryCall c = pw_entry("pointwise_split", M, K, N, 8);
    pw_entry_panels(&c, panels, panel_elems, 2, K, N);
    c.scale_without_shift = scale && !shift;
    c.ptrs = x && w && y;
    RUN(entry_check(c));
    const int Kp = (K + 31) / 32 * 32;
    hipStream_t st = (hipStream_t)stream;
    uint16_t* hi = panels;
    uint16_t* lo = panels + (size_t)N * Kp;
    RUN(launch_split_weights(w, N, 1, K, N, Kp, hi, lo, st));
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    a.scale = scale; a.shift = shift; a.act = act; a.res = res; a.ldr = N;
    return launch_pointwise_split(a, hi, lo, Kp, st);
}

int ams_k_pointwise_split3(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale, const float* shift,
                           int32_t act, const float* res, float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    EntryCall c = pw_entry("pointwise_split3", M, K, N, 8);
    pw_entry_panels(&c, panels, panel_elems, 3, K, N);
    c.scale_without_shift = scale && !shift;
    c.ptrs = x && w && y;
    RUN(entry_check(c));
    const int Kp = (K + 31) / 32 * 32;
    const size_t plane = (size_t)N * Kp;
    hipStream_t st = (hipStream_t)stream;
    RUN(launch_split_weights3(w, N, 1, K, N, Kp, panels, panels + plane, panels + 2 * plane, st));
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    a.scale = scale; a.shift = shift; a.act = act; a.res = res; a.ldr = N;
    return launch_pointwise_split3(a, panels, panels + plane, panels + 2 * plane, Kp, st);
}

int ams_k_pack_h2i(const float* x, int64_t M, int32_t Cn, float* out, void* stream) {
    EntryCall c;
    c.who = "pack_h2i";
    c.describe("M=%lld C=%d", (long long)M, Cn);
    c.sizes = M > 0 && Cn > 0;
    c.shape = Cn % 8 == 0;
    c.ptrs = x && out;
    RUN(entry_check(c));
    return launch_pack_h2i(x, M, Cn, out, (hipStream_t)stream);
}

int ams_k_pointwise_split_f16(const float* x, int64_t M, int32_t K, const float* w, int32_t N, const float* scale, const float* shift, int32_t act,
                              const float* res, float* y, uint16_t* panels, size_t panel_elems, float* x_h2i, uint16_t* y_parts, void* stream) {
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    a.scale = scale; a.shift = shift; a.act = act; a.res = res; a.ldr = N;
    EntryCall c = pw_entry("pointwise_split_f16", M, K, N, 8);
    // the fp16 form's own rule (K >= 32), and part planes only from a vector epilogue (N % 4 == 0)
    c.shape = c.sizes && pointwise_f16_applies(a) && (!y_parts || pointwise_split_writes_parts(a));
    pw_entry_panels(&c, panels, panel_elems, 2, K, N);
    c.scale_without_shift = scale && !shift;
    c.ptrs = x && w && y;
    RUN(entry_check(c));
    const int Kp = (K + 31) / 32 * 32;
    const size_t plane = (size_t)N * Kp;
    hipStream_t st = (hipStream_t)stream;
    RUN(launch_split_weights_f16(w, N, 1, K, N, Kp, panels, panels + plane, st));
    if (x_h2i) {                                   // the operand as fp16 pairs, as the streaming expand + depthwise kernels leave it
        if (x_h2i != x) RUN(launch_pack_h2i(x, M, K, x_h2i, st));      // x_h2i == x: x IS the packed operand already (tools/bench_kernel.py)
        a.x = x_h2i; a.x_fmt = 1;
    }
    if (y_parts) {                                 // the result also as two fp16 part planes [2][M][N] (the next block's operand)
        a.ysplit = y_parts; a.ysplit_plane = M * (int64_t)N; a.ysplit_np = 2; a.ysplit_fmt = 1;
    }
    return launch_pointwise_split_f16(a, panels, (int64_t)plane, Kp, st);
}

int ams_ingest_resize_u8(const uint8_t* src, int32_t Hs, int32_t Ws, int32_t Cn, int32_t mode, int32_t swap_rb, uint8_t* dst, int32_t H,
                         int32_t W, void* stream) {
    return launch_resize_u8(src, Hs, Ws, Cn, mode, swap_rb, dst, H, W, (hipStream_t)stream);
}

// ---- the frozen blocks (block_call.hpp).  Each entry fills the description, has it checked whole in front of its first launch (block_call_check, with
// the entry's name and its scratch), splits the weights into `panels` as ams_student_freeze does and hands the description to the launcher
static void set_panels(ConvLayer* l, const uint16_t* panels, int64_t plane, int np, int Kp) { l->panels = panels; l->plane = plane; l->np = np; l->Kp = Kp; }

int ams_k_dw_project(const float* e, int32_t B, int32_t H, int32_t W, int32_t Cc, const float* w_dw, int32_t rate, const float* scale_d,
                     const float* shift_d, const float* w_proj, int32_t N, const float* scale_p, const float* shift_p,
                     const float* res, float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t plane = (int64_t)N * Cc;
    BlockCall c;
    c.x = e; c.B = B; c.H = H; c.W = W; c.Cexp = Cc; c.rate = rate; c.Cout = N; c.residual = res != nullptr; c.res = res; c.y = y;
    c.dw = ConvLayer{w_dw, scale_d, shift_d, AMS_ACT_RELU6};
    c.project = ConvLayer{w_proj, scale_p, shift_p, AMS_ACT_NONE, panels, plane, 2, Cc};
    const EntryScratch sc{panels, panel_elems, (size_t)(2 * plane)};
    RUN(block_call_check("dw_project", BK_DW_PROJECT, c, &sc));
    RUN(launch_split_weights(w_proj, N, 1, Cc, N, Cc, panels, panels + plane, st));
    return launch_dw_project(c, st);
}

// ams_k_block_fused (exact f32; with panels the expand layer as three bf16 parts [part][Cexp][32]) and ams_k_block_fused_f16 (expand and project
// layers as two fp16 parts)
static int block_fused_entry(const char* who, bool f16, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp,
                             const float* scale_e, const float* shift_e, int32_t Cexp, const float* w_dw, int32_t stride, const float* scale_d,
                             const float* shift_d, const float* w_proj, int32_t Cout, const float* scale_p, const float* shift_p, int32_t residual,
                             float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int kp_p = (Cexp + 31) / 32 * 32;
    const int64_t pe = (int64_t)Cexp * 32, pp = (int64_t)Cout * kp_p;
    BlockCall c;
    c.x = x; c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cexp = Cexp; c.stride = stride; c.Cout = Cout; c.residual = residual != 0; c.y = y;
    c.expand = ConvLayer{w_exp, scale_e, shift_e, AMS_ACT_RELU6};
    c.dw = ConvLayer{w_dw, scale_d, shift_d, AMS_ACT_RELU6};
    c.project = ConvLayer{w_proj, scale_p, shift_p, AMS_ACT_NONE};
    uint16_t* hp = panels ? panels + 2 * pe : nullptr;
    if (f16) { set_panels(&c.expand, panels, pe, AMS_NP_F16, 32); set_panels(&c.project, hp, pp, AMS_NP_F16, kp_p); }
    else if (panels) set_panels(&c.expand, panels, pe, 3, 32);
    const EntryScratch sc{panels, panel_elems, (size_t)(f16 ? 2 * pe + 2 * pp : panels ? 3 * pe : 0)};
    RUN(block_call_check(who, BK_WHOLE, c, &sc));
    if (f16) {
        RUN(launch_split_weights_f16(w_exp, Cexp, 1, Cin, Cexp, 32, panels, panels + pe, st));
        RUN(launch_split_weights_f16(w_proj, Cout, 1, Cexp, Cout, kp_p, hp, hp + pp, st));
    } else if (panels)
        RUN(launch_split_weights3(w_exp, Cexp, 1, Cin, Cexp, 32, panels, panels + pe, panels + 2 * pe, st));
    return launch_block_fused(c, st);
}

int ams_k_block_fused(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e, const float* shift_e,
                      int32_t Cexp, const float* w_dw, int32_t stride, const float* scale_d, const float* shift_d, const float* w_proj, int32_t Cout,
                      const float* scale_p, const float* shift_p, int32_t residual, float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    return block_fused_entry("block_fused", false, x, B, H, W, Cin, w_exp, scale_e, shift_e, Cexp, w_dw, stride, scale_d, shift_d, w_proj, Cout, scale_p,
                             shift_p, residual, y, panels, panel_elems, stream);
}

int ams_k_block_fused_f16(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e, const float* shift_e,
                          int32_t Cexp, const float* w_dw, int32_t stride, const float* scale_d, const float* shift_d, const float* w_proj, int32_t Cout,
                          const float* scale_p, const float* shift_p, int32_t residual, float* y, uint16_t* panels, size_t panel_elems, void* stream) {
    return block_fused_entry("block_fused_f16", true, x, B, H, W, Cin, w_exp, scale_e, shift_e, Cexp, w_dw, stride, scale_d, shift_d, w_proj, Cout, scale_p,
                             shift_p, residual, y, panels, panel_elems, stream);
}

// ---- the first block (k_first_block.hip; the tile-per-wave form of k_block.hip): both entries and the plan query go through block_call_check
static_assert(sizeof(ams_first_block_plan) == sizeof(FirstBlockPlan) && sizeof(FirstBlockPlan) == 15 * sizeof(int32_t), "ams_first_block_plan is FirstBlockPlan, field by field");
static size_t first_block_scratch(int form) { return form == 1 ? 3 * 32 * 32 : (form == 2 ? 2 * 32 * 32 + 2 * 16 * 32 : 0); }
static BlockCall first_block_call(const void* frames, int dtype, int B, int H, int W, float pixel_scale, const float* w_stem, const float* scale_s,
                                  const float* shift_s, const float* w_dw, const float* scale_d, const float* shift_d, const float* w_proj,
                                  const float* scale_p, const float* shift_p, float* y) {
    BlockCall c;
    c.frames = frames; c.dtype = dtype; c.pixel_scale = pixel_scale; c.B = B; c.H = H; c.W = W; c.Cin = 3; c.Cexp = 32; c.Cout = 16; c.y = y;
    c.expand = ConvLayer{w_stem, scale_s, shift_s, AMS_ACT_RELU6};
    c.dw = ConvLayer{w_dw, scale_d, shift_d, AMS_ACT_RELU6};
    c.project = ConvLayer{w_proj, scale_p, shift_p, AMS_ACT_NONE};
    return c;
}

size_t ams_k_first_block_scratch(int32_t form) { return first_block_scratch(form); }

int ams_k_first_block_plan(int32_t frames_dtype, int32_t B, int32_t H, int32_t W, int32_t form, const int32_t* occupancy, ams_first_block_plan* plan_out) {
    BlockCall c;
    c.dtype = frames_dtype; c.B = B; c.H = H; c.W = W;
    const EntryScratch sc{nullptr, 0, 0, form, 3};
    RUN(block_call_check("first_block_plan", BK_FIRST_PLAN, c, &sc));
    AMS_REQUIRE(!occupancy || (occupancy[0] > 0 && occupancy[1] > 0 && occupancy[2] > 0), "first_block_plan: occupancy figures must be positive");
    AMS_REQUIRE(plan_out, "first_block_plan: null pointer");
    FirstBlockPlan p;
    RUN(first_block_plan(frames_dtype, B, H, W, form == 2, occupancy, &p));
    memcpy(plan_out, &p, sizeof(p));
    return AMS_OK;
}

int ams_k_first_block(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, float pixel_scale, const float* w_stem,
                      const float* scale_s, const float* shift_s, const float* w_dw, const float* scale_d, const float* shift_d, const float* w_proj,
                      const float* scale_p, const float* shift_p, float* y, int32_t form, uint16_t* panels, size_t panel_elems,
                      ams_first_block_plan* plan_out, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int64_t ps = 32 * 32, pj = 16 * 32;       // planes of the stem's [32 channels][32 k] and the project layer's [16][32] panels
    BlockCall c = first_block_call(frames, frames_dtype, B, H, W, pixel_scale, w_stem, scale_s, shift_s, w_dw, scale_d, shift_d, w_proj, scale_p, shift_p, y);
    uint16_t* hj = panels ? panels + 2 * ps : nullptr;
    if (form == 1) set_panels(&c.expand, panels, ps, 3, 32);
    else if (form == 2) { set_panels(&c.expand, panels, ps, AMS_NP_F16, 32); set_panels(&c.project, hj, pj, AMS_NP_F16, 32); }
    const EntryScratch sc{panels, panel_elems, first_block_scratch(form), form, 3};
    RUN(block_call_check("first_block", BK_FIRST, c, &sc));
    if (form == 1)                                  // as ams_student_freeze for layer 1: [27][32] -> three bf16 parts [32][32], k = tap * 3 + channel
        RUN(launch_split_weights3(w_stem, 32, 1, 27, 32, 32, panels, panels + ps, panels + 2 * ps, st));
    else if (form == 2) {                           // ... and for layers 1 and 3: two fp16 parts each
        RUN(launch_split_weights_f16(w_stem, 32, 1, 27, 32, 32, panels, panels + ps, st));
        RUN(launch_split_weights_f16(w_proj, 16, 1, 32, 16, 32, hj, hj + pj, st));
    }
    FirstBlockPlan p;
    RUN(launch_first_block(c, st, &p));
    if (plan_out) memcpy(plan_out, &p, sizeof(p));
    return AMS_OK;
}

int ams_k_first_block_tiles(const void* frames, int32_t frames_dtype, int32_t B, int32_t H, int32_t W, float pixel_scale, const float* w_stem,
                            const float* scale_s, const float* shift_s, const float* w_dw, const float* scale_d, const float* shift_d,
                            const float* w_proj, const float* scale_p, const float* shift_p, float* y, void* stream) {
    return launch_first_block_tiles(first_block_call(frames, frames_dtype, B, H, W, pixel_scale, w_stem, scale_s, shift_s, w_dw, scale_d, shift_d, w_proj,
                                                     scale_p, shift_p, y), (hipStream_t)stream);
}

int ams_k_expand_dw(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                    const float* shift_e, int32_t Cexp, const float* w_dw, int32_t stride, int32_t rate, const float* scale_d,
                    const float* shift_d, float* y, void* stream) {
    BlockCall c;
    c.x = x; c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cexp = Cexp; c.stride = stride; c.rate = rate; c.y = y;
    c.expand = ConvLayer{w_exp, scale_e, shift_e, AMS_ACT_RELU6};
    c.dw = ConvLayer{w_dw, scale_d, shift_d, AMS_ACT_RELU6};
    return launch_expand_dw(c, (hipStream_t)stream);
}

// ams_k_expand_dw_stream (f16 = false: `parts` = 2 | 3 of the three bf16 parts it splits; Cin <= 32: the exact-f32 form, where panels, parts and presplit
// are unused and rate = -2 selects stride 2) and ams_k_expand_dw_stream_f16 (the two fp16 parts).  presplit: x as parts behind the weight panels, 2 =
// the weight-register form (k_xdw_wreg.hip)
static int expand_dw_stream_entry(const char* who, bool f16, const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp,
                                  const float* scale_e, const float* shift_e, int32_t Cexp, const float* w_dw, int32_t rate, const float* scale_d,
                                  const float* shift_d, float* y, uint16_t* panels, size_t panel_elems, int32_t parts, int32_t presplit, int32_t y_h2i,
                                  void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const bool f32 = !f16 && Cin <= 32;
    const int ns = f16 ? 2 : 3;                     // planes the entry splits
    const size_t plane = (size_t)Cexp * Cin, xplane = (size_t)B * H * W * Cin;
    BlockCall c;
    c.x = x; c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cexp = Cexp; c.rate = rate; c.y = y; c.y_fmt = y_h2i ? 1 : 0;
    c.expand = ConvLayer{w_exp, scale_e, shift_e, AMS_ACT_RELU6};
    c.dw = ConvLayer{w_dw, scale_d, shift_d, AMS_ACT_RELU6};
    if (f32 && rate < 0) { c.stride = -rate; c.rate = 1; }
    const EntryScratch sc{panels, panel_elems, f32 ? 0 : ns * plane + (presplit ? ns * xplane : 0), 0, 1, f16 ? Cin >= 64 : (parts == 2 || parts == 3)};
    uint16_t* xq = panels && presplit ? panels + ns * plane : nullptr;      // the operand as parts, as a producing GEMM leaves it (PwArgs::ysplit)
    if (!f32) {
        set_panels(&c.expand, panels, (int64_t)plane, f16 ? AMS_NP_F16 : parts, Cin);
        c.x_parts = xq; c.x_plane = (int64_t)xplane;
    }
    const bool wreg = !f32 && presplit == 2;
    RUN(block_call_check(who, wreg ? BK_WREG : BK_STREAM, c, &sc));
    AMS_REQUIRE(x, "%s: null pointer", who);        // the weight-register form reads the parts only; the entry splits them from x
    if (!f32) {
        const int M = (int)((int64_t)B * H * W);
        if (f16) RUN(launch_split_weights_f16(w_exp, Cexp, 1, Cin, Cexp, Cin, panels, panels + plane, st));
        else RUN(launch_split_weights3(w_exp, Cexp, 1, Cin, Cexp, Cin, panels, panels + plane, panels + 2 * plane, st));
        if (xq && f16) RUN(launch_split_weights_f16(x, 1, Cin, Cin, M, Cin, xq, xq + xplane, st));
        else if (xq) RUN(launch_split_weights3(x, 1, Cin, Cin, M, Cin, xq, xq + xplane, xq + 2 * xplane, st));
    }
    return wreg ? launch_expand_dw_wreg(c, st) : launch_expand_dw_stream(c, st);
}

int ams_k_expand_dw_stream(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                           const float* shift_e, int32_t Cexp, const float* w_dw, int32_t rate, const float* scale_d, const float* shift_d,
                           float* y, uint16_t* panels, size_t panel_elems, int32_t parts, int32_t presplit, void* stream) {
    return expand_dw_stream_entry("expand_dw_stream", false, x, B, H, W, Cin, w_exp, scale_e, shift_e, Cexp, w_dw, rate, scale_d, shift_d, y, panels, panel_elems,
                                  parts, presplit, 0, stream);
}

int ams_k_expand_dw_stream_f16(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, const float* scale_e,
                               const float* shift_e, int32_t Cexp, const float* w_dw, int32_t rate, const float* scale_d, const float* shift_d,
                               float* y, uint16_t* panels, size_t panel_elems, int32_t presplit, int32_t y_h2i, void* stream) {
    return expand_dw_stream_entry("expand_dw_stream_f16", true, x, B, H, W, Cin, w_exp, scale_e, shift_e, Cexp, w_dw, rate, scale_d, shift_d, y, panels,
                                  panel_elems, 2, presplit, y_h2i, stream);
}

// The steps of the launch ams_k_expand_dw_stream[_f16] would make for these arguments (the launchers' own geometry functions, the kernels' own
// step rule): host arithmetic, no GPU call.  Checked as the launch entries check their shape.
int ams_k_expand_dw_steps(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cexp, int32_t rate, int32_t f16, int32_t presplit, int32_t* out, size_t n) {
    const bool f32 = !f16 && Cin <= 32;
    const bool wreg = !f32 && presplit == 2;
    BlockCall c;
    c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cexp = Cexp; c.rate = rate;
    if (f32 && rate < 0) { c.stride = -rate; c.rate = 1; }
    AMS_REQUIRE(B > 0 && H > 0 && W > 0, "expand_dw_steps: no pixels: B=%d, %d x %d", B, H, W);
    AMS_REQUIRE(expand_dw_stream_supported(Cin, Cexp, c.stride, c.rate) && (!f16 || Cin >= 64), "expand_dw_steps: unsupported shape Cin=%d Cexp=%d rate=%d",
                Cin, Cexp, rate);
    AMS_REQUIRE(out && n >= 10, "expand_dw_steps: out needs at least 10 elements");
    const int np = f32 ? 0 : (f16 ? 2 : 3);         // parts as staged: the bf16 entry is counted with its three parts
    XdwGeom g;
    const bool fits = wreg ? expand_dw_wreg_geom(B, H, W, Cin, Cexp, c.rate, np, &g) : expand_dw_stream_geom(B, H, W, Cin, Cexp, c.rate, np, &g);
    AMS_REQUIRE(fits, "expand_dw_steps: no segment geometry fits LDS (W=%d rate=%d)", W, rate);
    expand_dw_steps(g, H, W, c.rate, out, n);
    return AMS_OK;
}

int ams_k_global_mean(const float* x, int32_t B, int64_t HW, int32_t C, float* y, float* scratch, size_t scratch_floats,
                      void* stream) {
    AMS_REQUIRE(scratch && scratch_floats >= image_colsum_scratch(B, C), "global_mean: scratch too small (need %zu floats)",
                image_colsum_scratch(B, C));
    return launch_global_mean(x, B, HW, C, y, scratch, (hipStream_t)stream);
}
size_t ams_k_global_mean_scratch(int32_t B, int32_t C) { return image_colsum_scratch(B, C); }

int ams_k_upsample_argmax(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K,
                          int32_t H, int32_t W, const uint8_t* teacher, int32_t* labels_out, int64_t* conf_mat, double* loss,
                          void* stream) {
    const HeadCall c{logits, NC, B, h, w, class_idx_host, K, H, W, teacher, NC};
    return launch_upsample_argmax(c, labels_out, conf_mat, loss, (hipStream_t)stream);
}

int ams_k_upsample_confidence(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K,
                              int32_t H, int32_t W, const uint8_t* teacher, uint8_t* conf_u8, float* conf_f32, int64_t* stats, void* stream) {
    const HeadCall c{logits, NC, B, h, w, class_idx_host, K, H, W, teacher, NC};
    return launch_upsample_confidence(c, conf_u8, conf_f32, stats, (hipStream_t)stream);
}
size_t ams_confidence_stats_len(void) { return (size_t)confidence_stats_len(); }

int ams_k_upsample_soft_metric_layout(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                                      int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw,
                                      int32_t layout, int64_t* stats, float* p_f32, float* ce_f32, void* stream) {
    const HeadCall c{logits, ld, B, h, w, class_idx_host, K, H, W, teacher, NC};
    return launch_upsample_soft_metric(c, LossObjective{teacher_logits, th, tw, layout}, stats, p_f32, ce_f32, (hipStream_t)stream);
}

int ams_k_upsample_soft_metric(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K,
                               int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, int64_t* stats,
                               float* p_f32, float* ce_f32, void* stream) {
    return ams_k_upsample_soft_metric_layout(logits, B, h, w, NC, NC, class_idx_host, K, H, W, teacher, teacher_logits, th, tw, AMS_TLOGITS_FULL, stats, p_f32,
                                             ce_f32, stream);
}
size_t ams_soft_metric_stats_len(int32_t K) { return K >= 1 && K <= 32 ? (size_t)soft_metric_stats_len(K) : 0; }

int ams_k_ce_grad(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K, int32_t H,
                  int32_t W, const uint8_t* teacher, const double* loss_and_count_dev, float* dlogits, void* stream) {
    const HeadCall c{logits, NC, B, h, w, class_idx_host, K, H, W, teacher, NC};
    return launch_ce_grad(c, loss_and_count_dev, dlogits, NC, (hipStream_t)stream);
}

size_t ams_k_ce_loss_grad_scratch(int32_t B, int32_t h, int32_t w, int32_t K) { return ce_loss_grad_scratch(B, h, w, K); }

// The one body of the five kernel-level loss entries.  Refused in this order: the KD parameters; the weights, before any pointer is looked at;
// null teacher logits where the objective needs them (needs_teacher_logits: always, but for the weighted entry at alpha = 0 and gamma = 0); the
// class table; K; layout; row stride; geometry; scratch.  Then the two launches.
static int ce_loss_grad_entry(const char* who, const HeadCall& c, const LossObjective& o, bool needs_teacher_logits, double* loss_dev, float* dlogits,
                              float* scratch, size_t scratch_floats, void* stream) {
    RUN(kd_params_check(who, o.temperature, o.alpha));
    RUN(loss_weights_check(who, o.class_weights, c.K, c.K, o.conf_gamma));
    AMS_REQUIRE(o.teacher_logits || !needs_teacher_logits, "%s: null teacher logits (alpha %g, conf_gamma %g)", who, (double)o.alpha, (double)o.conf_gamma);
    AMS_REQUIRE(c.cls, "%s: null class table", who);
    AMS_REQUIRE(c.K >= 1 && c.K <= 32, "%s: K=%d out of range (1..32)", who, c.K);
    AMS_REQUIRE(tlogits_layout_ok(o.layout), "%s: unknown teacher-logit layout %d", who, o.layout);
    AMS_REQUIRE(c.ld >= c.NC && c.ld <= 256, "%s: row stride %d must hold %d classes", who, c.ld, c.NC);
    AMS_REQUIRE(ce_loss_grad_supported(c.w, c.W), "%s: %d output columns on %d source columns is outside the one-pass kernel", who, c.W, c.w);
    AMS_REQUIRE(scratch && scratch_floats >= ce_loss_grad_scratch(c.B, c.h, c.w, c.K), "%s: scratch too small (need %zu floats)", who,
                ce_loss_grad_scratch(c.B, c.h, c.w, c.K));
    hipStream_t st = (hipStream_t)stream;
    RUN(launch_ce_loss_grad(c, o, loss_dev, scratch, st));
    return launch_ce_combine(c, loss_dev, scratch, dlogits, c.ld, st);
}

int ams_k_ce_loss_grad(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K, int32_t H,
                       int32_t W, const uint8_t* teacher, double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream) {
    const HeadCall c{logits, NC, B, h, w, class_idx_host, K, H, W, teacher, NC};
    return ce_loss_grad_entry("ce_loss_grad", c, LossObjective{}, false, loss_dev, dlogits, scratch, scratch_floats, stream);
}

int ams_k_ce_loss_grad_soft(const float* logits, int32_t B, int32_t h, int32_t w, int32_t NC, const int32_t* class_idx_host, int32_t K, int32_t H,
                            int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, double* loss_dev, float* dlogits,
                            float* scratch, size_t scratch_floats, void* stream) {
    const HeadCall c{logits, NC, B, h, w, class_idx_host, K, H, W, teacher, NC};
    const LossObjective o{teacher_logits, th, tw, AMS_TLOGITS_FULL};
    return ce_loss_grad_entry("ce_loss_grad_soft", c, o, true, loss_dev, dlogits, scratch, scratch_floats, stream);
}

int ams_k_ce_loss_grad_soft_layout(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host,
                                   int32_t K, int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, int32_t layout,
                                   double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream) {
    const HeadCall c{logits, ld, B, h, w, class_idx_host, K, H, W, teacher, NC};
    const LossObjective o{teacher_logits, th, tw, layout};
    return ce_loss_grad_entry("ce_loss_grad_soft_layout", c, o, true, loss_dev, dlogits, scratch, scratch_floats, stream);
}

int ams_k_ce_loss_grad_kd(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host, int32_t K,
                          int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, int32_t layout,
                          double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream, float temperature, float alpha) {
    const HeadCall c{logits, ld, B, h, w, class_idx_host, K, H, W, teacher, NC};
    const LossObjective o{teacher_logits, th, tw, layout, temperature, alpha};
    return ce_loss_grad_entry("ce_loss_grad_kd", c, o, true, loss_dev, dlogits, scratch, scratch_floats, stream);
}

int ams_k_ce_loss_grad_weighted(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host, int32_t K,
                                int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, int32_t layout,
                                double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream, float temperature, float alpha,
                                const float* class_weights_host, float conf_gamma) {
    const HeadCall c{logits, ld, B, h, w, class_idx_host, K, H, W, teacher, NC};
    const LossObjective o{teacher_logits, th, tw, layout, temperature, alpha, class_weights_host, conf_gamma};
    // the one entry that takes NULL teacher logits: when neither the mix nor the weight looks at them
    return ce_loss_grad_entry("ce_loss_grad_weighted", c, o, conf_gamma != 0.f || alpha != 0.f, loss_dev, dlogits, scratch, scratch_floats, stream);
}

size_t ams_k_loss_mining_scratch(int32_t B, int32_t H, int32_t W) { return loss_mining_scratch(B, H, W); }

// The weighted entry's refusals in its order (ce_loss_grad_entry), then top_k, the mining scratch and the outputs; then steps 1 - 3 and the weighted
// entry's two launches on the mined map
int ams_k_ce_loss_grad_mined(const float* logits, int32_t B, int32_t h, int32_t w, int32_t ld, int32_t NC, const int32_t* class_idx_host, int32_t K,
                             int32_t H, int32_t W, const uint8_t* teacher, const float* teacher_logits, int32_t th, int32_t tw, int32_t layout,
                             double* loss_dev, float* dlogits, float* scratch, size_t scratch_floats, void* stream, float temperature, float alpha,
                             const float* class_weights_host, float conf_gamma, float top_k, uint8_t* labels_out_dev, float* key_out_dev,
                             ams_mining_result* result_dev, void* mining_scratch_dev, size_t mining_scratch_bytes) {
    const char* who = "ce_loss_grad_mined";
    HeadCall c{logits, ld, B, h, w, class_idx_host, K, H, W, teacher, NC};
    const LossObjective o{teacher_logits, th, tw, layout, temperature, alpha, class_weights_host, conf_gamma};
    RUN(kd_params_check(who, o.temperature, o.alpha));
    RUN(loss_weights_check(who, o.class_weights, c.K, c.K, o.conf_gamma));
    AMS_REQUIRE(o.teacher_logits || (conf_gamma == 0.f && alpha == 0.f), "%s: null teacher logits (alpha %g, conf_gamma %g)", who, (double)o.alpha, (double)o.conf_gamma);
    AMS_REQUIRE(c.cls, "%s: null class table", who);
    AMS_REQUIRE(c.K >= 1 && c.K <= 32, "%s: K=%d out of range (1..32)", who, c.K);
    AMS_REQUIRE(tlogits_layout_ok(o.layout), "%s: unknown teacher-logit layout %d", who, o.layout);
    AMS_REQUIRE(c.ld >= c.NC && c.ld <= 256, "%s: row stride %d must hold %d classes", who, c.ld, c.NC);
    AMS_REQUIRE(ce_loss_grad_supported(c.w, c.W), "%s: %d output columns on %d source columns is outside the one-pass kernel", who, c.W, c.w);
    AMS_REQUIRE(scratch && scratch_floats >= ce_loss_grad_scratch(c.B, c.h, c.w, c.K), "%s: scratch too small (need %zu floats)", who,
                ce_loss_grad_scratch(c.B, c.h, c.w, c.K));
    RUN(mining_top_k_check(who, top_k));
    hipStream_t st = (hipStream_t)stream;
    if (top_k < 1.f) {
        AMS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: no pixels: B=%d, %d x %d", who, B, H, W);
        AMS_REQUIRE(mining_scratch_dev && ((uintptr_t)mining_scratch_dev & 15) == 0 && mining_scratch_bytes >= loss_mining_scratch(B, H, W),
                    "%s: mining scratch NULL, misaligned or too small (need %zu bytes, 16-byte aligned)", who, loss_mining_scratch(B, H, W));
        AMS_REQUIRE(labels_out_dev && result_dev, "%s: null output (mined labels, result)", who);
        AMS_REQUIRE(((uintptr_t)result_dev & 7) == 0 && ((uintptr_t)key_out_dev & 3) == 0, "%s: misaligned output", who);
        MiningBuffers m = loss_mining_buffers(mining_scratch_dev, B, H, W);
        m.labels = labels_out_dev;
        m.result = result_dev;
        if (key_out_dev) m.keys = key_out_dev;
        AMS_REQUIRE(loss_dev && dlogits, "%s: null pointer", who);
        RUN(launch_loss_mining(c, o, top_k, m, st));
        c.teacher = labels_out_dev;
    } else {
        AMS_REQUIRE(labels_out_dev, "%s: null output (mined labels)", who);
        AMS_REQUIRE(c.logits && c.teacher && loss_dev && dlogits && B >= 1 && H >= 1 && W >= 1, "%s: null pointer", who);
        AMS_CHECK_HIP(hipMemcpyAsync(labels_out_dev, teacher, (size_t)B * H * W, hipMemcpyDeviceToDevice, st));
    }
    RUN(launch_ce_loss_grad(c, o, loss_dev, scratch, st));
    return launch_ce_combine(c, loss_dev, scratch, dlogits, c.ld, st);
}

size_t ams_k_pointwise_wgrad_scratch(int64_t M, int32_t K, int32_t N) {
    return AMS_ENTRY_SCRATCH(M > 0 && K > 0 && N > 0, pointwise_wgrad_scratch(M, K, N));
}

// the weight-gradient entries: M, K, N > 0; split: the three-part kernel's rule (pointwise_wgrad_x6_applies); scratch: the floats of the kernel
// the entry runs (the exact-f32 kernel's where split == 0 or the three-part kernel does not apply)
static EntryCall wg_entry(const char* who, int64_t M, int K, int N, int split, bool split_required, const float* scratch, size_t scratch_floats) {
    EntryCall c;
    c.who = who;
    c.describe("M=%lld K=%d N=%d", (long long)M, K, N);
    c.sizes = M > 0 && K > 0 && N > 0;
    const bool x6 = c.sizes && split && pointwise_wgrad_x6_applies(M, K, N, K, N);
    c.shape = !(split && split_required) || x6;
    c.scratch_what = "scratch"; c.scratch = scratch; c.have = scratch_floats;
    if (c.shaped()) c.need = (size_t)(x6 ? wgrad_x6_splits(M, K, N) : wgrad_f32_splits(M, K, N)) * K * N;
    return c;
}

int ams_k_pointwise_wgrad_split(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, float* dw, float* scratch,
                                size_t scratch_floats, void* stream) {
    EntryCall c = wg_entry("pointwise_wgrad_split", M, K, N, 1, true, scratch, scratch_floats);
    c.ptrs = x && dy && dw;
    RUN(entry_check(c));
    WgArgs a;
    a.x = x; a.ldx = K; a.K = K; a.dy = dy; a.ldy = N; a.N = N; a.M = M; a.dw = dw; a.scratch = scratch; a.scratch_floats = scratch_floats; a.allow_split = 1;
    return launch_pointwise_wgrad(a, (hipStream_t)stream);
}

int ams_k_pointwise_wgrad(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, float* dw, float* scratch,
                          size_t scratch_floats, void* stream) {
    EntryCall c = wg_entry("pointwise_wgrad", M, K, N, 0, false, scratch, scratch_floats);
    c.ptrs = x && dy && dw;
    RUN(entry_check(c));
    WgArgs a;
    a.x = x; a.ldx = K; a.K = K; a.dy = dy; a.ldy = N; a.N = N; a.M = M; a.dw = dw; a.scratch = scratch; a.scratch_floats = scratch_floats; a.allow_split = 0;
    return launch_pointwise_wgrad(a, (hipStream_t)stream);
}

int ams_k_depthwise3x3_dgrad(const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t stride, int32_t rate,
                             float* dx, void* stream) {
    EntryCall c = dw_entry("depthwise3x3_dgrad", B, H, W, C, stride, rate);
    c.ptrs = dy && w && dx;
    RUN(entry_check(c));
    return launch_depthwise_dgrad(dy, B, H, W, C, w, stride, rate, dx, (hipStream_t)stream);
}

int ams_k_depthwise3x3_wgrad(const float* x, const float* dy, int32_t B, int32_t H, int32_t W, int32_t C, int32_t stride, int32_t rate,
                             float* dw, float* scratch, size_t scratch_floats, void* stream) {
    EntryCall c = dw_entry("depthwise3x3_wgrad", B, H, W, C, stride, rate);
    c.scratch_what = "scratch"; c.scratch = scratch; c.have = scratch_floats;
    if (c.shaped()) c.need = depthwise_wgrad_scratch(B, H, W, C, stride, rate);
    c.ptrs = x && dy && dw;
    RUN(entry_check(c));
    return launch_depthwise_wgrad(x, dy, B, H, W, C, stride, rate, dw, scratch, scratch_floats, (hipStream_t)stream);
}

int ams_k_pointwise_red(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w, int32_t split, int32_t mode,
                        const float* center, const float* z, const float* scale, const float* shift, const float* mean, const float* rstd,
                        int32_t act, const float* res, float* y, float* part, size_t part_floats, int32_t* rows_out, uint16_t* panels,
                        size_t panel_elems, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    if (trans_w) { a.w_sk = 1; a.w_sn = K; }
    a.res = res; a.ldr = N;
    a.red_mode = mode; a.red_center = center; a.red_z = z; a.red_scale = scale; a.red_shift = shift; a.red_mean = mean; a.red_rstd = rstd;
    a.red_act = act; a.red_part = part; a.red_part_floats = part_floats;         // rows that would not fit: the launch runs unfused, *rows_out = 0
    int rows = 0;
    a.red_rows_out = &rows;
    // M, K, N > 0; mode 1 | 2; split 0: K % 4 == 0, split 1: K % 8 == 0 and 3 panel planes, split 2: the fp16 form's rule (mode 1, K >= 32, K % 8
    // == 0) and 2 planes; mode 2 reads z, scale, shift, mean, rstd
    EntryCall c = pw_entry("pointwise_red", M, K, N, split ? 8 : 4);
    c.shape = c.shape && (mode == 1 || mode == 2) && (split != 2 || (c.sizes && pointwise_f16_applies(a)));
    if (split) pw_entry_panels(&c, panels, panel_elems, split == 2 ? 2 : 3, K, N);
    c.ptrs = x && w && y && part && rows_out && (mode == 1 || (z && scale && shift && mean && rstd));
    RUN(entry_check(c));
    int rc;
    if (split == 2) {                              // two fp16 parts (mode 1 only: the forward statistics)
        const int Kp = (K + 31) / 32 * 32;
        const size_t plane = (size_t)N * Kp;
        RUN(launch_split_weights_f16(w, a.w_sk, a.w_sn, K, N, Kp, panels, panels + plane, st));
        rc = launch_pointwise_split_f16(a, panels, (int64_t)plane, Kp, st);
    } else if (split) {
        const int Kp = (K + 31) / 32 * 32;
        const size_t plane = (size_t)N * Kp;
        RUN(launch_split_weights3(w, a.w_sk, a.w_sn, K, N, Kp, panels, panels + plane, panels + 2 * plane, st));
        rc = launch_pointwise_split3(a, panels, panels + plane, panels + 2 * plane, Kp, st);
    } else {
        rc = launch_pointwise(a, st);
    }
    *rows_out = rows;
    return rc;
}

int ams_k_pointwise_xform(const float* x, int64_t M, int32_t K, const float* w, int32_t N, int32_t trans_w, int32_t split, int32_t x_mode,
                          int32_t x_act, const float* v0, const float* v1, const float* v2, const float* x2, float* y, float* x_tmp,
                          uint16_t* panels, size_t panel_elems, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    PwArgs a = pw_args(x, M, K, K, w, N, y, N);
    if (trans_w) { a.w_sk = 1; a.w_sn = K; }
    a.x_mode = x_mode; a.x_act = x_act; a.x_v0 = v0; a.x_v1 = v1; a.x_v2 = v2; a.x2 = x2; a.x_tmp = x_tmp;
    // M, K, N > 0; x_mode 1 | 2; split 0: K % 4 == 0, split 1: K % 8 == 0 and 3 panel planes, split 2: the fp16 form's rule (x_mode 1, 32 <= K <=
    // 1024, K % 8 == 0, a plain vector epilogue) and 2 planes; x_mode 2 reads v2 and x2
    EntryCall c = pw_entry("pointwise_xform", M, K, N, split ? 8 : 4);
    const bool vecs = v0 && v1 && (x_mode != 2 || (v2 && x2));
    c.shape = c.shape && (x_mode == 1 || x_mode == 2) && (split != 2 || !vecs || (c.sizes && pointwise_f16_applies(a)));      // (the fp16 rule looks at v0, v1: without them the call ends at 5)
    if (split) pw_entry_panels(&c, panels, panel_elems, split == 2 ? 2 : 3, K, N);
    c.ptrs = x && w && y && vecs;
    RUN(entry_check(c));
    if (split == 2) {                              // two fp16 parts (x_mode 1 only)
        const int Kp = (K + 31) / 32 * 32;
        const size_t plane = (size_t)N * Kp;
        RUN(launch_split_weights_f16(w, a.w_sk, a.w_sn, K, N, Kp, panels, panels + plane, st));
        return launch_pointwise_split_f16(a, panels, (int64_t)plane, Kp, st);
    }
    if (split) {
        const int Kp = (K + 31) / 32 * 32;
        const size_t plane = (size_t)N * Kp;
        RUN(launch_split_weights3(w, a.w_sk, a.w_sn, K, N, Kp, panels, panels + plane, panels + 2 * plane, st));
        return launch_pointwise_split3(a, panels, panels + plane, panels + 2 * plane, Kp, st);
    }
    return launch_pointwise(a, st);
}

int ams_k_pointwise_wgrad_xform(const float* x, const float* dy, int64_t M, int32_t K, int32_t N, int32_t split, int32_t x_mode, int32_t x_act,
                                const float* v0, const float* v1, int32_t dy_mode, const float* d0, const float* d1, const float* d2,
                                const float* dy2, float* dw, float* scratch, size_t scratch_floats, void* stream) {
    EntryCall c = wg_entry("pointwise_wgrad_xform", M, K, N, split, true, scratch, scratch_floats);
    c.shape = c.shape && (x_mode == 0 || x_mode == 1) && (dy_mode == 0 || dy_mode == 2);
    c.ptrs = x && dy && dw && (x_mode != 1 || (v0 && v1)) && (dy_mode != 2 || (d0 && d1 && d2 && dy2));
    RUN(entry_check(c));
    WgArgs a;
    a.x = x; a.ldx = K; a.K = K; a.dy = dy; a.ldy = N; a.N = N; a.M = M; a.dw = dw; a.scratch = scratch; a.scratch_floats = scratch_floats;
    a.allow_split = split != 0;
    a.x_mode = x_mode; a.x_act = x_act; a.x_v0 = v0; a.x_v1 = v1;
    a.dy_mode = dy_mode; a.dy_v0 = d0; a.dy_v1 = d1; a.dy_v2 = d2; a.dy2 = dy2;
    return launch_pointwise_wgrad(a, (hipStream_t)stream);
}

// the four one-kernel fine-tune forms: stride 1; the depthwise rule (dw_entry); fwd_bn_tiles: an image of fewer than 2^31 elements
static EntryCall dw_bn_entry(const char* who, int B, int H, int W, int C, int rate, const float* scratch, size_t scratch_floats) {
    EntryCall c = dw_entry(who, B, H, W, C, 1, rate);
    c.scratch_what = "scratch"; c.scratch = scratch; c.have = scratch_floats;
    return c;
}
static bool dw_bn_accepts(int B, int H, int W, int C, int rate) { return sizes3(B, H, W) && C > 0 && dw_entry_shape(C, 1, rate); }

size_t ams_k_depthwise3x3_fwd_bn_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate) {
    return AMS_ENTRY_SCRATCH(dw_bn_accepts(B, H, W, C, rate), depthwise_fwd_bn_scratch(B, H, W, C, rate));
}
int ams_k_depthwise3x3_fwd_bn(const float* ze, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate, const float* scale,
                              const float* shift, int32_t act, const float* center, float* zd, float* scratch, size_t scratch_floats,
                              int32_t* rows_out, void* stream) {
    EntryCall c = dw_bn_entry("depthwise3x3_fwd_bn", B, H, W, C, rate, scratch, scratch_floats);
    if (c.shaped()) c.need = depthwise_fwd_bn_scratch(B, H, W, C, rate);
    c.ptrs = ze && w && scale && shift && zd && rows_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_depthwise_fwd_bn(ze, B, H, W, C, w, rate, scale, shift, act, center, zd, scratch, &rows, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}
size_t ams_k_depthwise3x3_dgrad_bn_scratch(int32_t B, int32_t H, int32_t W, int32_t C) {
    return AMS_ENTRY_SCRATCH(dw_bn_accepts(B, H, W, C, 1), depthwise_dgrad_bn_scratch(B, H, W, C));
}
int ams_k_depthwise3x3_dgrad_bn(const float* dz, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate, const float* z_prev,
                                const float* scale, const float* shift, int32_t act, const float* mean, const float* rstd, float* out,
                                float* scratch, size_t scratch_floats, int32_t* rows_out, void* stream) {
    EntryCall c = dw_bn_entry("depthwise3x3_dgrad_bn", B, H, W, C, rate, scratch, scratch_floats);
    if (c.shaped()) c.need = depthwise_dgrad_bn_scratch(B, H, W, C);
    c.ptrs = dz && w && z_prev && scale && shift && mean && rstd && out && rows_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_depthwise_dgrad_bn(dz, B, H, W, C, w, rate, z_prev, scale, shift, act, mean, rstd, out, scratch, &rows, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}

size_t ams_k_depthwise3x3_fwd_bn_tiles_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate) {
    return AMS_ENTRY_SCRATCH(dw_bn_accepts(B, H, W, C, rate) && (int64_t)H * W * C < 0x7fffffffLL, depthwise_fwd_bn2_scratch(B, H, W, C, rate));
}
int ams_k_depthwise3x3_fwd_bn_tiles(const float* ze, int32_t B, int32_t H, int32_t W, int32_t C, const float* w, int32_t rate, const float* scale,
                                    const float* shift, int32_t act, const float* center, float* zd, float* scratch, size_t scratch_floats,
                                    int32_t* rows_out, void* stream) {
    EntryCall c = dw_bn_entry("depthwise3x3_fwd_bn_tiles", B, H, W, C, rate, scratch, scratch_floats);
    c.shape = c.shape && (int64_t)H * W * C < 0x7fffffffLL;
    if (c.shaped()) c.need = depthwise_fwd_bn2_scratch(B, H, W, C, rate);
    c.ptrs = ze && w && scale && shift && zd && rows_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_depthwise_fwd_bn2(ze, B, H, W, C, w, rate, scale, shift, act, center, zd, scratch, &rows, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}

size_t ams_k_depthwise3x3_dgrad_bn_apply_scratch(int32_t B, int32_t H, int32_t W, int32_t C, int32_t rate) {
    return AMS_ENTRY_SCRATCH(dw_bn_accepts(B, H, W, C, rate), depthwise_dgrad_bn2_scratch(B, H, W, C, rate));
}
int ams_k_depthwise3x3_dgrad_bn_apply(const float* dy, const float* zd, const float* cA, const float* cB, const float* cC, int32_t B, int32_t H, int32_t W,
                                      int32_t C, const float* w, int32_t rate, const float* z_prev, const float* scale, const float* shift, int32_t act,
                                      const float* mean, const float* rstd, float* out, float* scratch, size_t scratch_floats, int32_t* rows_out,
                                      void* stream) {
    EntryCall c = dw_bn_entry("depthwise3x3_dgrad_bn_apply", B, H, W, C, rate, scratch, scratch_floats);
    if (c.shaped()) c.need = depthwise_dgrad_bn2_scratch(B, H, W, C, rate);
    c.ptrs = dy && zd && cA && cB && cC && w && z_prev && scale && shift && mean && rstd && out && rows_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_depthwise_dgrad_bn2(dy, zd, cA, cB, cC, B, H, W, C, w, rate, z_prev, scale, shift, act, mean, rstd, out, scratch, &rows, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}

size_t ams_k_xx_gram_scratch(int64_t M, int32_t Cin) { return AMS_ENTRY_SCRATCH(M > 0 && xx_gram_shape(Cin), xx_stats_scratch_doubles(M, Cin)); }
int ams_k_xx_gram(const float* x, int64_t M, int32_t Cin, double* scratch, size_t scratch_doubles, double* xx64, float* xx32, void* stream) {
    EntryCall c;
    c.who = "xx_gram";
    c.describe("M=%lld Cin=%d", (long long)M, Cin);
    c.sizes = M > 0 && Cin > 0;
    c.shape = xx_gram_shape(Cin);
    c.scratch_what = "scratch"; c.scratch = scratch; c.have = scratch_doubles;
    if (c.shaped()) c.need = xx_stats_scratch_doubles(M, Cin);
    c.ptrs = x && xx64;
    RUN(entry_check(c));
    return launch_xx_gram(x, M, Cin, scratch, xx64, xx32, (hipStream_t)stream);
}
int ams_k_expand_stats(const double* xx64, int32_t Cin, const float* w_exp, int32_t Cexp, double n, const float* center, const float* gamma,
                       const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale, float* shift,
                       float* save_mean, float* save_rstd, double* sums, void* stream) {
    EntryCall c;
    c.who = "expand_stats";
    c.describe("Cin=%d Cexp=%d n=%g", Cin, Cexp, n);
    c.sizes = Cin > 0 && Cexp > 0 && n > 0;
    c.shape = xx_gram_shape(Cin);
    // the saved statistics and the moving averages each come as a pair or not at all
    c.ptrs = xx64 && w_exp && gamma && beta && scale && shift && (save_mean == nullptr) == (save_rstd == nullptr) &&
             (moving_mean == nullptr) == (moving_var == nullptr);
    RUN(entry_check(c));
    return launch_expand_stats(xx64, Cin, w_exp, Cexp, n, center, gamma, beta, eps, one_minus_decay, moving_mean, moving_var, scale, shift, save_mean,
                               save_rstd, sums, (hipStream_t)stream);
}

// the recompute entries of an early block: B, H, W, Cin, Cexp > 0; xdw_train_supported (Cin % 4 == 0 in 8..32, Cexp % 16 == 0 in 32..192, stride
// 1 | 2) and an image the kernels' 32-bit element offsets cover
static EntryCall xdw_entry(const char* who, int B, int H, int W, int Cin, int Cexp, int stride) {
    EntryCall c;
    c.who = who;
    c.describe("B=%d, %d x %d, Cin=%d Cexp=%d stride=%d", B, H, W, Cin, Cexp, stride);
    c.sizes = sizes3(B, H, W) && Cin > 0 && Cexp > 0;
    c.shape = xdw_train_supported(Cin, Cexp, stride, 1) && xdw_image_ok(H, W, Cin, Cexp);
    return c;
}
static void xdw_entry_scratch(EntryCall* c, const float* scratch, size_t scratch_floats, int B, int H, int W, int Cin, int Cexp) {
    c->scratch_what = "scratch"; c->scratch = scratch; c->have = scratch_floats;
    if (c->shaped()) c->need = xdw_train_scratch(B, H, W, Cin, Cexp);
}

size_t ams_k_xdw_train_scratch(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cexp) {
    return AMS_ENTRY_SCRATCH(xdw_entry("", B, H, W, Cin, Cexp, 1).shaped(), xdw_train_scratch(B, H, W, Cin, Cexp));
}
int ams_k_xdw_fwd_stats(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* center,
                        float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream) {
    EntryCall c = xdw_entry("xdw_fwd_stats", B, H, W, Cin, Cexp, 1);
    xdw_entry_scratch(&c, scratch, scratch_floats, B, H, W, Cin, Cexp);
    c.ptrs = x && w_exp && rows_out && stride_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_xdw_fwd_stats(x, B, H, W, Cin, w_exp, Cexp, center, scratch, &rows, stride_out, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}
int ams_k_xdw_bwd_reduce(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* sc_e,
                         const float* sh_e, const float* mean_e, const float* rstd_e, int32_t act_e, const float* w_dw, int32_t stride,
                         const float* dz_d, float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream) {
    EntryCall c = xdw_entry("xdw_bwd_reduce", B, H, W, Cin, Cexp, stride);
    xdw_entry_scratch(&c, scratch, scratch_floats, B, H, W, Cin, Cexp);
    c.ptrs = x && w_exp && sc_e && sh_e && mean_e && rstd_e && w_dw && dz_d && rows_out && stride_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_xdw_bwd_reduce(x, B, H, W, Cin, w_exp, Cexp, sc_e, sh_e, mean_e, rstd_e, act_e, w_dw, stride, dz_d, scratch, &rows, stride_out,
                                   (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}
int ams_k_xdw_bwd_dx(const float* x, int32_t B, int32_t H, int32_t W, int32_t Cin, const float* w_exp, int32_t Cexp, const float* sc_e,
                     const float* sh_e, int32_t act_e, const float* w_dw, int32_t stride, const float* dz_d, const float* cA, const float* cB,
                     const float* cC, const float* res, float* dx, void* stream) {
    EntryCall c = xdw_entry("xdw_bwd_dx", B, H, W, Cin, Cexp, stride);
    c.ptrs = x && w_exp && sc_e && sh_e && w_dw && dz_d && cA && cB && cC && dx;
    RUN(entry_check(c));
    return launch_xdw_bwd_dx(x, B, H, W, Cin, w_exp, Cexp, sc_e, sh_e, act_e, w_dw, stride, dz_d, cA, cB, cC, res, dx, (hipStream_t)stream);
}
size_t ams_k_xdw_stem_scratch(int32_t B, int32_t fH, int32_t fW) {
    return AMS_ENTRY_SCRATCH(sizes3(B, fH, fW) && (int64_t)fH * fW * 3 < 0x7fffffffLL, xdw_stem_scratch(B, fH, fW));
}
int ams_k_xdw_bwd_reduce_stem(const void* frames, int32_t frames_dtype, int32_t B, int32_t fH, int32_t fW, float pixel_scale, const float* w_stem,
                              const float* sc_e, const float* sh_e, const float* mean_e, const float* rstd_e, int32_t act_e, const float* w_dw,
                              const float* dz_d, float* scratch, size_t scratch_floats, int32_t* rows_out, int64_t* stride_out, void* stream) {
    EntryCall c;
    c.who = "xdw_bwd_reduce_stem";
    c.describe("B=%d, frames %d x %d, dtype=%d", B, fH, fW, frames_dtype);
    c.sizes = sizes3(B, fH, fW);
    c.shape = frame_dtype_ok(frames_dtype) && (int64_t)fH * fW * 3 < 0x7fffffffLL;
    c.scratch_what = "scratch"; c.scratch = scratch; c.have = scratch_floats;
    if (c.shaped()) c.need = xdw_stem_scratch(B, fH, fW);
    c.ptrs = frames && w_stem && sc_e && sh_e && mean_e && rstd_e && w_dw && dz_d && rows_out && stride_out;
    RUN(entry_check(c));
    int rows = 0;
    int rc = launch_xdw_bwd_reduce_stem(frames, frames_dtype, B, fH, fW, pixel_scale, w_stem, sc_e, sh_e, mean_e, rstd_e, act_e, w_dw, dz_d, scratch,
                                        &rows, stride_out, (hipStream_t)stream);
    *rows_out = rows;
    return rc;
}
int ams_k_xdw_dwe(const float* G1, const float* xx_g0, int32_t Cin, int32_t Cexp, const float* w_exp, const float* cA, const float* cB,
                  const float* cC, float* dw_exp, void* stream) {
    EntryCall c;
    c.who = "xdw_dwe";
    c.describe("Cin=%d Cexp=%d", Cin, Cexp);
    c.sizes = Cin > 0 && Cexp > 0;
    c.shape = xdw_dwe_shape(Cin, Cexp);
    c.ptrs = G1 && xx_g0 && w_exp && cA && cB && cC && dw_exp;
    RUN(entry_check(c));
    return launch_xdw_dwe(G1, xx_g0, Cin, Cexp, w_exp, cA, cB, cC, dw_exp, (hipStream_t)stream);
}

// ---- the BN pieces of k_elementwise.hip: column reductions, second stages over partial rows, per-channel arithmetic, apply passes, plain folds ----
int ams_k_col_plan(int64_t M, int32_t groups, int32_t C, int32_t* out) {
    AMS_REQUIRE(out, "col_plan: null output");
    return col_plan(M, groups, C, out);
}
size_t ams_k_colstats_scratch(int64_t M, int32_t C) { return colstats_scratch(M, C); }
int ams_k_colstats(const float* z, int64_t M, int32_t C, const float* center, double* sums, float* scratch, size_t scratch_floats, void* stream) {
    AMS_REQUIRE(z && sums && scratch, "colstats: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && scratch_floats >= colstats_scratch(M, C), "colstats: no rows (M=%lld C=%d) or scratch too small (need %zu floats)",
                (long long)M, C, colstats_scratch(M, C));
    return launch_colstats(z, M, C, center, sums, scratch, (hipStream_t)stream);
}
int ams_k_colstats_f64(const float* z, int64_t M, int32_t C, const float* center, double* sums, void* stream) {
    AMS_REQUIRE(z && sums, "colstats_f64: null pointer");
    AMS_REQUIRE(M > 0 && C > 0, "colstats_f64: no rows (M=%lld C=%d)", (long long)M, C);
    return launch_colstats_f64(z, M, C, center, sums, (hipStream_t)stream);
}
int ams_k_colstats_bn(const float* z, int64_t M, int32_t C, const float* center, double* sums, float* scratch, size_t scratch_floats, double n,
                      const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale,
                      float* shift, float* save_mean, float* save_rstd, void* stream) {
    AMS_REQUIRE(z && sums && scratch && gamma && beta && scale && shift, "colstats_bn: null pointer");
    AMS_REQUIRE(!moving_mean == !moving_var && !save_mean == !save_rstd, "colstats_bn: moving_mean / moving_var and save_mean / save_rstd come in pairs");
    AMS_REQUIRE(M > 0 && C > 0 && n >= 1.0 && scratch_floats >= colstats_scratch(M, C),
                "colstats_bn: no rows (M=%lld C=%d n=%g) or scratch too small (need %zu floats)", (long long)M, C, n, colstats_scratch(M, C));
    return launch_colstats_bn(z, M, C, center, sums, scratch, n, gamma, beta, eps, one_minus_decay, moving_mean, moving_var, scale, shift, save_mean,
                              save_rstd, (hipStream_t)stream);
}
int ams_k_bn_finalize(const double* sums, double n, int32_t C, const float* center, const float* gamma, const float* beta, float eps,
                      float one_minus_decay, float* moving_mean, float* moving_var, float* scale, float* shift, float* save_mean, float* save_rstd,
                      void* stream) {
    AMS_REQUIRE(sums && gamma && beta && scale && shift, "bn_finalize: null pointer");
    AMS_REQUIRE(!moving_mean == !moving_var && !save_mean == !save_rstd, "bn_finalize: moving_mean / moving_var and save_mean / save_rstd come in pairs");
    AMS_REQUIRE(C > 0 && n >= 1.0, "bn_finalize: C=%d n=%g", C, n);
    return launch_bn_finalize(sums, n, C, center, gamma, beta, eps, one_minus_decay, moving_mean, moving_var, scale, shift, save_mean, save_rstd,
                              (hipStream_t)stream);
}
// partial rows [rows][2][C], row_stride floats apart (0: dense, 2 * C)
static int partials_shape(const char* who, int rows, int64_t row_stride, int C) {
    AMS_REQUIRE(rows > 0 && C > 0 && (row_stride == 0 || row_stride >= 2 * (int64_t)C), "%s: rows=%d C=%d row_stride=%lld (0 or at least 2 * C)", who, rows,
                C, (long long)row_stride);
    return AMS_OK;
}
int ams_k_bn_fwd_partials(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, double n, const float* center,
                          const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale,
                          float* shift, float* save_mean, float* save_rstd, void* stream) {
    AMS_REQUIRE(part && sums && gamma && beta && scale && shift, "bn_fwd_partials: null pointer");
    AMS_REQUIRE(!moving_mean == !moving_var && !save_mean == !save_rstd, "bn_fwd_partials: moving_mean / moving_var and save_mean / save_rstd come in pairs");
    AMS_REQUIRE(n >= 1.0, "bn_fwd_partials: n=%g", n);
    if (int rc = partials_shape("bn_fwd_partials", rows, row_stride, C)) return rc;
    return launch_bn_fwd_finalize_partials(part, rows, row_stride, C, sums, n, center, gamma, beta, eps, one_minus_decay, moving_mean, moving_var, scale,
                                           shift, save_mean, save_rstd, (hipStream_t)stream);
}
int ams_k_partials_to_sums(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, void* stream) {
    AMS_REQUIRE(part && sums, "partials_to_sums: null pointer");
    if (int rc = partials_shape("partials_to_sums", rows, row_stride, C)) return rc;
    return launch_partials_to_sums(part, rows, row_stride, C, sums, (hipStream_t)stream);
}
int ams_k_bn_bwd_reduce(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* mean,
                        const float* rstd, double* sums, float* scratch, size_t scratch_floats, void* stream) {
    AMS_REQUIRE(da && z && scale && shift && mean && rstd && sums && scratch, "bn_bwd_reduce: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && scratch_floats >= colstats_scratch(M, C), "bn_bwd_reduce: no rows (M=%lld C=%d) or scratch too small (need %zu floats)",
                (long long)M, C, colstats_scratch(M, C));
    return launch_bn_bwd_reduce(da, z, M, C, scale, shift, act, mean, rstd, sums, scratch, (hipStream_t)stream);
}
int ams_k_bn_bwd_reduce_coef(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act,
                             const float* mean, const float* rstd, double* sums, float* scratch, size_t scratch_floats, double n, const float* gamma,
                             float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, void* stream) {
    AMS_REQUIRE(da && z && scale && shift && mean && rstd && sums && scratch && gamma && coefA && coefB && coefC && dgamma && dbeta,
                "bn_bwd_reduce_coef: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && n >= 1.0 && scratch_floats >= colstats_scratch(M, C),
                "bn_bwd_reduce_coef: no rows (M=%lld C=%d n=%g) or scratch too small (need %zu floats)", (long long)M, C, n, colstats_scratch(M, C));
    return launch_bn_bwd_reduce_coef(da, z, M, C, scale, shift, act, mean, rstd, sums, scratch, n, gamma, coefA, coefB, coefC, dgamma, dbeta,
                                     (hipStream_t)stream);
}
int ams_k_bn_bwd_partials(const float* part, int32_t rows, int64_t row_stride, int32_t C, double* sums, double n, const float* gamma, const float* mean,
                          const float* rstd, float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, void* stream) {
    AMS_REQUIRE(part && sums && gamma && mean && rstd && coefA && coefB && coefC && dgamma && dbeta, "bn_bwd_partials: null pointer");
    AMS_REQUIRE(n >= 1.0, "bn_bwd_partials: n=%g", n);
    if (int rc = partials_shape("bn_bwd_partials", rows, row_stride, C)) return rc;
    return launch_bn_bwd_finalize_partials(part, rows, row_stride, C, sums, n, gamma, mean, rstd, coefA, coefB, coefC, dgamma, dbeta, (hipStream_t)stream);
}
int ams_k_bn_bwd_coef(const double* sums, double n, int32_t C, const float* gamma, const float* mean, const float* rstd, float* coefA, float* coefB,
                      float* coefC, float* dgamma, float* dbeta, void* stream) {
    AMS_REQUIRE(sums && gamma && mean && rstd && coefA && coefB && coefC, "bn_bwd_coef: null pointer");
    AMS_REQUIRE(!dgamma == !dbeta, "bn_bwd_coef: dgamma and dbeta come as a pair");
    AMS_REQUIRE(C > 0 && n >= 1.0, "bn_bwd_coef: C=%d n=%g", C, n);
    return launch_bn_bwd_coef(sums, n, C, gamma, mean, rstd, coefA, coefB, coefC, dgamma, dbeta, (hipStream_t)stream);
}
int ams_k_bn_param_grads(const double* sums, int32_t C, float* dgamma, float* dbeta, void* stream) {
    AMS_REQUIRE(sums && dgamma && dbeta, "bn_param_grads: null pointer");
    AMS_REQUIRE(C > 0, "bn_param_grads: C=%d", C);
    return launch_bn_param_grads(sums, C, dgamma, dbeta, (hipStream_t)stream);
}
int ams_k_bn_act(const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* res, float* a, void* stream) {
    AMS_REQUIRE(z && scale && shift && a, "bn_act: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && act >= AMS_ACT_NONE && act <= AMS_ACT_RELU6, "bn_act: M=%lld C=%d act=%d", (long long)M, C, act);
    return launch_bn_act(z, M, C, scale, shift, act, res, a, (hipStream_t)stream);
}
int ams_k_bn_bwd_apply(const float* da, const float* z, int64_t M, int32_t C, const float* scale, const float* shift, int32_t act, const float* coefA,
                       const float* coefB, const float* coefC, float* dz, void* stream) {
    AMS_REQUIRE(da && z && scale && shift && coefA && coefB && coefC && dz, "bn_bwd_apply: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && act >= AMS_ACT_NONE && act <= AMS_ACT_RELU6, "bn_bwd_apply: M=%lld C=%d act=%d", (long long)M, C, act);
    return launch_bn_bwd_apply(da, z, M, C, scale, shift, act, coefA, coefB, coefC, dz, (hipStream_t)stream);
}
int ams_k_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int32_t C, float* scale, float* shift,
                  void* stream) {
    AMS_REQUIRE(gamma && beta && mean && var && scale && shift, "bn_fold: null pointer");
    AMS_REQUIRE(C > 0, "bn_fold: C=%d", C);
    return launch_bn_fold(gamma, beta, mean, var, eps, C, scale, shift, (hipStream_t)stream);
}
int ams_k_reduce_splits(const float* part, int32_t splits, int64_t n, int64_t stride, float* out, void* stream) {
    AMS_REQUIRE(part && out, "reduce_splits: null pointer");
    AMS_REQUIRE(splits > 0 && n > 0 && stride >= n, "reduce_splits: splits=%d n=%lld stride=%lld (at least n)", splits, (long long)n, (long long)stride);
    return launch_reduce_splits(part, splits, n, out, (hipStream_t)stream, stride);
}
int ams_k_reduce_batch(const float* const* part, const int32_t* splits, const int64_t* count, const int64_t* stride, float* const* out, int32_t n_jobs,
                       void* stream) {
    AMS_REQUIRE(part && splits && count && stride && out, "reduce_batch: null pointer");
    AMS_REQUIRE(n_jobs > 0 && n_jobs <= ReduceJobs::kMax, "reduce_batch: %d jobs (1..%d)", n_jobs, ReduceJobs::kMax);
    ReduceJobs jobs;
    for (int j = 0; j < n_jobs; ++j) {
        AMS_REQUIRE(part[j] && out[j] && splits[j] > 0 && count[j] > 0 && stride[j] >= count[j], "reduce_batch: job %d: null pointer, or splits=%d count=%lld stride=%lld",
                    j, splits[j], (long long)count[j], (long long)stride[j]);
        jobs.add(part[j], splits[j], count[j], out[j], stride[j]);
    }
    return launch_reduce_batch(jobs, (hipStream_t)stream);
}
size_t ams_k_colsum_scratch(int32_t C) { return colsum_scratch(C); }
int ams_k_colsum(const float* x, int64_t M, int32_t C, int32_t ldx, float* out, float* scratch, size_t scratch_floats, void* stream) {
    AMS_REQUIRE(x && out && scratch, "colsum: null pointer");
    AMS_REQUIRE(M > 0 && C > 0 && ldx >= C && scratch_floats >= colsum_scratch(C), "colsum: M=%lld C=%d ldx=%d, or scratch too small (need %zu floats)",
                (long long)M, C, ldx, colsum_scratch(C));
    return launch_colsum(x, M, C, ldx, out, scratch, (hipStream_t)stream);
}
size_t ams_k_image_colsum_scratch(int32_t B, int32_t C) { return image_colsum_scratch(B, C); }
int ams_k_image_colsum(const float* x, int32_t B, int64_t HW, int32_t C, int32_t ldx, float* out, float* scratch, size_t scratch_floats, void* stream) {
    AMS_REQUIRE(x && out && scratch, "image_colsum: null pointer");
    AMS_REQUIRE(B > 0 && HW > 0 && C > 0 && ldx >= C && scratch_floats >= image_colsum_scratch(B, C),
                "image_colsum: B=%d HW=%lld C=%d ldx=%d, or scratch too small (need %zu floats)", B, (long long)HW, C, ldx, image_colsum_scratch(B, C));
    return launch_image_colsum(x, B, HW, C, ldx, out, scratch, (hipStream_t)stream);
}

int ams_k_l2_regularizer(const float* params, float* grads, const uint8_t* mask, int64_t n, int32_t n_vars, float coef, double* scratch,
                         size_t scratch_doubles, double* loss, void* stream) {
    AMS_REQUIRE(n > 0 && scratch_doubles >= 256, "l2_regularizer: n=%lld, or scratch too small (need 256 doubles)", (long long)n);
    return launch_l2_regularizer(params, grads, mask, n, n_vars, coef, scratch, loss, (hipStream_t)stream);
}

int ams_k_adam(float* params, const float* grads, float* m, float* v, const uint8_t* mask, int64_t n, float lr_t, float beta1,
               float beta2, float eps, void* stream) {
    return launch_adam(params, grads, m, v, mask, n, lr_t, beta1, beta2, eps, (hipStream_t)stream);
}

}  // extern "C"

