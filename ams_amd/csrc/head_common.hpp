// Geometry and interpolation arithmetic shared by the output-head kernels (k_head.hip, k_confidence.hip, k_soft_metric.hip): every kernel that walks the
// full-resolution pixels forms a pixel's K interpolated logits with these functions, in this order, so they all see the same bits.
#pragma once
#include "kernels.hpp"
#include "cross_conf.hpp"
#include <cmath>
#include <type_traits>

namespace ams {

struct HeadGeom {
    int B, h, w, ld, K, H, W, NC;
    int per_frame;         // metrics per frame: conf [B][K][K], loss [B][2] instead of the batch totals
    int labels_u8;         // the label map as uint8 [B][H][W] through the same pointer (K <= 32 fits a byte: a quarter of the device -> host bytes)
    float sy, sx;          // (h-1)/(H-1), (w-1)/(W-1) as f32 (TF: CalculateResizeScale with align_corners)
};

__device__ __forceinline__ void src_tap(int dst, float scale, int n_in, int& lo, int& hi, float& t) {
    const float src = __fmul_rn((float)dst, scale);
    const float fl = floorf(src);
    lo = (int)fl;
    hi = lo + 1 < n_in ? lo + 1 : n_in - 1;
    t = __fsub_rn(src, fl);
}

// v = top + (bot - top) * ty,  top = tl + (tr - tl) * tx   (unfused, like the TF CPU kernel / the oracle)
__device__ __forceinline__ float bilerp(float tl, float tr, float bl, float br, float tx, float ty) {
    const float top = __fadd_rn(tl, __fmul_rn(__fsub_rn(tr, tl), tx));
    const float bot = __fadd_rn(bl, __fmul_rn(__fsub_rn(br, bl), tx));
    return __fadd_rn(top, __fmul_rn(__fsub_rn(bot, top), ty));
}

// the scale of an align-corners resize of n_in samples to n_out, as f32 (TF: CalculateResizeScale with align_corners)
static inline float align_corners_scale(int n_in, int n_out) { return n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0.f; }

static inline HeadGeom head_geom(int ld, int B, int h, int w, int K, int H, int W, int NC) {
    HeadGeom g;
    g.B = B; g.h = h; g.w = w; g.ld = ld; g.K = K; g.H = H; g.W = W; g.NC = NC; g.per_frame = 0; g.labels_u8 = 0;
    g.sy = align_corners_scale(h, H);
    g.sx = align_corners_scale(w, W);
    return g;
}

// Soft-teacher targets (create_student_v3 with soft_teacher=True, utils/graph_utils.py:359, 375-376, 403-404): teacher logits
// [B][th][tw][ld] f32 fed through teacher_labels_logits_pl; the target of a pixel is softmax(gather(teacher_logits, class_weights)).  th x tw is
// either the label size (the reference's feed: the loss needs the shape of filtered_logits) or any smaller grid, which is then interpolated
// to H x W exactly as the student's own logits are (align corners) — at th == H, tw == W that interpolation is the identity, bit for bit.
//
// Two layouts of a teacher pixel (AMS_TLOGITS_*): FULL, ld = NC floats of which channel ct.idx[k] is class k's; SELECTED, ld = K floats, channel k
// holding what the full layout holds at ct.idx[k] (what a replay memory built with logits_select caches).  tidx[k] is class k's channel
// in whichever layout is fed: the kernels are the same instantiations for both, so the same values meet the same instructions.
struct SoftTeacher {
    const float* t;
    int th, tw, ld;
    float sy, sx;
    int tidx[kMaxK];
};

// The soft step's two KD knobs, by value beside SoftTeacher (ce_loss_grad_kernel<K, SOFT, KD>): 1 / T, alpha T^2, alpha T, 1 - alpha
struct KdParams { float inv_t, at2, at, om; };

// T finite and > 0 with 1 / T and T^2 finite in f32 as well, alpha in [0, 1]: checked before anything else of a call is looked at
static inline int kd_params_check(const char* who, float temperature, float alpha) {
    AMS_REQUIRE(std::isfinite(temperature) && temperature > 0.f && std::isfinite(1.f / temperature) && std::isfinite(temperature * temperature),
                "%s: temperature %g must be finite and > 0", who, (double)temperature);
    AMS_REQUIRE(alpha >= 0.f && alpha <= 1.f, "%s: alpha %g must lie in [0, 1]", who, (double)alpha);
    return AMS_OK;
}

// The weighted loss's two knobs (ce_loss_grad_kernel<K, SOFT, KD, WT = true>), by value beside KdParams: pk[label byte] = rint(cw_k 2^20) << 5 | k for the label's class k (the QUANTISED class weight,
// at most 2^24, over the subset index that ct.lut holds), 0 for a label outside the subset or of weight 0; gamma, the exponent of the teacher's confidence.
struct LossWeights { uint32_t pk[256]; float gamma; };
struct NoLossWeights {};               // what the WT = false forms take in its place: nothing

// class_weights (HOST, K floats, or NULL = ones): each 0 or in [2^-6, 16]; gamma finite in [0, 8]: checked before anything else of a call is looked at
static inline int loss_weights_check(const char* who, const float* cw, int n, int K, float gamma) {
    AMS_REQUIRE(std::isfinite(gamma) && gamma >= 0.f && gamma <= 8.f, "%s: conf_gamma %g must lie in [0, 8]", who, (double)gamma);
    if (!cw) return AMS_OK;
    AMS_REQUIRE(n == K && K >= 1 && K <= kMaxK, "%s: %d class weights for %d selected classes", who, n, K);
    for (int k = 0; k < K; ++k)
        AMS_REQUIRE(cw[k] == 0.f || (cw[k] >= 0.015625f && cw[k] <= 16.f), "%s: class_weights[%d] = %g must be 0 or lie in [2^-6, 16]", who, k, (double)cw[k]);
    return AMS_OK;
}

static inline bool loss_weights_default(const float* cw, int K, float gamma) {
    if (gamma != 0.f) return false;
    if (cw) for (int k = 0; k < K; ++k) if (cw[k] != 1.f) return false;
    return true;
}

// ct: the filled class table; cw checked (loss_weights_check).  rintf(cw 2^20) is exact in f32 for cw <= 16 (<= 2^24)
static inline void fill_loss_weights(const ClassTable& ct, const float* cw, int K, float gamma, LossWeights* lw) {
    for (int i = 0; i < 256; ++i) {
        const int k = ct.lut[i];
        const uint32_t q = k < 0 || k >= K ? 0u : (uint32_t)rintf((cw ? cw[k] : 1.f) * 1048576.f);
        lw->pk[i] = q ? q << 5 | (uint32_t)k : 0u;
    }
    lw->gamma = gamma;
}

static inline bool tlogits_layout_ok(int layout) { return layout == AMS_TLOGITS_FULL || layout == AMS_TLOGITS_SELECTED; }

// ---- one head call, as the host describes it (every head launcher, the ams_k_* head and loss entries, the student: student_head_call) ----
// The head call: whose logits against which labels
struct HeadCall {
    const float* logits = nullptr;     // [B][h][w][ld] f32, the student's
    int ld = 0, B = 0, h = 0, w = 0;
    const int32_t* cls = nullptr;      // HOST, the K selected classes' ids
    int K = 0;
    int H = 0, W = 0;
    const uint8_t* teacher = nullptr;  // the teacher's labels [B][H][W]
    int NC = 0;
};

// What every head launcher refuses first, in this order, and what it gets in return: the class table and the geometry of the call.  After it
// come the launcher's own conditions and, last, in front of its first memset or launch, the null checks of the pointers it reads.
static inline int head_call_check(const char* who, const HeadCall& c, ClassTable* ct, HeadGeom* g) {
    AMS_REQUIRE(c.cls, "%s: null class table", who);
    AMS_REQUIRE(c.K > 0 && c.K <= kMaxK, "%s: K=%d out of range (1..%d)", who, c.K, kMaxK);
    for (int i = 0; i < 256; ++i) ct->lut[i] = -1;
    for (int k = 0; k < kMaxK; ++k) ct->idx[k] = 0;
    for (int k = 0; k < c.K; ++k) {
        AMS_REQUIRE(c.cls[k] >= 0 && c.cls[k] < c.NC && c.cls[k] < 256, "%s: class id %d out of range", who, c.cls[k]);
        ct->idx[k] = c.cls[k];
        ct->lut[c.cls[k]] = k;
    }
    AMS_REQUIRE(c.B > 0 && c.h > 0 && c.w > 0 && c.H > 0 && c.W > 0, "%s: no pixels: B=%d, %d x %d -> %d x %d", who, c.B, c.h, c.w, c.H, c.W);
    AMS_REQUIRE(c.ld >= c.NC, "%s: row stride %d below %d classes", who, c.ld, c.NC);
    *g = head_geom(c.ld, c.B, c.h, c.w, c.K, c.H, c.W, c.NC);
    return AMS_OK;
}

// The objective: what the loss of a pixel is.  The defaults are the reference's hard loss.
struct LossObjective {
    // != nullptr: soft-teacher targets, teacher logits [B][th][tw][NC] f32 (utils/graph_utils.py:375-376, 403-404; SoftTeacher above), th x tw at most the
    // label size; layout AMS_TLOGITS_FULL, or AMS_TLOGITS_SELECTED = [B][th][tw][K], channel k holding class cls[k]'s logit
    const float* teacher_logits = nullptr;
    int th = 0, tw = 0, layout = AMS_TLOGITS_FULL;
    // T, alpha (used with teacher logits only; checked always): softmax(./T) on both logit sets with the T^2 factor, mixed alpha : 1 - alpha with the
    // hard-label CE (k_head.hip KD); (1, 1) launches the soft kernel and alpha = 0 the hard one, as without them
    float temperature = 1.f, alpha = 1.f;
    // class_weights (HOST, K floats in the order of cls, nullptr = ones), conf_gamma (needs teacher logits when > 0; both checked always): per-pixel weight
    // cw_y max_k p_k ^ gamma and a weighted mean, loss[1] = sum of the weights (k_head.hip WT); all ones with gamma = 0 launch the kernels as without them
    const float* class_weights = nullptr;
    float conf_gamma = 0.f;
    // the student's switch (AMS_OPT_SOFT_TEACHER): its step goes by objective_of_step below; the kernel-level entries go by teacher_logits alone
    int soft_teacher = 0;
};

// soft off: no teacher logits, T = alpha = 1, whatever was fed or set (the weights stay)
static inline LossObjective objective_of_step(LossObjective o) {
    if (!o.soft_teacher) { o.teacher_logits = nullptr; o.temperature = o.alpha = 1.f; }
    return o;
}

// the class tier of the one-pass loss kernels' instantiations
static inline int ce_kmax(int K) { return K <= 8 ? 8 : K <= 20 ? 20 : 32; }

// Which ce_loss_grad_kernel<KMAX, SOFT, KD, WT> an objective runs, and that form's name for the profiler.  (T, alpha) = (1, 1) is the soft form and
// alpha = 0 the hard one, the same launches as without the two parameters, so those cases are the same bits by construction; all-ones class
// weights with gamma = 0 go to the WT = false forms, which are compiled from the code as it was.
struct LossForm { bool soft; int kd; bool weighted; const char* name; };
static inline LossForm loss_form(const LossObjective& o, int K) {
    static const char* const names[2][4] = {
        {"ce_loss_grad_kernel", "ce_loss_grad_kernel<soft>", "ce_loss_grad_kernel<soft, T>", "ce_loss_grad_kernel<soft, mix>"},
        {"ce_loss_grad_kernel<weighted>", "ce_loss_grad_kernel<soft, weighted>", "ce_loss_grad_kernel<soft, T, weighted>", "ce_loss_grad_kernel<soft, mix, weighted>"}};
    const bool weighted = !loss_weights_default(o.class_weights, K, o.conf_gamma);
    int kd = !o.teacher_logits || o.alpha == 0.f ? -1 : o.alpha == 1.f ? (o.temperature == 1.f ? 0 : 1) : 2;
    // gamma > 0 with alpha = 0: the hard form has no teacher distribution, the mix form computes p anyway (alpha T^2 = alpha T = 0, 1 - alpha = 1)
    if (kd < 0 && weighted && o.conf_gamma > 0.f) kd = 2;
    return LossForm{kd >= 0, kd < 0 ? 0 : kd, weighted, names[weighted][kd + 1]};
}

// ct: the filled class table of the K selected classes (fill_class_table)
static inline SoftTeacher soft_teacher_geom(const float* t, int th, int tw, int layout, const ClassTable& ct, int K, int NC, int H, int W) {
    SoftTeacher s;
    const bool selected = layout == AMS_TLOGITS_SELECTED;
    s.t = t; s.th = th; s.tw = tw; s.ld = selected ? K : NC;
    s.sy = align_corners_scale(th, H);                              // as head_geom does for the student's own logits
    s.sx = align_corners_scale(tw, W);
    for (int k = 0; k < kMaxK; ++k) s.tidx[k] = k < K ? (selected ? k : ct.idx[k]) : 0;
    return s;
}

// the grid of the kernels that walk down columns: (column strips of 256, row bands, frames).  32 bands per column strip and image, fewer
// rows per band when that leaves the chip short of blocks
static inline dim3 head_band_grid(int B, int H, int W) {
    int rows_y = H < 32 ? H : 32;
    while (rows_y < H && (int64_t)cdiv(W, 256) * rows_y * B < 2048) rows_y *= 2;
    if (rows_y > H) rows_y = H;
    return dim3(cdiv(W, 256), rows_y, B);
}

}  // namespace ams
