// Evaluation of the soft-teacher objective (create_student_v3 with soft_teacher=True, reference utils/graph_utils.py:265-317, 375-376,
// 397, 403-408) without an optimisation step: per full-resolution pixel the teacher's distribution p = softmax(gather(teacher logits)) over
// the K selected classes and the pixel's soft cross-entropy ce = sum_k p_k (logsumexp(z) - z_k) against the student's interpolated logits
// z.  The kernel walks the pixels exactly as upsample_argmax_kernel does (k_head.hip: same geometry, same interpolation arithmetic in the
// same order, so the argmax it derives is that kernel's label bit for bit); the teacher logits come at the label size or on a smaller
// grid that is interpolated like the student's own (the extension ce_loss_grad_kernel<K, SOFT> documents).  Next to the two maps it
// leaves one row of integer statistics per frame: the summed ce and the two probabilistic confusion matrices prob_confmat (student
// labels against p) and prob_confmat_star (the teacher's own hard labels against p).
#include "head_common.hpp"

namespace ams {

// row layout (int64): valid_cnt | ce_sum | M_stu[K * K] | M_star[K * K],  M[c * K + i]: probability class c, label i
int soft_metric_stats_len(int K) { return 2 + 2 * K * K; }

// a thread's column sums are 32-bit: rows of a band x 2^20 must stay below 2^31
constexpr int kSoftMaxBandRows = 2047;

// KMAX > 0: K <= KMAX, the student's two horizontally interpolated source rows and a pixel's z and t live in registers.  KMAX = 0: any
// K <= kMaxK; z and t are formed twice per pixel (the second time from the cache) instead of being kept.
//
// Counting: a valid pixel adds its K fixed-point probabilities to ONE column of each matrix, and the pixels a thread meets walking down
// its column mostly share that column.  So a thread sums them in K registers per matrix for as long as the column stays the same and
// hands the K sums to the block's LDS matrix when it changes and at the end of the band: K LDS atomics per run of equal labels instead
// of K per pixel.  Everything is an integer, so the sums do not depend on how pixels are dealt to threads, blocks or batches.
template <int KMAX>
__global__ __launch_bounds__(256) void upsample_soft_metric_kernel(const float* __restrict__ logits, HeadGeom g, ClassTable ct,
                                                                   const uint8_t* __restrict__ teacher, SoftTeacher sft,
                                                                   unsigned long long* __restrict__ stats, float* __restrict__ p_f32,
                                                                   float* __restrict__ ce_f32) {
    constexpr int KA = KMAX > 0 ? KMAX : kMaxK;
    __shared__ unsigned long long s_m[2 * kMaxK * kMaxK];
    __shared__ double s_ce[4];
    __shared__ int s_cnt[4];
    const bool want_stats = stats != nullptr;
    const bool masked = teacher != nullptr;
    const bool want_maps = p_f32 != nullptr || ce_f32 != nullptr;
    const int KK = g.K * g.K;
    if (want_stats) {
        for (int e = threadIdx.x; e < 2 * KK; e += blockDim.x) s_m[e] = 0;
        __syncthreads();
    }
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    double my_ce = 0.0;                      // integer multiples of 2^-20 per pixel, held in f64: exact
    int my_cnt = 0;
    int acc_s[KA], acc_t[KA];                // the running column of M_stu / M_star: sum of rint(p_k * 2^20) per probability class k
#pragma unroll
    for (int k = 0; k < KA; ++k) { acc_s[k] = 0; acc_t[k] = 0; }
    int cur_s = -1, cur_t = -1;
    auto flush = [&](int (&acc)[KA], int col, int plane) {
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            if (k < g.K && acc[k] != 0) atomicAdd(&s_m[plane * KK + k * g.K + col], (unsigned long long)(long long)acc[k]);
            acc[k] = 0;
        }
    };
    int x0 = 0, x1 = 0; float tx = 0.f;
    int qx0 = 0, qx1 = 0; float qtx = 0.f;
    if (x < g.W) {
        src_tap(x, g.sx, g.w, x0, x1, tx);
        src_tap(x, sft.sx, sft.tw, qx0, qx1, qtx);
    }
    const float* base = logits + (int64_t)b * g.h * g.w * g.ld;
    const float* qbase = sft.t + (int64_t)b * sft.th * sft.tw * sft.ld;
    const int band = (g.H + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ybeg = blockIdx.y * band, yend = ybeg + band < g.H ? ybeg + band : g.H;
    constexpr int KR = KMAX > 0 ? KMAX : 1;
    float top[KR], bot[KR];
    int cur_y0 = -1;
    for (int y = ybeg; y < yend; ++y) {
        if (x >= g.W) break;
        int y0, y1; float ty;
        src_tap(y, g.sy, g.h, y0, y1, ty);
        const float* ptl = base + ((int64_t)y0 * g.w + x0) * g.ld;
        const float* ptr = base + ((int64_t)y0 * g.w + x1) * g.ld;
        const float* pbl = base + ((int64_t)y1 * g.w + x0) * g.ld;
        const float* pbr = base + ((int64_t)y1 * g.w + x1) * g.ld;
        if (KMAX > 0 && y0 != cur_y0) {               // block-uniform (one output row per iteration)
            cur_y0 = y0;
#pragma unroll
            for (int k = 0; k < KR; ++k) {
                const int c = ct.idx[k < g.K ? k : 0];
                top[k] = __fadd_rn(ptl[c], __fmul_rn(__fsub_rn(ptr[c], ptl[c]), tx));
                bot[k] = __fadd_rn(pbl[c], __fmul_rn(__fsub_rn(pbr[c], pbl[c]), tx));
            }
        }
        const int64_t pix = ((int64_t)b * g.H + y) * g.W + x;
        int target = -1;
        if (masked) target = ct.lut[teacher[pix]];
        const bool valid = !masked || target >= 0;    // weight != 0: the hard teacher id is in the subset
        if (!(want_stats && valid) && !want_maps) continue;
        // the teacher's taps (ce_loss_grad_kernel<K, SOFT>'s: on a grid point, always at the label size, the logit itself)
        int qy0, qy1; float qty;
        src_tap(y, sft.sy, sft.th, qy0, qy1, qty);
        const float* qtl = qbase + ((int64_t)qy0 * sft.tw + qx0) * sft.ld;
        const float* qtr = qbase + ((int64_t)qy0 * sft.tw + qx1) * sft.ld;
        const float* qbl = qbase + ((int64_t)qy1 * sft.tw + qx0) * sft.ld;
        const float* qbr = qbase + ((int64_t)qy1 * sft.tw + qx1) * sft.ld;
        const bool on_grid = qty == 0.f && qtx == 0.f;
        auto student = [&](int k) -> float {
            if constexpr (KMAX > 0) return __fadd_rn(top[k], __fmul_rn(__fsub_rn(bot[k], top[k]), ty));
            const int c = ct.idx[k];
            return bilerp(ptl[c], ptr[c], pbl[c], pbr[c], tx, ty);
        };
        auto teach = [&](int k) -> float {
            const int c = sft.tidx[k];
            return on_grid ? qtl[c] : bilerp(qtl[c], qtr[c], qbl[c], qbr[c], qtx, qty);
        };
        // pass 1: the argmax (first maximum wins, tf.argmax) and both streaming log-sum-exps, as the loss path of upsample_argmax_kernel:
        // keep the running max, rescale the running sum
        float zk[KR], tk[KR];
        float best = 0.f, zmax = 0.f, ssum = 0.f, tmax = 0.f, tsum = 0.f;
        int arg = 0;
#pragma unroll
        for (int k = 0; k < KA; ++k) {
            if (k >= g.K) continue;
            const float v = student(k), t = teach(k);
            if constexpr (KMAX > 0) { zk[k] = v; tk[k] = t; }
            if (k == 0 || v > best) { best = v; arg = k; }
            if (k == 0) { zmax = v; ssum = 1.f; }
            else if (v > zmax) { ssum = ssum * __expf(zmax - v) + 1.f; zmax = v; }
            else ssum += __expf(v - zmax);
            if (k == 0) { tmax = t; tsum = 1.f; }
            else if (t > tmax) { tsum = tsum * __expf(tmax - t) + 1.f; tmax = t; }
            else tsum += __expf(t - tmax);
        }
        const float lse = zmax + __logf(ssum);
        const float rp = 1.f / tsum;
        // a NaN (or an infinity that makes one) in either vector leaves lse or tsum not finite: the pixel is counted and adds nothing else
        const bool count = want_stats && valid;
        const bool add = count && lse - lse == 0.f && tsum - tsum == 0.f;
        if (count) my_cnt += 1;
        if (add) {
            if (arg != cur_s) { if (cur_s >= 0) flush(acc_s, cur_s, 0); cur_s = arg; }
            if (masked && target != cur_t) { if (cur_t >= 0) flush(acc_t, cur_t, 1); cur_t = target; }
        }
        // pass 2: p_k = exp(t_k - tmax) / tsum and ce = sum_k p_k (lse - z_k); sign: what the pixel's fixed-point p adds to the columns
        auto second = [&](int sign, bool store) -> float {
            float ce = 0.f;
#pragma unroll
            for (int k = 0; k < KA; ++k) {
                if (k >= g.K) continue;
                float v, t;
                if constexpr (KMAX > 0) { v = zk[k]; t = tk[k]; } else { v = student(k); t = teach(k); }
                const float p = __expf(t - tmax) * rp;
                ce += p * (lse - v);
                if (store && p_f32) p_f32[pix * g.K + k] = p;
                if (sign != 0) {
                    const int pf = sign * (int)rint((double)p * 1048576.0);
                    acc_s[k] += pf;
                    if (masked) acc_t[k] += pf;
                }
            }
            return ce;
        };
        const float ce = second(add ? 1 : 0, true);
        if (ce_f32) ce_f32[pix] = ce;
        if (add) {
            // finite logits can still leave a loss that is not (z_k = -inf under p_k > 0; a difference beyond the f32 range): no conversion of
            // such a value to an integer, and the pixel's p leave the columns again (integers: exactly)
            if (ce - ce == 0.f) my_ce += rint((double)ce * 1048576.0);
            else second(-1, false);
        }
    }
    if (!want_stats) return;
    if (cur_s >= 0) flush(acc_s, cur_s, 0);
    if (cur_t >= 0) flush(acc_t, cur_t, 1);
    my_ce = wave_sum(my_ce);
    my_cnt = (int)wave_sum((float)my_cnt);       // <= 64 x 2047: exact in f32
    if ((threadIdx.x & 63) == 0) { s_ce[threadIdx.x >> 6] = my_ce; s_cnt[threadIdx.x >> 6] = my_cnt; }
    __syncthreads();
    unsigned long long* row = stats + (size_t)b * (2 + 2 * KK);
    for (int e = threadIdx.x; e < 2 * KK; e += blockDim.x)
        if (s_m[e]) atomicAdd(&row[2 + e], s_m[e]);
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        double ce = 0.0; int cn = 0;
        for (int i = 0; i < nw; ++i) { ce += s_ce[i]; cn += s_cnt[i]; }
        if (cn) atomicAdd(&row[0], (unsigned long long)cn);
        if (ce != 0.0) atomicAdd(&row[1], (unsigned long long)(long long)ce);
    }
}

// o: the teacher logits, their grid and their layout (nothing else of it is read).  Every output pointer may be null: nothing is written there.
// A refused call writes nothing.
int launch_upsample_soft_metric(const HeadCall& c, const LossObjective& o, int64_t* stats, float* p_f32, float* ce_f32, hipStream_t st) {
    ClassTable ct;
    HeadGeom g;
    if (int rc = head_call_check("soft_metric", c, &ct, &g)) return rc;
    AMS_REQUIRE(tlogits_layout_ok(o.layout), "soft_metric: unknown teacher-logit layout %d", o.layout);
    AMS_REQUIRE(o.th >= 1 && o.tw >= 1 && o.th <= c.H && o.tw <= c.W, "soft_metric: teacher logits of %d x %d for labels of %d x %d", o.th, o.tw, c.H, c.W);
    const dim3 grid = head_band_grid(c.B, c.H, c.W);
    AMS_REQUIRE(cdiv(c.H, (int)grid.y) <= kSoftMaxBandRows, "soft_metric: %d rows per band overflow a thread's column sums", cdiv(c.H, (int)grid.y));
    AMS_REQUIRE(c.logits && o.teacher_logits, "soft_metric: null pointer");
    const SoftTeacher sft = soft_teacher_geom(o.teacher_logits, o.th, o.tw, o.layout, ct, c.K, c.NC, c.H, c.W);
    if (stats) AMS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int64_t) * soft_metric_stats_len(c.K) * c.B, st));
    note_kernel("upsample_soft_metric_kernel");
    if (c.K <= 8)
        hipLaunchKernelGGL(upsample_soft_metric_kernel<8>, grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, sft, (unsigned long long*)stats, p_f32, ce_f32);
    else
        hipLaunchKernelGGL(upsample_soft_metric_kernel<0>, grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, sft, (unsigned long long*)stats, p_f32, ce_f32);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
