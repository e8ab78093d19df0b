// The student's own certainty (create_student_v3's probabilities_reduced, reference utils/graph_utils.py:388-389): per full-resolution
// pixel the maximum of the softmax over the K selected classes, p = 1 / sum_k exp(z_k - z_max).  The kernel walks the pixels exactly as
// upsample_argmax_kernel does (k_head.hip: same geometry, same interpolation arithmetic in the same order, so the argmax it derives is
// that kernel's label bit for bit) and the full-resolution logits are never materialised.  Next to the map it leaves one row of integer
// statistics per frame: the histogram of p and, against teacher labels, the reliability curve (pixels, hits and summed confidence per
// bin) and the sums of the selective loss (loss_sel, utils/graph_utils.py:410-418).
#include "head_common.hpp"

namespace ams {

// row layout (int64): hist[NB] | hist_valid[NB] | hist_hit[NB] | bin_sum[NB] | sel_cnt[kMaxK] | sel_sum[kMaxK] | sum_all
constexpr int kConfNB = AMS_CONFIDENCE_BINS;
constexpr int kConfOffSelCnt = 4 * kConfNB;
constexpr int kConfOffSelSum = kConfOffSelCnt + kMaxK;
constexpr int kConfOffSumAll = kConfOffSelSum + kMaxK;
constexpr int kConfStatsLen = kConfOffSumAll + 1;
// the three pixel counts of a bin share one 64-bit LDS word while they are a block's: 21 bits each
constexpr int kConfPackBits = 21;

int confidence_stats_len() { return kConfStatsLen; }

template <int KMAX>
__global__ __launch_bounds__(256) void upsample_confidence_kernel(const float* __restrict__ logits, HeadGeom g, ClassTable ct,
                                                                  const uint8_t* __restrict__ teacher, uint8_t* __restrict__ conf_u8,
                                                                  float* __restrict__ conf_f32, unsigned long long* __restrict__ stats) {
    // Everything a block adds up is an integer (counts; p and the pixel loss as multiples of 2^-20), so every sum is exact and does not
    // depend on how pixels are dealt to threads, blocks or batches: a frame's row is the same bits in a one-frame call and inside an N-frame one.
    __shared__ unsigned long long s_bins[kConfNB];        // hist | hist_valid << 21 | hist_hit << 42
    __shared__ unsigned long long s_bin_sum[kConfNB];
    __shared__ unsigned long long s_sel_sum[kMaxK];
    __shared__ int s_sel_cnt[kMaxK];
    __shared__ double s_all[4];
    const bool want_stats = stats != nullptr;
    const bool metric = teacher != nullptr;
    if (want_stats) {
        for (int e = threadIdx.x; e < kConfNB; e += blockDim.x) { s_bins[e] = 0; s_bin_sum[e] = 0; }
        for (int e = threadIdx.x; e < kMaxK; e += blockDim.x) { s_sel_sum[e] = 0; s_sel_cnt[e] = 0; }
        __syncthreads();
    }
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    double my_all = 0.0;                     // sum of the fixed-point p over this thread's pixels (integers in f64: exact)
    int x0 = 0, x1 = 0; float tx = 0.f;
    if (x < g.W) src_tap(x, g.sx, g.w, x0, x1, tx);
    const float* base = logits + (int64_t)b * g.h * g.w * g.ld;
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
        if (metric) target = ct.lut[teacher[pix]];
        float best = 0.f, zt = 0.f, zmax = 0.f, ssum = 0.f;
        int arg = 0;
        auto visit = [&](int k, float v) {
            if (k == 0 || v > best) { best = v; arg = k; }        // first maximum wins (tf.argmax)
            // streaming log-sum-exp, as the loss path of upsample_argmax_kernel: keep the running max, rescale the running sum
            if (k == 0) { zmax = v; ssum = 1.f; }
            else if (v > zmax) { ssum = ssum * __expf(zmax - v) + 1.f; zmax = v; }
            else ssum += __expf(v - zmax);
            if (k == target) zt = v;
        };
        if (KMAX > 0) {
#pragma unroll
            for (int k = 0; k < KR; ++k)
                if (k < g.K) visit(k, __fadd_rn(top[k], __fmul_rn(__fsub_rn(bot[k], top[k]), ty)));
        } else {
            for (int k = 0; k < g.K; ++k) {
                const int c = ct.idx[k];
                visit(k, bilerp(ptl[c], ptr[c], pbl[c], pbr[c], tx, ty));
            }
        }
        const float p = 1.f / ssum;                   // softmax of the largest logit: exp(zmax - zmax) / ssum
        if (conf_u8) conf_u8[pix] = p == p ? (uint8_t)rintf(p * 255.f) : (uint8_t)0;      // a NaN p is stored as 0 (no conversion of a NaN to an integer)
        if (conf_f32) conf_f32[pix] = p;
        if (!want_stats) continue;
        int bin = (int)(p * (float)kConfNB);
        bin = bin < kConfNB - 1 ? bin : kConfNB - 1;  // p == 1
        bin = bin > 0 ? bin : 0;                      // (a NaN logit: no index leaves the tables)
        // a NaN logit gives a NaN p: the pixel is counted in bin 0 and adds nothing to the confidence sums; a loss that is not finite adds
        // nothing to sel_sum either (no conversion of a non-finite value to an integer)
        const long long pf = p == p ? (long long)rint((double)p * 1048576.0) : 0;
        my_all += (double)pf;
        unsigned long long cnt = 1ull;
        if (target >= 0) {
            const bool hit = arg == target;
            cnt |= 1ull << kConfPackBits;
            if (hit) cnt |= 1ull << (2 * kConfPackBits);
            atomicAdd(&s_bin_sum[bin], (unsigned long long)pf);
            const float loss = (zmax + __logf(ssum)) - zt;
            const unsigned long long ce = loss - loss == 0.f ? (unsigned long long)(long long)rint((double)loss * 1048576.0) : 0ull;
            atomicAdd(&s_sel_cnt[target], 1);
            atomicAdd(&s_sel_sum[target], ce);
            if (!hit) {                               // a pixel with target == arg counts once
                atomicAdd(&s_sel_cnt[arg], 1);
                atomicAdd(&s_sel_sum[arg], ce);
            }
        }
        atomicAdd(&s_bins[bin], cnt);
    }
    if (!want_stats) return;
    my_all = wave_sum(my_all);
    if ((threadIdx.x & 63) == 0) s_all[threadIdx.x >> 6] = my_all;
    __syncthreads();
    unsigned long long* row = stats + (size_t)b * kConfStatsLen;
    constexpr unsigned long long field = (1ull << kConfPackBits) - 1;
    for (int e = threadIdx.x; e < kConfNB; e += blockDim.x) {
        const unsigned long long c = s_bins[e];
        if (c & field) atomicAdd(&row[e], c & field);
        if ((c >> kConfPackBits) & field) atomicAdd(&row[kConfNB + e], (c >> kConfPackBits) & field);
        if (c >> (2 * kConfPackBits)) atomicAdd(&row[2 * kConfNB + e], c >> (2 * kConfPackBits));
        if (s_bin_sum[e]) atomicAdd(&row[3 * kConfNB + e], s_bin_sum[e]);
    }
    for (int e = threadIdx.x; e < g.K; e += blockDim.x)
        if (s_sel_cnt[e]) {
            atomicAdd(&row[kConfOffSelCnt + e], (unsigned long long)s_sel_cnt[e]);
            atomicAdd(&row[kConfOffSelSum + e], s_sel_sum[e]);
        }
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        double all = 0.0;
        for (int i = 0; i < nw; ++i) all += s_all[i];
        if (all > 0.0) atomicAdd(&row[kConfOffSumAll], (unsigned long long)all);
    }
}

// Every output pointer may be null: nothing is written there.
int launch_upsample_confidence(const HeadCall& c, uint8_t* conf_u8, float* conf_f32, int64_t* stats, hipStream_t st) {
    ClassTable ct;
    HeadGeom g;
    if (int rc = head_call_check("confidence", c, &ct, &g)) return rc;
    const dim3 grid = head_band_grid(c.B, c.H, c.W);
    // a block's pixel counts per bin live in 21-bit fields
    AMS_REQUIRE((int64_t)cdiv(c.H, (int)grid.y) * 256 < (1 << kConfPackBits), "confidence: %d rows per band overflow a block's counters", cdiv(c.H, (int)grid.y));
    AMS_REQUIRE(c.logits, "confidence: null pointer");
    if (stats) AMS_CHECK_HIP(hipMemsetAsync(stats, 0, sizeof(int64_t) * kConfStatsLen * c.B, st));
    note_kernel("upsample_confidence_kernel");
    if (c.K <= 8)
        hipLaunchKernelGGL(upsample_confidence_kernel<8>, grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, conf_u8, conf_f32, (unsigned long long*)stats);
    else
        hipLaunchKernelGGL(upsample_confidence_kernel<0>, grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, conf_u8, conf_f32, (unsigned long long*)stats);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
