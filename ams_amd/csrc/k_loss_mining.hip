// Hard-pixel mining for the fine-tune loss (DeepLab's top_k_percent_pixels): the step keeps the fraction top_k of the valid pixels
// whose objective value is largest and takes the loss and gradient of the existing objective over those alone.  Nothing here touches the loss
// kernel: the kept set reaches ce_loss_grad_kernel as a label map in which every dropped pixel reads 255, which that kernel ignores in every form.
//
//   mining_key_kernel<KMAX, SOFT>  one walk over the B H W pixels, as upsample_confidence_kernel / upsample_soft_metric_kernel walk them (a thread owns
//                                  a pixel column and a band of rows, the K horizontally interpolated values of both source rows in registers): the
//                                  pixel's key = max(0, w_q pixel) in f32, -1 for a pixel that is not valid, and the number of valid pixels
//   mining_hist_kernel<P>          digit histogram (11 + 11 + 10 bits) of the keys >= 0 whose higher digits equal the prefix found so far: per block in
//                                  LDS (integer LDS atomics), flushed with integer global atomics, so the counts do not depend on any order
//   mining_scan_kernel             one block: pass 0 forms the rank k = max(1, floor(top_k n)) from the count the key pass left; every pass walks the
//                                  bins from the LARGEST digit down, fixes the digit that holds the rank and reduces the rank to one inside that bin
//   mining_relabel_kernel          labels' = key >= threshold ? label : 255, the number kept and the threshold into the result block; 16 pixels per
//                                  lane in 16-byte accesses where the pointers allow
//
// A key >= 0 orders like its bit pattern read as uint32, so the key of rank k from the top is found exactly; ties at the threshold are all kept.
// The key is this file's own evaluation of the objective (expf / logf, not the loss kernel's fast forms): it defines the kept set and nothing
// else, the kept pixels' loss comes from the loss kernel.
#include "head_common.hpp"
#include "block_scan.hpp"

namespace ams {

namespace {

constexpr int MIN_THREADS = BLOCK_SCAN_THREADS;
constexpr int MIN_BINS = 2048;
constexpr int MIN_PER_THREAD = MIN_BINS / MIN_THREADS;
constexpr int MIN_MAX_BLOCKS = 1024;
// state words (uint32) behind the three histograms
enum { MS_PREFIX = 0, MS_RANK = 1, MS_WORDS = 8 };
constexpr size_t MIN_HIST_WORDS = 3 * MIN_BINS + MS_WORDS;
// byte offsets inside a mining scratch block: the result, the histograms and the state, the key map; the mined labels follow the keys
constexpr size_t MIN_OFF_HIST = 64;
constexpr size_t MIN_OFF_KEYS = (MIN_OFF_HIST + MIN_HIST_WORDS * sizeof(uint32_t) + 255) / 256 * 256;
static_assert(MIN_OFF_KEYS == AMS_MINING_KEYS_OFFSET, "the scratch layout include/ams_hip.h documents");
constexpr float kMiningInvalid = -1.f;

__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int mining_grid(int64_t items) {
    const int64_t b = cdiv64(items, (int64_t)MIN_THREADS * 8);
    return (int)(b < 1 ? 1 : b > MIN_MAX_BLOCKS ? MIN_MAX_BLOCKS : b);
}

}  // namespace

// SOFT: the objective reads the teacher's distribution (alpha > 0 or gamma > 0); otherwise it is the hard loss under the class weights.
// lw.pk holds the class index and the quantised class weight of every label byte, all ones without class weights (fill_loss_weights).
template <int KMAX, bool SOFT>
__global__ __launch_bounds__(256) void mining_key_kernel(const float* __restrict__ logits, HeadGeom g, ClassTable ct, const uint8_t* __restrict__ teacher,
                                                         SoftTeacher sft, KdParams kd, LossWeights lw, float* __restrict__ keys,
                                                         unsigned long long* __restrict__ valid_cnt) {
    __shared__ uint32_t s_cnt[4];
    const int b = blockIdx.z;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t my_cnt = 0;
    int x0 = 0, x1 = 0; float tx = 0.f;
    int qx0 = 0, qx1 = 0; float qtx = 0.f;
    if (x < g.W) {
        src_tap(x, g.sx, g.w, x0, x1, tx);
        if constexpr (SOFT) src_tap(x, sft.sx, sft.tw, qx0, qx1, qtx);
    }
    const float* base = logits + (int64_t)b * g.h * g.w * g.ld;
    const int band = (g.H + (int)gridDim.y - 1) / (int)gridDim.y;
    const int ybeg = blockIdx.y * band, yend = ybeg + band < g.H ? ybeg + band : g.H;
    float top[KMAX], bot[KMAX];
    int cur_y0 = -1;
    for (int y = ybeg; y < yend; ++y) {
        if (x >= g.W) break;
        int y0, y1; float ty;
        src_tap(y, g.sy, g.h, y0, y1, ty);
        if (y0 != cur_y0) {                           // block-uniform (one output row per iteration)
            cur_y0 = y0;
            const float* ptl = base + ((int64_t)y0 * g.w + x0) * g.ld;
            const float* ptr = base + ((int64_t)y0 * g.w + x1) * g.ld;
            const float* pbl = base + ((int64_t)y1 * g.w + x0) * g.ld;
            const float* pbr = base + ((int64_t)y1 * g.w + x1) * g.ld;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int c = ct.idx[k < g.K ? k : 0];
                top[k] = __fadd_rn(ptl[c], __fmul_rn(__fsub_rn(ptr[c], ptl[c]), tx));
                bot[k] = __fadd_rn(pbl[c], __fmul_rn(__fsub_rn(pbr[c], pbl[c]), tx));
            }
        }
        const int64_t pix = ((int64_t)b * g.H + y) * g.W + x;
        const uint32_t pk = lw.pk[teacher[pix]];
        if (pk < 32u) { keys[pix] = kMiningInvalid; continue; }          // a label outside the subset, or a class of weight 0
        const int target = (int)(pk & 31u);
        float wq = (float)(pk >> 5) * (1.f / 1048576.f);                 // quantised on the host (fill_loss_weights): <= 2^24, exact
        // a class slot beyond K repeats class 0's logit: finite, <= the maximum, and left out of every sum by a select
        float z[KMAX];
        float zmax = -3.0e38f, zt = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            z[k] = __fadd_rn(top[k], __fmul_rn(__fsub_rn(bot[k], top[k]), ty));
            if (k < g.K) zmax = fmaxf(zmax, z[k]);
            if (k == target) zt = z[k];
        }
        float s1 = 0.f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) s1 += k < g.K ? expf(z[k] - zmax) : 0.f;
        const float hard = (zmax + logf(s1)) - zt;
        float v = hard;
        if constexpr (SOFT) {
            // the teacher's taps (ce_loss_grad_kernel<K, SOFT>'s: on a grid point, always at the label size, the logit itself)
            int qy0, qy1; float qty;
            src_tap(y, sft.sy, sft.th, qy0, qy1, qty);
            const float* qbase = sft.t + (int64_t)b * sft.th * sft.tw * sft.ld;
            const float* qtl = qbase + ((int64_t)qy0 * sft.tw + qx0) * sft.ld;
            const float* qtr = qbase + ((int64_t)qy0 * sft.tw + qx1) * sft.ld;
            const float* qbl = qbase + ((int64_t)qy1 * sft.tw + qx0) * sft.ld;
            const float* qbr = qbase + ((int64_t)qy1 * sft.tw + qx1) * sft.ld;
            const bool on_grid = qty == 0.f && qtx == 0.f;
            float pt[KMAX];
            float pmax = -3.0e38f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int c = sft.tidx[k < g.K ? k : 0];
                pt[k] = on_grid ? qtl[c] : bilerp(qtl[c], qtr[c], qbl[c], qbr[c], qtx, qty);
                if (k < g.K) pmax = fmaxf(pmax, pt[k]);
            }
            float psum = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                pt[k] = k < g.K ? expf((pt[k] - pmax) * kd.inv_t) : 0.f;
                psum += pt[k];
            }
            const float rp = 1.f / psum;
            // c = max_k p_k = 1 / psum (the largest entry is exp(0) = 1 before the scaling); c^gamma = exp(-gamma log psum), 1 at gamma = 0 exactly
            wq = rintf(wq * expf(-lw.gamma * logf(psum)) * 1048576.f) * (1.f / 1048576.f);
            // sum_k p_k (lse(zq) - zq_k), zq = (z - max) / T <= 0 <= lse: no cancellation
            float qsum = 0.f, pz = 0.f, p1 = 0.f;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const float zq = (z[k] - zmax) * kd.inv_t;
                const float p = pt[k] * rp;
                qsum += k < g.K ? expf(zq) : 0.f;
                pz += p * zq;
                p1 += p;
            }
            v = kd.at2 * (logf(qsum) * p1 - pz) + kd.om * hard;
        }
        if (!(wq > 0.f)) { keys[pix] = kMiningInvalid; continue; }       // the confidence weight rounded to 0: left out like a class of weight 0
        v *= wq;
        keys[pix] = v > 0.f ? v : 0.f;                                   // clamped at 0 from below; a NaN becomes 0
        my_cnt += 1;
    }
    my_cnt = wave_sum_u32(my_cnt);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = my_cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t cn = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        if (cn) atomicAdd(valid_cnt, (unsigned long long)cn);
    }
}

template <int PASS>
__global__ void __launch_bounds__(MIN_THREADS) mining_hist_kernel(const float* __restrict__ keys, int64_t n, uint32_t* hist, const uint32_t* state, int vec) {
    constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;         // the digit's lowest bit
    constexpr int ABOVE = PASS == 0 ? 31 : PASS == 1 ? 21 : 10;        // the bits from here up are the prefix (pass 0: none, bit 31 is 0)
    constexpr uint32_t DIGIT = PASS == 2 ? 0x3FFu : 0x7FFu;
    __shared__ uint32_t h[MIN_BINS];
    for (int b = threadIdx.x; b < MIN_BINS; b += MIN_THREADS) h[b] = 0;
    __syncthreads();
    const uint32_t prefix = PASS == 0 ? 0u : state[MS_PREFIX] >> ABOVE;
    auto one = [&](float key) {
        const uint32_t u = __float_as_uint(key);
        if (u < 0x80000000u && (u >> ABOVE) == prefix) atomicAdd(&h[(u >> SHIFT) & DIGIT], 1u);      // the sign bit: the sentinel of an invalid pixel
    };
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t; i < n4; i += step) {
            const float4 a = ld4(keys + 4 * i);
            one(a.x); one(a.y); one(a.z); one(a.w);
        }
        const int64_t i = 4 * n4 + t;
        if (i < n) one(keys[i]);
    } else {
        for (int64_t i = t; i < n; i += step) one(keys[i]);
    }
    __syncthreads();
    for (int b = threadIdx.x; b < MIN_BINS; b += MIN_THREADS)
        if (h[b]) atomicAdd(&hist[b], h[b]);
}

// The bins are walked from the top: thread t holds bins MIN_BINS - 1 - (t PER + j).  Without a valid pixel no bin holds the rank and the prefix
// stays 0: the threshold is 0 and no sentinel reaches it.
__global__ void __launch_bounds__(MIN_THREADS) mining_scan_kernel(const uint32_t* hist, uint32_t* state, int pass, int shift, float top_k,
                                                                  ams_mining_result* result) {
    __shared__ int64_t sh[MIN_THREADS];
    uint32_t rank;                                                      // 0-based from the largest key
    if (pass == 0) {
        const int64_t n = result->valid;
        int64_t k = (int64_t)floor((double)top_k * (double)n);
        if (k < 1) k = 1;
        rank = (uint32_t)(k - 1);
        if (threadIdx.x == 0) result->rank = k;
    } else {
        rank = state[MS_RANK];
    }
    // both are read before the scan's first barrier and written after its last one
    const uint32_t prefix = pass == 0 ? 0u : state[MS_PREFIX];
    uint32_t c[MIN_PER_THREAD], mine = 0;
#pragma unroll
    for (int j = 0; j < MIN_PER_THREAD; ++j) { c[j] = hist[MIN_BINS - 1 - ((int)threadIdx.x * MIN_PER_THREAD + j)]; mine += c[j]; }
    uint32_t run = (uint32_t)block_exclusive_scan((int64_t)mine, sh);
    if (rank < run || rank >= run + mine) return;                       // at most one thread's bins hold the rank
#pragma unroll
    for (int j = 0; j < MIN_PER_THREAD; ++j) {
        if (rank < run + c[j]) {
            state[MS_PREFIX] = prefix | ((uint32_t)(MIN_BINS - 1 - ((int)threadIdx.x * MIN_PER_THREAD + j)) << shift);
            state[MS_RANK] = rank - run;
            return;
        }
        run += c[j];
    }
}

__global__ void __launch_bounds__(MIN_THREADS) mining_relabel_kernel(const float* __restrict__ keys, const uint8_t* __restrict__ labels, int64_t n,
                                                                     const uint32_t* state, uint8_t* __restrict__ out, ams_mining_result* result,
                                                                     int vec) {
    const float cut = __uint_as_float(state[MS_PREFIX]);                // >= 0: a sentinel never reaches it
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    uint32_t kept = 0;
    auto one = [&](int64_t i) {
        const bool m = keys[i] >= cut;
        out[i] = m ? labels[i] : (uint8_t)255;
        kept += m ? 1u : 0u;
    };
    if (vec) {                                                          // all three pointers 16-byte aligned: 16 pixels per lane and step
        const int64_t n16 = n >> 4;
        for (int64_t i = t; i < n16; i += step) {
            const uint4 l = *reinterpret_cast<const uint4*>(labels + 16 * i);
            const uint32_t lv[4] = {l.x, l.y, l.z, l.w};
            uint32_t ov[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 a = ld4(keys + 16 * i + 4 * q);
                const bool m0 = a.x >= cut, m1 = a.y >= cut, m2 = a.z >= cut, m3 = a.w >= cut;
                const uint32_t keep = (m0 ? 0xFFu : 0u) | (m1 ? 0xFF00u : 0u) | (m2 ? 0xFF0000u : 0u) | (m3 ? 0xFF000000u : 0u);
                ov[q] = lv[q] | ~keep;                                  // a dropped pixel's byte becomes 255
                kept += (uint32_t)m0 + (uint32_t)m1 + (uint32_t)m2 + (uint32_t)m3;
            }
            *reinterpret_cast<uint4*>(out + 16 * i) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
        }
        const int64_t i = 16 * n16 + t;
        if (i < n) one(i);
    } else {
        for (int64_t i = t; i < n; i += step) one(i);
    }
    kept = wave_sum_u32(kept);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(reinterpret_cast<unsigned long long*>(&result->kept), (unsigned long long)kept);
    if (t == 0) result->threshold = cut;
}

// bytes of a mining scratch block for batches of up to B frames: the result, the histograms, the key map [B][H][W] f32, the mined labels [B][H][W]
size_t loss_mining_scratch(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    const size_t n = (size_t)B * H * W;
    return MIN_OFF_KEYS + (4 * n + 15) / 16 * 16 + (n + 15) / 16 * 16;
}

MiningBuffers loss_mining_buffers(void* scratch, int B, int H, int W) {
    char* p = static_cast<char*>(scratch);
    const size_t n = (size_t)B * H * W;
    MiningBuffers m;
    m.result = reinterpret_cast<ams_mining_result*>(p);
    m.hist = reinterpret_cast<uint32_t*>(p + MIN_OFF_HIST);
    m.keys = reinterpret_cast<float*>(p + MIN_OFF_KEYS);
    m.labels = reinterpret_cast<uint8_t*>(p + MIN_OFF_KEYS + (4 * n + 15) / 16 * 16);
    return m;
}

int mining_top_k_check(const char* who, float top_k) {
    AMS_REQUIRE(std::isfinite(top_k) && top_k > 0.f && top_k <= 1.f, "%s: top_k %g must lie in (0, 1]", who, (double)top_k);
    return AMS_OK;
}

// Everything a mined call is refused for, before its first memset: what launch_ce_loss_grad refuses of the same call, top_k, the geometry of the
// one-pass loss kernel (the mined map is for that kernel alone), 2^31 pixels and more (the counts are 32-bit), null pointers
int loss_mining_check(const HeadCall& c, const LossObjective& o, float top_k, const MiningBuffers& m, ClassTable* ct, HeadGeom* g) {
    if (int rc = kd_params_check("loss_mining", o.temperature, o.alpha)) return rc;
    if (int rc = loss_weights_check("loss_mining", o.class_weights, c.K, c.K, o.conf_gamma)) return rc;
    AMS_REQUIRE(o.conf_gamma == 0.f || o.teacher_logits, "loss_mining: conf_gamma %g weights by the teacher's confidence: it needs teacher logits", (double)o.conf_gamma);
    if (int rc = mining_top_k_check("loss_mining", top_k)) return rc;
    if (int rc = head_call_check("loss_mining", c, ct, g)) return rc;
    AMS_REQUIRE(ce_loss_grad_supported(c.w, c.W), "loss_mining: %d output columns on %d source columns is outside the one-pass loss kernel", c.W, c.w);
    AMS_REQUIRE((int64_t)c.B * c.H * c.W < ((int64_t)1 << 31), "loss_mining: %lld pixels overflow the 32-bit counts", (long long)((int64_t)c.B * c.H * c.W));
    if (o.teacher_logits) {
        AMS_REQUIRE(o.th >= 1 && o.tw >= 1 && o.th <= c.H && o.tw <= c.W, "loss_mining: teacher logits of %d x %d for labels of %d x %d", o.th, o.tw, c.H, c.W);
        AMS_REQUIRE(tlogits_layout_ok(o.layout), "loss_mining: unknown teacher-logit layout %d", o.layout);
    }
    AMS_REQUIRE(c.logits && c.teacher && m.keys && m.labels && m.hist && m.result, "loss_mining: null pointer");
    AMS_REQUIRE(((uintptr_t)m.result & 7) == 0 && ((uintptr_t)m.hist & 3) == 0 && ((uintptr_t)m.keys & 3) == 0, "loss_mining: misaligned buffer");
    return AMS_OK;
}

// step 1: the key map and the valid count (the result block and the histograms zeroed here)
int launch_mining_keys(const HeadCall& c, const LossObjective& o, float top_k, const MiningBuffers& m, hipStream_t st) {
    ClassTable ct;
    HeadGeom g;
    if (int rc = loss_mining_check(c, o, top_k, m, &ct, &g)) return rc;
    const LossForm f = loss_form(o, c.K);
    SoftTeacher sft;
    memset(&sft, 0, sizeof(sft));
    if (f.soft) sft = soft_teacher_geom(o.teacher_logits, o.th, o.tw, o.layout, ct, c.K, c.NC, c.H, c.W);
    KdParams kd;
    kd.inv_t = 1.f / o.temperature;
    kd.at2 = o.alpha * (o.temperature * o.temperature);
    kd.at = o.alpha * o.temperature;
    kd.om = 1.f - o.alpha;
    LossWeights lw;
    fill_loss_weights(ct, o.class_weights, c.K, o.conf_gamma, &lw);
    AMS_CHECK_HIP(hipMemsetAsync(m.result, 0, sizeof(ams_mining_result), st));
    AMS_CHECK_HIP(hipMemsetAsync(m.hist, 0, MIN_HIST_WORDS * sizeof(uint32_t), st));
    const dim3 grid = head_band_grid(c.B, c.H, c.W);
    unsigned long long* cnt = reinterpret_cast<unsigned long long*>(&m.result->valid);
    note_kernel("mining_key_kernel");
    auto launch = [&](auto soft_c) {
        constexpr bool S = decltype(soft_c)::value;
        const int KM = ce_kmax(c.K);
        if (KM == 8) hipLaunchKernelGGL((mining_key_kernel<8, S>), grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, sft, kd, lw, m.keys, cnt);
        else if (KM == 20) hipLaunchKernelGGL((mining_key_kernel<20, S>), grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, sft, kd, lw, m.keys, cnt);
        else hipLaunchKernelGGL((mining_key_kernel<32, S>), grid, dim3(256), 0, st, c.logits, g, ct, c.teacher, sft, kd, lw, m.keys, cnt);
    };
    if (f.soft) launch(std::true_type{}); else launch(std::false_type{});
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// step 2: the key of rank k from the top into the state words, k into the result block; n and k are read on the device
int launch_mining_select(int64_t n, float top_k, const MiningBuffers& m, hipStream_t st) {
    uint32_t* state = m.hist + 3 * MIN_BINS;
    const int vec = aligned16(m.keys) ? 1 : 0;
    const int grid = mining_grid(n);
    note_kernel("mining_hist_kernel");
    hipLaunchKernelGGL(mining_hist_kernel<0>, dim3(grid), dim3(MIN_THREADS), 0, st, m.keys, n, m.hist, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mining_scan_kernel, dim3(1), dim3(MIN_THREADS), 0, st, m.hist, state, 0, 21, top_k, m.result);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mining_hist_kernel<1>, dim3(grid), dim3(MIN_THREADS), 0, st, m.keys, n, m.hist + MIN_BINS, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mining_scan_kernel, dim3(1), dim3(MIN_THREADS), 0, st, m.hist + MIN_BINS, state, 1, 10, top_k, m.result);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mining_hist_kernel<2>, dim3(grid), dim3(MIN_THREADS), 0, st, m.keys, n, m.hist + 2 * MIN_BINS, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(mining_scan_kernel, dim3(1), dim3(MIN_THREADS), 0, st, m.hist + 2 * MIN_BINS, state, 2, 0, top_k, m.result);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// step 3: the mined label map, the kept count and the threshold
int launch_mining_relabel(const uint8_t* labels, int64_t n, const MiningBuffers& m, hipStream_t st) {
    const int vec = aligned16(m.keys) && aligned16(labels) && aligned16(m.labels) ? 1 : 0;
    note_kernel("mining_relabel_kernel");
    hipLaunchKernelGGL(mining_relabel_kernel, dim3(mining_grid(cdiv64(n, 16))), dim3(MIN_THREADS), 0, st, m.keys, labels, n, m.hist + 3 * MIN_BINS,
                       m.labels, m.result, vec);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// steps 1 - 3 of a mined step; a refused call launches and writes nothing
int launch_loss_mining(const HeadCall& c, const LossObjective& o, float top_k, const MiningBuffers& m, hipStream_t st) {
    if (int rc = launch_mining_keys(c, o, top_k, m, st)) return rc;
    const int64_t n = (int64_t)c.B * c.H * c.W;
    if (int rc = launch_mining_select(n, top_k, m, st)) return rc;
    return launch_mining_relabel(c.teacher, n, m, st);
}

}  // namespace ams
