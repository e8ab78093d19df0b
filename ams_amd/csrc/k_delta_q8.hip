// The downlink delta in 8 bits, encoded (server) and decoded (edge) on the device.  Both ends hold the model the update starts from, so
// the change travels and not the value: one int8 code per masked element, one f32 scale per variable.
//
// Payload, over the descriptor table of k_delta.hip, no header, no padding:
//   [mask section: per variable np.packbits(mask)] [n_vars little-endian f32 scales] [one int8 per set mask bit, in mask order]
// The mask section has an odd length in both layouts of the 19-class model, so the scales are read and written as bytes.
//
// Arithmetic, f32 with one rounding per operation (the products and sums go through __fmul_rn / __fadd_rn so that no fma can form):
//   d = cur - base;  amax_v = max |d| over the masked elements of v;  scale_v = amax_v / 127, 0 if below 2^-126 (the same bits whether
//   or not denormals are flushed);  q = scale_v == 0 ? 0 : clamp(rintf(d / scale_v), -127, 127);  decoded = base + scale_v * q.
//
// Both sides walk the mask section as k_delta.hip does (delta_walk.hpp): one block per 2048-byte segment, 64 mask bits per thread.
//
//   q8_amax_kernel          per segment: its set bits, and per variable the largest |d| of its masked elements compared as the uint32
//                           bits of the non-negative float (NaN above inf): per thread over each run of one variable, LDS atomicMax per
//                           run, then one global atomicMax per (block, variable) — integer maxima, so the arrival order does not matter
//   q8_encode_scan_kernel   one block: exclusive scan of the counts; maxima -> scales in place; a maximum of inf or NaN sets the status
//                           AMS_DELTA_Q8_NONFINITE and the size 0; else the size = mask bytes + 4 n_vars + set bits
//   q8_encode_write_kernel  nothing unless the status is OK and the size fits: mask bytes, the scales (block 0), one code per set bit and,
//                           with advance_base, the decoder's value of the element into the base
//   delta_count_kernel      (k_delta.hip) the decoder's first pass, as it is
//   q8_delta_scan_kernel    one block: exclusive scan, then the validation: size, padding bits, scales
//   q8_delta_apply_kernel   nothing unless the status is OK: element += scale of its variable x the code at its scanned position
#include "common.hpp"
#include "kernels.hpp"
#include "block_scan.hpp"
#include "delta_walk.hpp"

namespace ams {

namespace {

__device__ inline float q8_scale(uint32_t amax_bits) {
    const float s = __fdiv_rn(__uint_as_float(amax_bits), 127.f);
    return s < 0x1p-126f ? 0.f : s;
}
__device__ inline int q8_code(float d, float scale) {
    if (scale == 0.f) return 0;
    const float q = rintf(__fdiv_rn(d, scale));              // ties to even
    return (int)fminf(fmaxf(q, -127.f), 127.f);
}
__device__ inline float q8_decode(float base, float scale, int q) { return __fadd_rn(base, __fmul_rn(scale, (float)q)); }

// 8 mask entries (0 / non-0, one byte each, the first at the lowest address) -> 8 bits, the first entry in bit 7
__device__ inline uint32_t pack8(uint64_t x) {
    const uint64_t nz = ((((x & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | x) & 0x8080808080808080ull) >> 7;
    return (uint32_t)((nz * 0x8040201008040201ull) >> 56);   // bit 8 i -> bit 63 - i: the shifted copies meet in no bit
}

// The 64 mask bits of payload bytes [b, b + 8) made from the element mask (uint8 per element in layout order, est[v] = the first element
// of variable v; nullptr = every element): bit 63 = the first element of byte b; padding bits and bytes beyond the section are 0.
__device__ inline uint64_t q8_mask_word(const uint8_t* mask, const int64_t* moff, const int64_t* est, int n_vars, int64_t b,
                                        int64_t mask_bytes) {
    uint64_t w = 0;
    int v = -1;
    for (int j = 0; j < 8; ++j) {
        const int64_t byte = b + j;
        uint32_t bits = 0;
        if (byte < mask_bytes) {
            v = delta_var_of_byte(moff, n_vars, byte, v);
            const int64_t e0 = (byte - moff[v]) * 8, left = est[v + 1] - est[v] - e0;
            const int n = left >= 8 ? 8 : left > 0 ? (int)left : 0;
            if (!mask) {
                bits = (0xFFu << (8 - n)) & 0xFFu;
            } else {
                const uint8_t* m = mask + est[v] + e0;
                if (n == 8 && ((uintptr_t)m & 7) == 0) bits = pack8(*reinterpret_cast<const uint64_t*>(m));
                else for (int i = 0; i < n; ++i) bits |= m[i] ? 0x80u >> i : 0u;
            }
        }
        w = (w << 8) | bits;
    }
    return w;
}

__device__ inline uint32_t load_u32_bytes(const uint8_t* p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

}  // namespace

__global__ void __launch_bounds__(DELTA_THREADS) q8_amax_kernel(const uint8_t* mask, const ams_delta_var* vars, const int64_t* estart, int n_vars,
                                                                int64_t mask_bytes, const float* params, const float* stats,
                                                                const float* base_params, const float* base_stats, int64_t* counts,
                                                                uint32_t* amax) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int64_t moff[AMS_DELTA_MAX_VARS], est[AMS_DELTA_MAX_VARS + 1];
    __shared__ uint32_t bmax[AMS_DELTA_MAX_VARS];
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) { moff[v] = vars[v].mask_offset; bmax[v] = 0; }
    for (int v = threadIdx.x; v <= n_vars; v += DELTA_THREADS) est[v] = estart[v];
    __syncthreads();
    const int64_t b = blockIdx.x * DELTA_SEG + 8 * (int64_t)threadIdx.x;
    uint64_t w = b < mask_bytes ? q8_mask_word(mask, moff, est, n_vars, b, mask_bytes) : 0;
    const int64_t total = block_sum(__popcll(w), sh);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
    int v = -1, run = -1;
    uint32_t m = 0;
    const float *cur = nullptr, *base = nullptr;
    while (w) {
        const int lz = __clzll(w);
        w &= ~(1ull << (63 - lz));
        const int64_t byte = b + (lz >> 3);
        v = delta_var_of_byte(moff, n_vars, byte, v);
        if (v != run) {                                     // a new variable: hand the finished run to the block
            if (m) atomicMax(&bmax[run], m);
            m = 0;
            run = v;
            const ams_delta_var d = vars[v];
            cur = (d.region == AMS_REGION_PARAMS ? params : stats) + d.offset;
            base = (d.region == AMS_REGION_PARAMS ? base_params : base_stats) + d.offset;
        }
        const int64_t e = (byte - moff[v]) * 8 + (lz & 7);
        const uint32_t u = __float_as_uint(fabsf(cur[e] - base[e]));
        m = u > m ? u : m;
    }
    if (m) atomicMax(&bmax[run], m);
    __syncthreads();
    for (int i = threadIdx.x; i < n_vars; i += DELTA_THREADS)
        if (bmax[i]) atomicMax(&amax[i], bmax[i]);          // at most one per (block, variable)
}

__global__ void __launch_bounds__(DELTA_THREADS) q8_encode_scan_kernel(int64_t* counts, int nseg, int n_vars, int64_t mask_bytes, uint32_t* amax,
                                                                       int64_t* need, int64_t* payload_bytes, int32_t* status) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int nonfinite;
    if (threadIdx.x == 0) nonfinite = 0;
    const int chunk = (nseg + DELTA_THREADS - 1) / DELTA_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < nseg ? s0 + chunk : nseg;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += counts[s];
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh);
    for (int s = s0; s < s1; ++s) { const int64_t c = counts[s]; counts[s] = run; run += c; }
    // the maxima become the scales, in place; the bits of inf and of every NaN lie at or above inf's
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) {
        const uint32_t u = amax[v];
        if (u >= 0x7F800000u) atomicOr(&nonfinite, 1);
        amax[v] = __float_as_uint(q8_scale(u));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int64_t size = mask_bytes + 4 * (int64_t)n_vars + total;
        *status = nonfinite ? AMS_DELTA_Q8_NONFINITE : AMS_DELTA_OK;
        *need = size;
        *payload_bytes = nonfinite ? 0 : size;
    }
}

__global__ void __launch_bounds__(DELTA_THREADS) q8_encode_write_kernel(const uint8_t* mask, const ams_delta_var* vars, const int64_t* estart,
                                                                        int n_vars, int64_t mask_bytes, const float* params, const float* stats,
                                                                        float* base_params, float* base_stats, int advance_base,
                                                                        const int64_t* offs, const float* scales, const int64_t* need,
                                                                        const int32_t* status, uint8_t* payload, int64_t cap) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int64_t moff[AMS_DELTA_MAX_VARS], est[AMS_DELTA_MAX_VARS + 1];
    __shared__ float scl[AMS_DELTA_MAX_VARS];
    if (*status != AMS_DELTA_OK || *need > cap) return;     // all or nothing (the same words for every thread)
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) { moff[v] = vars[v].mask_offset; scl[v] = scales[v]; }
    for (int v = threadIdx.x; v <= n_vars; v += DELTA_THREADS) est[v] = estart[v];
    __syncthreads();
    const int64_t b = blockIdx.x * DELTA_SEG + 8 * (int64_t)threadIdx.x;
    uint64_t w = b < mask_bytes ? q8_mask_word(mask, moff, est, n_vars, b, mask_bytes) : 0;
    int64_t k = offs[blockIdx.x] + block_exclusive_scan(__popcll(w), sh);
    for (int j = 0; j < 8; ++j)
        if (b + j < mask_bytes) payload[b + j] = (uint8_t)(w >> (56 - 8 * j));
    if (blockIdx.x == 0) {
        for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) {
            const uint32_t u = __float_as_uint(scl[v]);
            uint8_t* p = payload + mask_bytes + 4 * (int64_t)v;
            p[0] = (uint8_t)u; p[1] = (uint8_t)(u >> 8); p[2] = (uint8_t)(u >> 16); p[3] = (uint8_t)(u >> 24);
        }
    }
    const int64_t codes = mask_bytes + 4 * (int64_t)n_vars;  // the code section's first byte
    int v = -1, run = -1;
    float scale = 0.f;
    const float* cur = nullptr;
    float* base = nullptr;
    while (w) {
        const int lz = __clzll(w);
        w &= ~(1ull << (63 - lz));
        const int64_t byte = b + (lz >> 3);
        v = delta_var_of_byte(moff, n_vars, byte, v);
        if (v != run) {
            run = v;
            scale = scl[v];
            const ams_delta_var d = vars[v];
            cur = (d.region == AMS_REGION_PARAMS ? params : stats) + d.offset;
            base = (d.region == AMS_REGION_PARAMS ? base_params : base_stats) + d.offset;
        }
        const int64_t e = (byte - moff[v]) * 8 + (lz & 7);
        const float bv = base[e];
        const int q = q8_code(cur[e] - bv, scale);
        const int64_t pos = codes + k++;
        if (pos < cap) payload[pos] = (uint8_t)(int8_t)q;    // (implied by *need <= cap)
        if (advance_base) base[e] = q8_decode(bv, scale, q);
    }
}

__global__ void __launch_bounds__(DELTA_THREADS) q8_delta_scan_kernel(int64_t* counts, int nseg, const ams_delta_var* vars, int n_vars,
                                                                      const uint8_t* payload, int64_t payload_bytes, int64_t mask_bytes,
                                                                      int64_t* n_applied, int32_t* status) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int bad_pad, bad_scale;
    if (threadIdx.x == 0) bad_pad = bad_scale = 0;
    const int chunk = (nseg + DELTA_THREADS - 1) / DELTA_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < nseg ? s0 + chunk : nseg;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += counts[s];
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh);
    for (int s = s0; s < s1; ++s) { const int64_t c = counts[s]; counts[s] = run; run += c; }
    const int64_t readable = payload_bytes < mask_bytes ? payload_bytes : mask_bytes;
    const bool has_scales = payload_bytes >= mask_bytes + 4 * (int64_t)n_vars;
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) {
        const int64_t n = vars[v].count;
        const int r = (int)(n & 7);
        const int64_t byte = vars[v].mask_offset + (n >> 3);
        if (r && byte < readable && (payload[byte] & (0xFFu >> r))) atomicOr(&bad_pad, 1);
        if (has_scales) {                                   // NaN or inf; nonzero below 2^-126; negative
            const uint32_t u = load_u32_bytes(payload + mask_bytes + 4 * (int64_t)v), a = u & 0x7FFFFFFFu;
            if (a >= 0x7F800000u || (a != 0 && a < 0x00800000u) || ((u >> 31) && a != 0)) atomicOr(&bad_scale, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t st = mask_bytes + 4 * (int64_t)n_vars + total != payload_bytes ? AMS_DELTA_BAD_SIZE
                           : bad_pad ? AMS_DELTA_BAD_PADDING : bad_scale ? AMS_DELTA_BAD_SCALE : AMS_DELTA_OK;
        *status = st;
        *n_applied = st == AMS_DELTA_OK ? total : 0;
    }
}

__global__ void __launch_bounds__(DELTA_THREADS) q8_delta_apply_kernel(const uint8_t* payload, int64_t mask_bytes, const int64_t* offs,
                                                                       const ams_delta_var* vars, int n_vars, float* params, int64_t n_params,
                                                                       float* stats, int64_t n_stats, const int32_t* status) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int64_t moff[AMS_DELTA_MAX_VARS];
    __shared__ float scl[AMS_DELTA_MAX_VARS];
    if (*status != AMS_DELTA_OK) return;                    // all or nothing: a payload that failed validation writes no element
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) {
        moff[v] = vars[v].mask_offset;
        scl[v] = __uint_as_float(load_u32_bytes(payload + mask_bytes + 4 * (int64_t)v));
    }
    const int64_t b = blockIdx.x * DELTA_SEG + 8 * (int64_t)threadIdx.x;
    uint64_t w = b < mask_bytes ? mask_word(payload, b, mask_bytes) : 0;
    int64_t k = offs[blockIdx.x] + block_exclusive_scan(__popcll(w), sh);       // (the scan's barriers also publish moff and scl)
    const uint8_t* codes = payload + mask_bytes + 4 * (int64_t)n_vars;
    int v = -1;
    while (w) {
        const int lz = __clzll(w);
        w &= ~(1ull << (63 - lz));
        const int64_t byte = b + (lz >> 3);
        v = delta_var_of_byte(moff, n_vars, byte, v);
        const int64_t e = (byte - moff[v]) * 8 + (lz & 7);
        const int q = (int8_t)codes[k++];
        const ams_delta_var d = vars[v];
        if (e < 0 || e >= d.count) continue;                 // a padding bit (validation rejects those) or a malformed table
        float* dst = d.region == AMS_REGION_PARAMS ? params : d.region == AMS_REGION_STATS ? stats : nullptr;
        const int64_t n_region = d.region == AMS_REGION_PARAMS ? n_params : n_stats;
        if (dst && d.offset + e < n_region) dst[d.offset + e] = q8_decode(dst[d.offset + e], scl[v], q);
    }
}

size_t q8_encode_table_words(int n_vars) { return 5 * (size_t)n_vars + 1 + ((size_t)n_vars + 1) / 2; }

int launch_encode_delta_q8(const uint8_t* mask, int64_t* table_dev, int n_vars, int64_t mask_bytes, const float* params, const float* stats,
                           float* base_params, float* base_stats, int advance_base, int64_t* work, uint8_t* payload, int64_t cap,
                           int64_t* payload_bytes, int32_t* status, hipStream_t st) {
    const ams_delta_var* vars = reinterpret_cast<const ams_delta_var*>(table_dev);
    const int64_t* estart = table_dev + 4 * (int64_t)n_vars;
    uint32_t* amax = reinterpret_cast<uint32_t*>(table_dev + 5 * (int64_t)n_vars + 1);
    int64_t* need = work;
    int64_t* counts = work + 1;
    const int nseg = (int)delta_segments(mask_bytes);
    hipLaunchKernelGGL(q8_amax_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, mask, vars, estart, n_vars, mask_bytes, params, stats,
                       (const float*)base_params, (const float*)base_stats, counts, amax);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(q8_encode_scan_kernel, dim3(1), dim3(DELTA_THREADS), 0, st, counts, nseg, n_vars, mask_bytes, amax, need, payload_bytes,
                       status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(q8_encode_write_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, mask, vars, estart, n_vars, mask_bytes, params, stats,
                       base_params, base_stats, advance_base, (const int64_t*)counts, reinterpret_cast<const float*>(amax),
                       (const int64_t*)need, (const int32_t*)status, payload, cap);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// scratch (int64): [descriptor table: 4 per variable][segment counts -> offsets], as launch_apply_delta
int launch_apply_delta_q8(const uint8_t* payload, int64_t payload_bytes, const ams_delta_var* vars_dev, int n_vars, int64_t mask_bytes,
                          float* params, int64_t n_params, float* stats, int64_t n_stats, int64_t* counts, int64_t* n_applied, int32_t* status,
                          hipStream_t st) {
    const int nseg = (int)delta_segments(mask_bytes);
    const int64_t readable = payload_bytes < mask_bytes ? payload_bytes : mask_bytes;
    RUN_RC(launch_delta_count(payload, readable, nseg, counts, st));
    hipLaunchKernelGGL(q8_delta_scan_kernel, dim3(1), dim3(DELTA_THREADS), 0, st, counts, nseg, vars_dev, n_vars, payload, payload_bytes,
                       mask_bytes, n_applied, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(q8_delta_apply_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, payload, mask_bytes, counts, vars_dev, n_vars, params,
                       n_params, stats, n_stats, status);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
