// Server-side model update: the coordinates of coord_desc_auto chosen on the device (SemanticNetwork.py:263-288) and the downlink delta
// encoded there (run.py:316-336).  The mirror image of k_delta.hip.
//
// Selection.  change[i] = |after[i] - before[i]| is one IEEE subtraction; a non-negative float orders like its bit pattern read as uint32
// (NaNs above +inf), so the change of rank k is found exactly by a radix select over the bits, 11 + 11 + 10 of them per pass.  The change
// is recomputed in every pass: the two arenas (17 MB) stay in the caches, and the chain is latency, not bandwidth.
//
//   select_hist_kernel<P>  digit histogram of the elements whose higher digits equal the prefix found so far: per block in LDS (integer LDS
//                          atomics), flushed with integer global atomics; integer counts do not depend on the arrival order
//   select_scan_kernel     one block: scans the bins, fixes the digit that holds the rank, reduces the rank to a rank inside that bin
//   select_tail_kernel     with a = the change of rank k known: the number of changes <= a and the smallest change > a
//   select_finish_kernel   the result block: a, b = the change of rank k + 1 (a again when it ties or k + 1 == n), the number of NaN changes
//   select_apply_kernel    mask = change > cut, params = mask ? after : before, the number kept; 16 bytes per lane where the pointers allow
//
// Encode.  Over the ams_delta_var table of the decoder: a wave owns a 512-byte segment of the mask section and takes 64 mask bits (8 payload
// bytes) per step: lane l holds bit l & 7 of byte l >> 3, the wave's ballot is the 8 bytes with each byte's bits in reverse order.
//
//   encode_kernel<false>   set bits per segment
//   encode_scan_kernel     one block: exclusive scan of the segment counts; the payload size = mask bytes + 2 x set bits
//   encode_kernel<true>    nothing unless the size fits the buffer; mask bytes, and each set bit's value as the two bytes of its fp16
#include "common.hpp"
#include "kernels.hpp"
#include "block_scan.hpp"

#include <hip/hip_fp16.h>

namespace ams {

namespace {

constexpr int SEL_THREADS = BLOCK_SCAN_THREADS;
constexpr int SEL_BINS = 2048;
constexpr int SEL_PER_THREAD = SEL_BINS / SEL_THREADS;
constexpr int SEL_MAX_BLOCKS = 1024;
// state words (uint32) behind the three histograms
enum { ST_PREFIX = 0, ST_RANK = 1, ST_LE = 2, ST_GT_INV = 3, ST_NAN = 4, ST_WORDS = 8 };
constexpr size_t SEL_SCRATCH_WORDS = 3 * SEL_BINS + ST_WORDS;

constexpr int ENC_THREADS = 256;
constexpr int ENC_WAVES = ENC_THREADS / 64;
constexpr int64_t ENC_SEG = 512;                           // mask bytes per wave: 64 steps of 8

__device__ inline uint32_t change_bits(float a, float b) { return __float_as_uint(fabsf(a - b)); }

__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}

// f(after[i], before[i]) for every i < n, a grid-stride loop; vec: both pointers are 16-byte aligned
template <class F>
__device__ inline void for_each_pair(const float* after, const float* before, int64_t n, bool vec, F f) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        const int64_t n4 = n >> 2;
        for (int64_t i = t; i < n4; i += step) {
            const float4 a = ld4(after + 4 * i), b = ld4(before + 4 * i);
            f(a.x, b.x); f(a.y, b.y); f(a.z, b.z); f(a.w, b.w);
        }
        const int64_t i = 4 * n4 + t;
        if (i < n) f(after[i], before[i]);
    } else {
        for (int64_t i = t; i < n; i += step) f(after[i], before[i]);
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int select_grid(int64_t n) {
    const int64_t b = cdiv64(n, (int64_t)SEL_THREADS * 8);
    return (int)(b < 1 ? 1 : b > SEL_MAX_BLOCKS ? SEL_MAX_BLOCKS : b);
}

}  // namespace

template <int PASS>
__global__ void __launch_bounds__(SEL_THREADS) select_hist_kernel(const float* after, const float* before, int64_t n, uint32_t* hist,
                                                                  uint32_t* state, int vec) {
    constexpr int SHIFT = PASS == 0 ? 21 : PASS == 1 ? 10 : 0;         // the digit's lowest bit
    constexpr int ABOVE = PASS == 0 ? 31 : PASS == 1 ? 21 : 10;        // the bits from here up are the prefix (pass 0: none, bit 31 is 0)
    constexpr uint32_t DIGIT = PASS == 2 ? 0x3FFu : 0x7FFu;
    __shared__ uint32_t h[SEL_BINS];
    for (int b = threadIdx.x; b < SEL_BINS; b += SEL_THREADS) h[b] = 0;
    __syncthreads();
    const uint32_t prefix = PASS == 0 ? 0u : state[ST_PREFIX] >> ABOVE;
    uint32_t nan = 0;
    for_each_pair(after, before, n, vec != 0, [&](float a, float b) {
        const uint32_t u = change_bits(a, b);
        if (PASS == 0) nan += u > 0x7F800000u ? 1u : 0u;
        if ((u >> ABOVE) == prefix) atomicAdd(&h[(u >> SHIFT) & DIGIT], 1u);
    });
    __syncthreads();
    for (int b = threadIdx.x; b < SEL_BINS; b += SEL_THREADS)
        if (h[b]) atomicAdd(&hist[b], h[b]);
    if (PASS == 0) {
        nan = wave_sum_u32(nan);
        if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&state[ST_NAN], nan);
    }
}

__global__ void __launch_bounds__(SEL_THREADS) select_scan_kernel(const uint32_t* hist, uint32_t* state, int pass, int shift, uint32_t k) {
    __shared__ int64_t sh[SEL_THREADS];
    // both are read before the scan's first barrier and written after its last one
    const uint32_t rank = pass == 0 ? k : state[ST_RANK];
    const uint32_t prefix = pass == 0 ? 0u : state[ST_PREFIX];
    uint32_t c[SEL_PER_THREAD], mine = 0;
#pragma unroll
    for (int j = 0; j < SEL_PER_THREAD; ++j) { c[j] = hist[threadIdx.x * SEL_PER_THREAD + j]; mine += c[j]; }
    uint32_t run = (uint32_t)block_exclusive_scan((int64_t)mine, sh);
    if (rank < run || rank >= run + mine) return;                       // exactly one thread's bins hold the rank
#pragma unroll
    for (int j = 0; j < SEL_PER_THREAD; ++j) {
        if (rank < run + c[j]) {
            state[ST_PREFIX] = prefix | ((uint32_t)(threadIdx.x * SEL_PER_THREAD + j) << shift);
            state[ST_RANK] = rank - run;
            return;
        }
        run += c[j];
    }
}

__global__ void __launch_bounds__(SEL_THREADS) select_tail_kernel(const float* after, const float* before, int64_t n, uint32_t* state, int vec) {
    const uint32_t a = state[ST_PREFIX];
    uint32_t le = 0, gt_inv = 0;                                        // ~(the smallest change > a), so that zeroed scratch means "none"
    for_each_pair(after, before, n, vec != 0, [&](float x, float y) {
        const uint32_t u = change_bits(x, y);
        le += u <= a ? 1u : 0u;
        if (u > a && ~u > gt_inv) gt_inv = ~u;
    });
    le = wave_sum_u32(le);
    gt_inv = wave_max_u32(gt_inv);
    if ((threadIdx.x & 63) == 0) {
        if (le) atomicAdd(&state[ST_LE], le);
        if (gt_inv) atomicMax(&state[ST_GT_INV], gt_inv);
    }
}

__global__ void select_finish_kernel(const uint32_t* state, int64_t n, int64_t k, ams_select_result* result) {
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t a = state[ST_PREFIX];
    // rank k + 1 is a again when more than k + 1 changes are <= a, or when there is no such rank
    const bool again = (int64_t)state[ST_LE] > k + 1 || k + 1 >= n || state[ST_GT_INV] == 0;
    result->a = __uint_as_float(a);
    result->b = __uint_as_float(again ? a : ~state[ST_GT_INV]);
    result->nan_count = (int64_t)state[ST_NAN];
}

__global__ void __launch_bounds__(SEL_THREADS) select_apply_kernel(float* params, const float* before, int64_t n, float cut, uint8_t* mask,
                                                                   unsigned long long* n_kept, int vec) {
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    uint32_t kept = 0;
    auto one = [&](int64_t i) {
        const float p = params[i], b = before[i];
        const bool m = fabsf(p - b) > cut;                              // false for a NaN change and for cut = NaN
        mask[i] = m ? 1 : 0;
        params[i] = m ? p : b;
        kept += m ? 1u : 0u;
    };
    if (vec) {                                                          // floats 16-byte aligned, mask 4-byte aligned
        const int64_t n4 = n >> 2;
        for (int64_t i = t; i < n4; i += step) {
            const float4 p = ld4(params + 4 * i), b = ld4(before + 4 * i);
            const bool m0 = fabsf(p.x - b.x) > cut, m1 = fabsf(p.y - b.y) > cut, m2 = fabsf(p.z - b.z) > cut, m3 = fabsf(p.w - b.w) > cut;
            st4(params + 4 * i, make_float4(m0 ? p.x : b.x, m1 ? p.y : b.y, m2 ? p.z : b.z, m3 ? p.w : b.w));
            *reinterpret_cast<uint32_t*>(mask + 4 * i) = (uint32_t)m0 | ((uint32_t)m1 << 8) | ((uint32_t)m2 << 16) | ((uint32_t)m3 << 24);
            kept += (uint32_t)m0 + (uint32_t)m1 + (uint32_t)m2 + (uint32_t)m3;
        }
        const int64_t i = 4 * n4 + t;
        if (i < n) one(i);
    } else {
        for (int64_t i = t; i < n; i += step) one(i);
    }
    kept = wave_sum_u32(kept);
    if ((threadIdx.x & 63) == 0 && kept) atomicAdd(n_kept, (unsigned long long)kept);
}

size_t select_scratch() { return (SEL_SCRATCH_WORDS * sizeof(uint32_t) + sizeof(int64_t) - 1) / sizeof(int64_t); }

// scratch: select_scratch() int64 = three histograms of SEL_BINS uint32 + the state words
int launch_select_changed(const float* after, const float* before, int64_t n, int64_t k, ams_select_result* result, int64_t* scratch,
                          hipStream_t st) {
    uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
    uint32_t* state = hist + 3 * SEL_BINS;
    const int vec = aligned16(after) && aligned16(before) ? 1 : 0;
    const int grid = select_grid(n);
    AMS_CHECK_HIP(hipMemsetAsync(scratch, 0, SEL_SCRATCH_WORDS * sizeof(uint32_t), st));
    hipLaunchKernelGGL(select_hist_kernel<0>, dim3(grid), dim3(SEL_THREADS), 0, st, after, before, n, hist, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, st, hist, state, 0, 21, (uint32_t)k);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_hist_kernel<1>, dim3(grid), dim3(SEL_THREADS), 0, st, after, before, n, hist + SEL_BINS, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, st, hist + SEL_BINS, state, 1, 10, 0u);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_hist_kernel<2>, dim3(grid), dim3(SEL_THREADS), 0, st, after, before, n, hist + 2 * SEL_BINS, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(SEL_THREADS), 0, st, hist + 2 * SEL_BINS, state, 2, 0, 0u);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_tail_kernel, dim3(grid), dim3(SEL_THREADS), 0, st, after, before, n, state, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(64), 0, st, state, n, k, result);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_select_apply(float* params, const float* before, int64_t n, float cut, uint8_t* mask, int64_t* n_kept, hipStream_t st) {
    const int vec = aligned16(params) && aligned16(before) && ((uintptr_t)mask & 3) == 0 ? 1 : 0;
    AMS_CHECK_HIP(hipMemsetAsync(n_kept, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(select_apply_kernel, dim3(select_grid(n)), dim3(SEL_THREADS), 0, st, params, before, n, cut, mask,
                       reinterpret_cast<unsigned long long*>(n_kept), vec);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// ---- encode ------------------------------------------------------------------------------------------------------------------------------
// WRITE = false: counts[segment] = set bits of the segment.  WRITE = true: counts holds the segments' exclusive offsets and *need the
// payload size; the payload is written only if it fits `cap`.  mask: flat uint8 in layout order (estart[v] = the first element of variable
// v there, estart[n_vars] = all of them), nullptr = every bit set.
template <bool WRITE>
__global__ void __launch_bounds__(ENC_THREADS) encode_kernel(const uint8_t* mask, const ams_delta_var* vars, const int64_t* estart, int n_vars,
                                                             int64_t mask_bytes, const float* params, const float* stats, int64_t* counts,
                                                             const int64_t* need, uint8_t* payload, int64_t cap) {
    __shared__ int64_t moff[AMS_DELTA_MAX_VARS], est[AMS_DELTA_MAX_VARS + 1];
    if (WRITE && *need > cap) return;                       // all or nothing (the same word for every thread)
    for (int v = threadIdx.x; v < n_vars; v += ENC_THREADS) moff[v] = vars[v].mask_offset;
    for (int v = threadIdx.x; v <= n_vars; v += ENC_THREADS) est[v] = estart[v];
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t seg = (int64_t)blockIdx.x * ENC_WAVES + (threadIdx.x >> 6);
    const int64_t b0 = seg * ENC_SEG, b1 = b0 + ENC_SEG < mask_bytes ? b0 + ENC_SEG : mask_bytes;
    if (b0 >= mask_bytes) return;
    int64_t k = WRITE ? counts[seg] : 0;
    int v = -1;
    for (int64_t base = b0; base < b1; base += 8) {
        const int64_t byte = base + (lane >> 3);
        bool set = false;
        int64_t e = 0;
        if (byte < b1) {
            if (v < 0) {                                    // last variable whose mask starts at or before this byte
                int lo = 0, hi = n_vars - 1;
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (moff[mid] <= byte) lo = mid; else hi = mid - 1;
                }
                v = lo;
            }
            while (v + 1 < n_vars && moff[v + 1] <= byte) ++v;
            e = (byte - moff[v]) * 8 + (lane & 7);
            if (e < est[v + 1] - est[v]) set = !mask || mask[est[v] + e] != 0;          // beyond the count: a padding bit, 0
        }
        const uint64_t bits = __ballot(set);
        if (WRITE) {
            if ((lane & 7) == 0 && byte < b1) payload[byte] = (uint8_t)(__brev((uint32_t)((bits >> lane) & 0xFFu)) >> 24);
            if (set) {
                const ams_delta_var d = vars[v];
                const float x = (d.region == AMS_REGION_PARAMS ? params : stats)[d.offset + e];
                const unsigned short hbits = __half_as_ushort(__float2half_rn(x));
                const int64_t pos = mask_bytes + 2 * (k + __popcll(bits & ((1ull << lane) - 1ull)));
                if (pos + 2 <= cap) {                       // (implied by *need <= cap)
                    payload[pos] = (uint8_t)(hbits & 0xFF);
                    payload[pos + 1] = (uint8_t)(hbits >> 8);
                }
            }
        }
        k += __popcll(bits);
    }
    if (!WRITE && lane == 0) counts[seg] = k;
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) encode_scan_kernel(int64_t* counts, int nseg, int64_t mask_bytes, int64_t* need,
                                                                         int64_t* payload_bytes) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    const int chunk = (nseg + BLOCK_SCAN_THREADS - 1) / BLOCK_SCAN_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < nseg ? s0 + chunk : nseg;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += counts[s];
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh);
    for (int s = s0; s < s1; ++s) { const int64_t c = counts[s]; counts[s] = run; run += c; }
    if (threadIdx.x == 0) *need = *payload_bytes = mask_bytes + 2 * total;
}

int64_t encode_segments(int64_t mask_bytes) { return mask_bytes > 0 ? cdiv64(mask_bytes, ENC_SEG) : 1; }

// table_dev (int64): [descriptors: 4 per variable][element starts: n_vars + 1]; work (int64): [payload size][segment counts -> offsets]
int launch_encode_delta(const uint8_t* mask, const int64_t* table_dev, int n_vars, int64_t mask_bytes, const float* params, const float* stats,
                        int64_t* work, uint8_t* payload, int64_t cap, int64_t* payload_bytes, hipStream_t st) {
    const ams_delta_var* vars = reinterpret_cast<const ams_delta_var*>(table_dev);
    const int64_t* estart = table_dev + 4 * (int64_t)n_vars;
    int64_t* need = work;
    int64_t* counts = work + 1;
    const int nseg = (int)encode_segments(mask_bytes);
    const int grid = cdiv(nseg, ENC_WAVES);
    hipLaunchKernelGGL(encode_kernel<false>, dim3(grid), dim3(ENC_THREADS), 0, st, mask, vars, estart, n_vars, mask_bytes, params, stats, counts,
                       (const int64_t*)need, payload, cap);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(encode_scan_kernel, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, st, counts, nseg, mask_bytes, need, payload_bytes);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(encode_kernel<true>, dim3(grid), dim3(ENC_THREADS), 0, st, mask, vars, estart, n_vars, mask_bytes, params, stats, counts,
                       (const int64_t*)need, payload, cap);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
