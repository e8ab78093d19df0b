// Edge-side model update: the downlink delta (mask bits + masked values as fp16, run.py:316-336) decoded back into the
// student's unfolded variables.  The inverse of pack_count_kernel / pack_scan_kernel / pack_write_kernel (k_elementwise.hip).
//
// Payload: for each variable of the layout, np.packbits(mask) (big-endian: bit 7 of a variable's first byte is its element 0; each
// variable starts on a byte, its last byte zero-padded), then the masked values of every variable in the same order as little-endian
// fp16.  The mask section has an odd length in both layouts of the 19-class model, so the fp16 values are read as byte pairs.
//
//   delta_count_kernel  one block per 2048-byte segment of the mask section: set bits of the segment (popcount on 64-bit words)
//   delta_scan_kernel   one block: exclusive scan of the segment counts, then the validation — mask bytes + 2 x set bits == payload
//                       bytes, and no padding bit set — written as the status word (0 = valid)
//   delta_apply_kernel  one block per segment: reads the status word first and writes nothing unless it is 0; each thread takes 64 mask
//                       bits, finds its first value by a block scan of the popcounts, and each set bit's variable by a binary search
//                       of the variables' mask offsets held in LDS
#include "common.hpp"
#include "kernels.hpp"
#include "block_scan.hpp"
#include "delta_walk.hpp"                                   // DELTA_THREADS, DELTA_SEG, mask_word: shared with k_delta_q8.hip

#include <hip/hip_fp16.h>

namespace ams {

__global__ void __launch_bounds__(DELTA_THREADS) delta_count_kernel(const uint8_t* payload, int64_t end, int64_t* counts) {
    __shared__ int64_t sh[DELTA_THREADS];
    const int64_t b = blockIdx.x * DELTA_SEG + 8 * (int64_t)threadIdx.x;
    const int64_t c = b < end ? __popcll(mask_word(payload, b, end)) : 0;
    const int64_t t = block_sum(c, sh);
    if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

__global__ void __launch_bounds__(DELTA_THREADS) delta_scan_kernel(int64_t* counts, int nseg, const ams_delta_var* vars, int n_vars,
                                                                   const uint8_t* payload, int64_t payload_bytes, int64_t mask_bytes,
                                                                   int64_t* n_applied, int32_t* status) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int bad_pad;
    if (threadIdx.x == 0) bad_pad = 0;
    // segment counts -> exclusive offsets: each thread owns a contiguous chunk, the chunk sums are scanned across the block
    const int chunk = (nseg + DELTA_THREADS - 1) / DELTA_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < nseg ? s0 + chunk : nseg;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += counts[s];
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh);
    for (int s = s0; s < s1; ++s) { const int64_t c = counts[s]; counts[s] = run; run += c; }
    // padding bits: the low 8 - count % 8 bits of a variable's last mask byte
    const int64_t readable = payload_bytes < mask_bytes ? payload_bytes : mask_bytes;
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) {
        const int64_t n = vars[v].count;
        const int r = (int)(n & 7);
        const int64_t byte = vars[v].mask_offset + (n >> 3);
        if (r && byte < readable && (payload[byte] & (0xFFu >> r))) atomicOr(&bad_pad, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int32_t st = mask_bytes + 2 * total != payload_bytes ? AMS_DELTA_BAD_SIZE : bad_pad ? AMS_DELTA_BAD_PADDING : AMS_DELTA_OK;
        *status = st;
        *n_applied = st == AMS_DELTA_OK ? total : 0;
    }
}

__global__ void __launch_bounds__(DELTA_THREADS) delta_apply_kernel(const uint8_t* payload, int64_t mask_bytes, const int64_t* offs,
                                                                    const ams_delta_var* vars, int n_vars, float* params, int64_t n_params,
                                                                    float* stats, int64_t n_stats, const int32_t* status) {
    __shared__ int64_t sh[DELTA_THREADS];
    __shared__ int64_t moff[AMS_DELTA_MAX_VARS];
    if (*status != AMS_DELTA_OK) return;                    // all or nothing: a payload that failed validation writes no element
    for (int v = threadIdx.x; v < n_vars; v += DELTA_THREADS) moff[v] = vars[v].mask_offset;
    const int64_t b = blockIdx.x * DELTA_SEG + 8 * (int64_t)threadIdx.x;
    uint64_t w = b < mask_bytes ? mask_word(payload, b, mask_bytes) : 0;
    int64_t k = offs[blockIdx.x] + block_exclusive_scan(__popcll(w), sh);       // (the scan's barriers also publish moff)
    int v = -1;
    while (w) {
        const int lz = __clzll(w);
        w &= ~(1ull << (63 - lz));
        const int64_t byte = b + (lz >> 3);
        if (v < 0) {                                        // last variable whose mask starts at or before this byte
            int lo = 0, hi = n_vars - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (moff[mid] <= byte) lo = mid; else hi = mid - 1;
            }
            v = lo;
        }
        while (v + 1 < n_vars && moff[v + 1] <= byte) ++v;
        const int64_t e = (byte - moff[v]) * 8 + (lz & 7);
        const uint8_t* q = payload + mask_bytes + 2 * k++;
        const ams_delta_var d = vars[v];
        if (e < 0 || e >= d.count) continue;                 // a padding bit (validation rejects those) or a malformed table
        const float val = __half2float(__ushort_as_half((unsigned short)(q[0] | (q[1] << 8))));
        if (d.region == AMS_REGION_PARAMS) {
            if (d.offset + e < n_params) params[d.offset + e] = val;
        } else if (d.region == AMS_REGION_STATS) {
            if (d.offset + e < n_stats) stats[d.offset + e] = val;
        }
    }
}

int64_t delta_segments(int64_t mask_bytes) { return mask_bytes > 0 ? cdiv64(mask_bytes, DELTA_SEG) : 1; }

// the count pass alone, for the q8 decoder (k_delta_q8.hip): the mask section is the same
int launch_delta_count(const uint8_t* payload, int64_t readable, int nseg, int64_t* counts, hipStream_t st) {
    hipLaunchKernelGGL(delta_count_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, payload, readable, counts);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// scratch (int64): [descriptor table: 4 per variable][segment counts -> offsets]
int launch_apply_delta(const uint8_t* payload, int64_t payload_bytes, const ams_delta_var* vars_dev, int n_vars, int64_t mask_bytes,
                       float* params, int64_t n_params, float* stats, int64_t n_stats, int64_t* counts, int64_t* n_applied, int32_t* status,
                       hipStream_t st) {
    const int nseg = (int)delta_segments(mask_bytes);
    const int64_t readable = payload_bytes < mask_bytes ? payload_bytes : mask_bytes;
    hipLaunchKernelGGL(delta_count_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, payload, readable, counts);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(delta_scan_kernel, dim3(1), dim3(DELTA_THREADS), 0, st, counts, nseg, vars_dev, n_vars, payload, payload_bytes,
                       mask_bytes, n_applied, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(delta_apply_kernel, dim3(nseg), dim3(DELTA_THREADS), 0, st, payload, mask_bytes, counts, vars_dev, n_vars, params,
                       n_params, stats, n_stats, status);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
