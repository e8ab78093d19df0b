// How the delta kernels walk a mask section (k_delta.hip, k_delta_q8.hip): 2048-byte segments, one block each; a thread takes 8 mask
// bytes = 64 elements as one word, and finds a bit's variable in the variables' mask offsets held in LDS.
#pragma once

#include "block_scan.hpp"

namespace ams {

constexpr int DELTA_THREADS = BLOCK_SCAN_THREADS;
constexpr int64_t DELTA_SEG = 8 * DELTA_THREADS;          // mask bytes per segment: 8 per thread

// mask bytes [b, b + 8) clipped at e, as one word in element order: bit 63 = bit 7 of byte b
__device__ inline uint64_t mask_word(const uint8_t* p, int64_t b, int64_t e) {
    if (b + 8 <= e && ((uintptr_t)(p + b) & 7) == 0) return __builtin_bswap64(*reinterpret_cast<const uint64_t*>(p + b));
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k) w = (w << 8) | (uint64_t)(b + k < e ? p[b + k] : 0);
    return w;
}

// the last variable whose mask starts at or before `byte` (variables without elements share their successor's offset and are passed
// over); v: the answer for an earlier byte of the same walk, or -1
__device__ inline int delta_var_of_byte(const int64_t* moff, int n_vars, int64_t byte, int v) {
    if (v < 0) {
        int lo = 0, hi = n_vars - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (moff[mid] <= byte) lo = mid; else hi = mid - 1;
        }
        v = lo;
    }
    while (v + 1 < n_vars && moff[v + 1] <= byte) ++v;
    return v;
}

}  // namespace ams
