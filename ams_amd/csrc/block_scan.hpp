// Sum and exclusive prefix over the 256 threads of a block, in LDS (k_delta.hip, k_select.hip).
#pragma once

#include <stdint.h>

namespace ams {

constexpr int BLOCK_SCAN_THREADS = 256;

__device__ inline int64_t block_sum(int64_t v, int64_t* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = BLOCK_SCAN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const int64_t r = sh[0];
    __syncthreads();
    return r;
}

// exclusive prefix of v over the block's threads (Hillis-Steele in LDS; 256 entries)
__device__ inline int64_t block_exclusive_scan(int64_t v, int64_t* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < BLOCK_SCAN_THREADS; o <<= 1) {
        const int64_t add = (int)threadIdx.x >= o ? sh[threadIdx.x - o] : 0;
        __syncthreads();
        sh[threadIdx.x] += add;
        __syncthreads();
    }
    const int64_t r = sh[threadIdx.x] - v;
    __syncthreads();
    return r;
}

}  // namespace ams
