// The class table of the output head and the phi-score confusion count (SemanticNetwork.py:124-139), shared by k_head.hip (one pair of
// label maps) and k_replay.hip (the consecutive pairs of a replay memory in one launch).
#pragma once
#include "common.hpp"

namespace ams {

constexpr int kMaxK = 32;

struct ClassTable {
    int32_t idx[kMaxK];      // selected class ids
    int32_t lut[256];        // teacher id -> subset index, -1 = ignored
};

// One block's share of conf[before][after] += 1 over the pixels whose label is in the subset in BOTH maps: the blocks of grid.x stride
// over the n pixels, count in LDS (s_conf: kMaxK * kMaxK ints) and flush with integer atomics, so the counts do not depend on the order.
__device__ __forceinline__ void cross_conf_block(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t n, const ClassTable& ct,
                                                 int K, unsigned long long* __restrict__ conf, int* s_conf) {
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) s_conf[e] = 0;
    __syncthreads();
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int ka = ct.lut[a[i]], kb = ct.lut[b[i]];
        if (ka >= 0 && kb >= 0) atomicAdd(&s_conf[ka * K + kb], 1);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < K * K; e += blockDim.x)
        if (s_conf[e]) atomicAdd(&conf[e], (unsigned long long)s_conf[e]);
}

}  // namespace ams
