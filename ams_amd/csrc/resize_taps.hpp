// cv::resize's tap arithmetic for uint8 images, shared by the kernels that restate it (k_ingest.hip: a whole frame; k_replay.hip: the crop
// of a rescaled frame that is never formed).  The including file must be compiled with -ffp-contract=off: no fused multiply-add may merge
// the float roundings below.
#pragma once
#include "common.hpp"

namespace ams {

// the source step of one axis: cv::resize forms inv_scale = dsize / ssize and scale = 1. / inv_scale in double
inline __host__ __device__ double cv_step(int n_in, int n_out) { return 1.0 / ((double)n_out / (double)n_in); }

// one axis of cv::resize's tap table
__device__ __forceinline__ void fixed_tap(int d, double step, int n_in, bool zero_at_border, int& t0, int& t1, int& w0, int& w1) {
    float f = (float)(((double)d + 0.5) * step - 0.5);
    int s = (int)floorf(f);
    f = f - (float)s;
    if (zero_at_border && (s < 0 || s >= n_in - 1)) {
        s = s < 0 ? 0 : n_in - 1;
        f = 0.f;
    }
    t0 = s < 0 ? 0 : (s > n_in - 1 ? n_in - 1 : s);
    t1 = s + 1 < 0 ? 0 : (s + 1 > n_in - 1 ? n_in - 1 : s + 1);
    w0 = __float2int_rn((1.f - f) * 2048.f);       // cvRound: nearest, halves to even
    w1 = __float2int_rn(f * 2048.f);
}

// INTER_NEAREST: s = min(floor(d * step), size - 1)
__device__ __forceinline__ int nearest_tap(int d, double step, int n_in) {
    const long s = (long)floor((double)d * step);
    return (int)(s > n_in - 1 ? n_in - 1 : s);
}

// the vertical pass of the 8-bit INTER_LINEAR on two horizontally filtered rows
__device__ __forceinline__ uint8_t fixed_blend(int d0, int d1, int b0, int b1) {
    const int v = (((b0 * (d0 >> 4)) >> 16) + ((b1 * (d1 >> 4)) >> 16) + 2) >> 2;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

}  // namespace ams
