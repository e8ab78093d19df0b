// The server's replay memory on the device (reference run.py:136-137 frame_memory / label_memory, utils/utils.py:129-185 mini_batch): a ring
// of uint8 frame / label slots in HBM, and one launch that builds a mini-batch from it.
//
//   replay_gather_kernel          per batch entry (blockIdx.z) a descriptor {slot, th, tw, top, left, flip}: the crop [top, top + H) x
//                                 [left, left + W) of cv2.resize(frame, (tw, th)) [INTER_LINEAR] / cv2.resize(label, ..., INTER_NEAREST),
//                                 mirrored when flip.  A tap table depends on the output index alone, so the taps are evaluated at
//                                 (top + y, left + x) and the rescaled frame is never formed.  The cases of launch_resize_u8, per sample:
//                                 equal sizes copy, an exact 2x down-scale is the box average, anything else the 11-bit fixed-point bilinear
//                                 form (resize_taps.hpp).  The case is uniform per sample: the branch is on blockIdx.z, not per lane.
//                                 The copy case, what a scale list of [1] over frames at the network size hits on every step, is byte
//                                 traffic: 16 bytes per lane where the row pitches, the crop origin and the bases allow it.
//   replay_gather_rows_kernel     whole f32 slots (the cached teacher logits of the drawn frames) by the same table
//   replay_gather_logits_kernel   f32 [Hs, Ws, C] slots (teacher logits cached at the frame size) through the same descriptors: the crop of the
//                                 logits rescaled to (th, tw), mirrored when flip, at the label size [B, H, W, C].  The rule is this
//                                 project's (include/ams_hip.h: the reference never resamples logits): cv2.resize's float INTER_LINEAR
//                                 geometry, taps in double (linear_tap), the blend in f32 with every operation rounded once (logits_blend).
//                                 A block owns a segment of an output row: its x-taps go to LDS once per pixel, then the segment's seg * C
//                                 floats are walked flat (FlatWalk), so that stores are contiguous and the four tap loads of neighbouring
//                                 lanes fall in the same lines.  Equal sizes copy (nothing of a neighbouring pixel enters), 16 bytes per
//                                 lane where the pitches, the origin and the bases allow it and the sample is not mirrored; with channels a
//                                 multiple of 4 (a slot that holds the K selected channels, K = 4 or 8) every pixel starts on 16 bytes and
//                                 the mirrored copy moves 16 bytes per lane too.
//   replay_gather_logits_lowres_kernel
//                                 f32 [lh, lw, C] slots (teacher logits cached on a grid no larger than the frame) through the same
//                                 descriptors: the slot behaves, bit for bit, as a frame-size slot that holds its own align-corners
//                                 upsample U (the soft loss kernel's: src_tap / bilerp of head_common.hpp, a grid point the cached sample
//                                 itself), and replay_gather_logits_kernel's rule (the same linear_tap and logits_blend) is applied to U,
//                                 which is never stored.  Same block shape and walk: the y-side (the rule's two rows of U, and for each the
//                                 two cached rows and ty) is uniform per block, the x-side (per tap of the rule two element offsets into a
//                                 cached row and tx, plus wx) goes to LDS once per pixel.  Where both rows of U fall between the same two
//                                 cached rows (15 of 16 output rows for a 33 x 65 cache of 512 x 1024 frames) the x-interpolated pair is
//                                 formed once and serves both: 8 loads per float instead of 16, the same operations on the same values.
//                                 The loads hit L1 / L2 (a 33 x 65 x 19 slot is 163 KB): HBM sees the stores alone, the time is the tap loads'.
//   replay_pack_logits_kernel     f32 [th, tw, NC] teacher logits -> a slot in the selected layout f32 [th, tw, K], channel k = input channel
//                                 idx[k]: what append does to logits that are already on the device.  A block owns a run of pixels of one
//                                 row: the run's run * NC input floats go through LDS with contiguous loads, the run * K output floats
//                                 leave contiguously (FlatWalk over them).  16-byte loads and 16-byte stores where the bases and the row
//                                 pitches allow them, each chosen by the launcher for the whole launch.  Copies only: every bit pattern
//                                 survives.
//   teacher_labels_kernel         f32 [lh, lw, NC] teacher logits -> the uint8 [Hs, Ws] label map a slot stores beside them: the argmax over
//                                 every class (the first maximum, tf.argmax's) of the same upsample U, what the reference's teacher calls
//                                 its predictions (utils/graph_utils.py:143-152).  append(frame, None, logits) fills the label slot with it.
//   cross_confusion_pairs_kernel  the K x K phi-score confusion matrices of n pairs of label slots in one launch (blockIdx.z = the pair)
//
// Shared by the kernels, each written once: the descriptor check (replay_sample_ok on the device, check_replay_samples on the host), the
// division-free flat walk over a block's floats (FlatWalk), one axis of the logits rule and its blend (linear_tap, logits_blend), U at one
// point (upsampled).  Every descriptor is checked on the host before the launch (check_replay_samples); the kernels check it again against
// the sizes they are given (replay_sample_ok) and skip a sample that fails, so that a table that changed between the two cannot reach
// outside the slots.
#include "common.hpp"
#include "kernels.hpp"
#include "resize_taps.hpp"
#include "cross_conf.hpp"
#include "head_common.hpp"

namespace ams {

struct ReplayGeom {
    int capacity, Hs, Ws, H, W;
    int64_t frame_stride, label_stride;          // bytes from one slot to the next
    int vec;                                     // pitches and bases allow 16-byte accesses
};

// the descriptor check: the slot exists and the H x W crop lies inside the th x tw image
__device__ __forceinline__ bool replay_sample_ok(const ams_replay_sample& d, int capacity, int H, int W) {
    return d.slot >= 0 && d.slot < capacity && d.th > 0 && d.tw > 0 && d.top >= 0 && d.left >= 0 && d.top <= d.th - H && d.left <= d.tw - W;
}

// The flat walk: a block of `block` threads walks n * C floats, thread t taking the elements i = t, t + block, ...; element i is channel c of
// pixel p.  One division when the walk starts, none inside the loop: next() follows i += block.
// (c < C and dc = block % C < C, with dp = 0 and dc = block where C > block: c + dc < 2 C, so one conditional subtraction suffices)
struct FlatWalk {
    int p, c, dp, dc, C;
    __device__ __forceinline__ FlatWalk(int t, int C_, int block) : p(t / C_), c(t - p * C_), dp(block / C_), dc(block - dp * C_), C(C_) {}
    __device__ __forceinline__ void next() {
        p += dp; c += dc;
        if (c >= C) { c -= C; ++p; }
    }
};

__global__ __launch_bounds__(256) void replay_gather_kernel(const uint8_t* __restrict__ frame_slots, const uint8_t* __restrict__ label_slots,
                                                            const ams_replay_sample* __restrict__ samples, ReplayGeom g,
                                                            uint8_t* __restrict__ frames_out, uint8_t* __restrict__ labels_out) {
    const int b = blockIdx.z, oy = blockIdx.y;
    const ams_replay_sample d = samples[b];
    if (!replay_sample_ok(d, g.capacity, g.H, g.W)) return;
    const uint8_t* fsrc = frame_slots + (int64_t)d.slot * g.frame_stride;
    const uint8_t* lsrc = label_slots + (int64_t)d.slot * g.label_stride;
    uint8_t* fdst = frames_out + ((int64_t)b * g.H + oy) * g.W * 3;
    uint8_t* ldst = labels_out + ((int64_t)b * g.H + oy) * g.W;
    const bool same = d.th == g.Hs && d.tw == g.Ws;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;

    if (same && g.vec && !d.flip && (d.left & 15) == 0) {
        // whole rows of bytes: the frame row's 16-byte pieces first, the label row's behind them
        const int fc = g.W * 3 / 16, lc = g.W / 16;
        const uint8_t* frow = fsrc + ((int64_t)(d.top + oy) * g.Ws + d.left) * 3;
        const uint8_t* lrow = lsrc + (int64_t)(d.top + oy) * g.Ws + d.left;
        for (int c = t; c < fc + lc; c += gridDim.x * blockDim.x) {
            if (c < fc) reinterpret_cast<uint4*>(fdst)[c] = reinterpret_cast<const uint4*>(frow)[c];
            else reinterpret_cast<uint4*>(ldst)[c - fc] = reinterpret_cast<const uint4*>(lrow)[c - fc];
        }
        return;
    }

    if (t >= g.W) return;
    const int cy = d.top + oy, cx = d.left + (d.flip ? g.W - 1 - t : t);          // the pixel of the rescaled image
    uint8_t* fout = fdst + (int64_t)t * 3;
    if (same) {
        const uint8_t* p = fsrc + ((int64_t)cy * g.Ws + cx) * 3;
        fout[0] = p[0]; fout[1] = p[1]; fout[2] = p[2];
        ldst[t] = lsrc[(int64_t)cy * g.Ws + cx];
        return;
    }
    const double sy = cv_step(g.Hs, d.th), sx = cv_step(g.Ws, d.tw);
    ldst[t] = lsrc[(int64_t)nearest_tap(cy, sy, g.Hs) * g.Ws + nearest_tap(cx, sx, g.Ws)];
    if (g.Hs == 2 * d.th && g.Ws == 2 * d.tw) {
        const uint8_t* p0 = fsrc + ((int64_t)(2 * cy) * g.Ws + 2 * cx) * 3;
        const uint8_t* p1 = p0 + (int64_t)g.Ws * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) fout[c] = (uint8_t)(((int)p0[c] + (int)p0[3 + c] + (int)p1[c] + (int)p1[3 + c] + 2) >> 2);
        return;
    }
    int y0, y1, x0, x1, b0, b1, a0, a1;
    fixed_tap(cy, sy, g.Hs, false, y0, y1, b0, b1);
    fixed_tap(cx, sx, g.Ws, true, x0, x1, a0, a1);
    const uint8_t* p00 = fsrc + ((int64_t)y0 * g.Ws + x0) * 3;
    const uint8_t* p01 = fsrc + ((int64_t)y0 * g.Ws + x1) * 3;
    const uint8_t* p10 = fsrc + ((int64_t)y1 * g.Ws + x0) * 3;
    const uint8_t* p11 = fsrc + ((int64_t)y1 * g.Ws + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        fout[c] = fixed_blend((int)p00[c] * a0 + (int)p01[c] * a1, (int)p10[c] * a0 + (int)p11[c] * a1, b0, b1);
}

__global__ __launch_bounds__(256) void replay_gather_rows_kernel(const float* __restrict__ slots, int64_t slot_stride, int capacity,
                                                                 const ams_replay_sample* __restrict__ samples, int64_t n, int vec,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.z;
    const int slot = samples[b].slot;
    if (slot < 0 || slot >= capacity) return;
    const float* src = slots + (int64_t)slot * slot_stride;
    float* dst = out + (int64_t)b * n;
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
    if (vec) {
        for (int64_t i = t; i < (n >> 2); i += step) st4(dst + 4 * i, ld4(src + 4 * i));
    } else {
        for (int64_t i = t; i < n; i += step) dst[i] = src[i];
    }
}

constexpr int kLogitsSeg = 128;                  // pixels of an output row per block (19 classes: 2432 floats, 9.5 per thread)

struct LogitsGeom {
    int capacity, Hs, Ws, C, H, W;
    int64_t slot_stride;                         // f32 elements from one slot to the next
    int vec;                                     // pitches and bases allow 16-byte accesses
};

// one axis of the logits rule: the source position of output index d in double, the weight of the second tap in f32; past either border
// the nearest sample alone
__device__ __forceinline__ void linear_tap(int d, int n_in, int n_out, int& s0, int& s1, float& w) {
    const double f = ((double)d + 0.5) * ((double)n_in / (double)n_out) - 0.5;
    const double fl = floor(f);
    int s = (int)fl;
    w = (float)(f - fl);
    if (s < 0) { s = 0; w = 0.f; }
    if (s >= n_in - 1) { s = n_in - 1; w = 0.f; }
    s0 = s;
    s1 = s + 1 < n_in - 1 ? s + 1 : n_in - 1;
}

// the blend of the logits rule: u[row][column] of the four taps, the weights of the second column and the second row; every operation rounded once
__device__ __forceinline__ float logits_blend(float u00, float u01, float u10, float u11, float wx, float wy) {
    const float mx = __fsub_rn(1.f, wx), my = __fsub_rn(1.f, wy);
    const float r0 = __fadd_rn(__fmul_rn(u00, mx), __fmul_rn(u01, wx));
    const float r1 = __fadd_rn(__fmul_rn(u10, mx), __fmul_rn(u11, wx));
    return __fadd_rn(__fmul_rn(r0, my), __fmul_rn(r1, wy));
}

__global__ __launch_bounds__(256) void replay_gather_logits_kernel(const float* __restrict__ slots, const ams_replay_sample* __restrict__ samples,
                                                                   LogitsGeom g, float* __restrict__ out) {
    __shared__ int s_x0[kLogitsSeg], s_x1[kLogitsSeg];          // element offsets of a pixel's two taps inside a source row
    __shared__ float s_wx[kLogitsSeg];
    const int b = blockIdx.z, oy = blockIdx.y, x_first = blockIdx.x * kLogitsSeg, t = threadIdx.x;
    const ams_replay_sample d = samples[b];
    if (!replay_sample_ok(d, g.capacity, g.H, g.W)) return;
    const int seg = g.W - x_first < kLogitsSeg ? g.W - x_first : kLogitsSeg;
    const int n = seg * g.C;
    const int64_t pitch = (int64_t)g.Ws * g.C;
    const float* src = slots + (int64_t)d.slot * g.slot_stride;
    float* dst = out + (((int64_t)b * g.H + oy) * g.W + x_first) * g.C;
    const int cy = d.top + oy;                                   // the row of the rescaled logits
    const bool same = d.th == g.Hs && d.tw == g.Ws;              // (every branch on d is uniform over the block)

    if (same && !d.flip) {
        const float* row = src + cy * pitch + (int64_t)(d.left + x_first) * g.C;
        if (g.vec && (((int64_t)d.left * g.C) & 3) == 0) {
            for (int i = t; i < (n >> 2); i += 256) st4(dst + 4 * i, ld4(row + 4 * i));
        } else {
            for (int i = t; i < n; i += 256) dst[i] = row[i];
        }
        return;
    }

    if (t < seg) {
        const int x = x_first + t, cx = d.left + (d.flip ? g.W - 1 - x : x);
        if (same) {
            s_x0[t] = cx * g.C;
        } else {
            int x0, x1;
            float wx;
            linear_tap(cx, g.Ws, d.tw, x0, x1, wx);
            s_x0[t] = x0 * g.C;
            s_x1[t] = x1 * g.C;
            s_wx[t] = wx;
        }
    }
    __syncthreads();

    FlatWalk w(t, g.C, 256);                                     // over the segment's floats
    if (same) {                                                  // the mirrored copy
        const float* row = src + cy * pitch;
        if (g.vec && (g.C & 3) == 0) {                           // every pixel starts on 16 bytes: whole quads of one pixel
            const int q = g.C >> 2;
            for (int i = t; i < (n >> 2); i += 256) {
                const int pp = i / q;
                st4(dst + 4 * i, ld4(row + s_x0[pp] + 4 * (i - pp * q)));
            }
            return;
        }
        for (int i = t; i < n; i += 256, w.next()) dst[i] = row[s_x0[w.p] + w.c];
        return;
    }
    int y0, y1;
    float wy;
    linear_tap(cy, g.Hs, d.th, y0, y1, wy);
    const float* row0 = src + y0 * pitch;
    const float* row1 = src + y1 * pitch;
    for (int i = t; i < n; i += 256, w.next()) {
        const int a0 = s_x0[w.p] + w.c, a1 = s_x1[w.p] + w.c;
        dst[i] = logits_blend(row0[a0], row0[a1], row1[a0], row1[a1], s_wx[w.p], wy);
    }
}

struct LowresGeom {
    int capacity, lh, lw, C, Hs, Ws, H, W;       // slots f32 [lh, lw, C], frames Hs x Ws, crop H x W
    int64_t slot_stride;                         // f32 elements from one slot to the next
    float sy, sx;                                // (lh-1)/(Hs-1), (lw-1)/(Ws-1) as f32: soft_teacher_geom's scales for a teacher grid read at Hs x Ws
};

// U at one point from the four cached samples around it: the soft loss kernel's two branches (k_head.hip), the cached sample itself on a grid point
__device__ __forceinline__ float upsampled(float tl, float tr, float bl, float br, float tx, float ty) {
    const float v = bilerp(tl, tr, bl, br, tx, ty);
    return (tx == 0.f && ty == 0.f) ? tl : v;
}

__global__ __launch_bounds__(256) void replay_gather_logits_lowres_kernel(const float* __restrict__ slots, const ams_replay_sample* __restrict__ samples,
                                                                          LowresGeom g, float* __restrict__ out) {
    // per pixel and tap of the frame-size rule (one tap in the copy case): element offsets of U's two cached columns inside a cached row, tx
    __shared__ int s_lo[2][kLogitsSeg], s_hi[2][kLogitsSeg];
    __shared__ float s_tx[2][kLogitsSeg], s_wx[kLogitsSeg];
    const int b = blockIdx.z, oy = blockIdx.y, x_first = blockIdx.x * kLogitsSeg, t = threadIdx.x;
    const ams_replay_sample d = samples[b];
    if (!replay_sample_ok(d, g.capacity, g.H, g.W)) return;
    if (!(g.lh >= 1 && g.lh <= g.Hs && g.lw >= 1 && g.lw <= g.Ws && g.slot_stride >= (int64_t)g.lh * g.lw * g.C)) return;
    const int seg = g.W - x_first < kLogitsSeg ? g.W - x_first : kLogitsSeg;
    const int n = seg * g.C;
    const int64_t pitch = (int64_t)g.lw * g.C;
    const float* src = slots + (int64_t)d.slot * g.slot_stride;
    float* dst = out + (((int64_t)b * g.H + oy) * g.W + x_first) * g.C;
    const int cy = d.top + oy;                                   // the row of the rescaled logits
    const bool same = d.th == g.Hs && d.tw == g.Ws;              // (every branch on d is uniform over the block)

    // src_tap of a position p <= n_src - 1 of U stays inside the cached axis: p * scale <= (n_in - 1) * (1 + 2^-23) < n_in, so lo <= n_in - 1
    if (t < seg) {
        const int x = x_first + t, cx = d.left + (d.flip ? g.W - 1 - x : x);
        int lo, hi;
        float tx;
        if (same) {
            src_tap(cx, g.sx, g.lw, lo, hi, tx);
            s_lo[0][t] = lo * g.C; s_hi[0][t] = hi * g.C; s_tx[0][t] = tx;
        } else {
            int x0, x1;
            float wx;
            linear_tap(cx, g.Ws, d.tw, x0, x1, wx);
            src_tap(x0, g.sx, g.lw, lo, hi, tx);
            s_lo[0][t] = lo * g.C; s_hi[0][t] = hi * g.C; s_tx[0][t] = tx;
            src_tap(x1, g.sx, g.lw, lo, hi, tx);
            s_lo[1][t] = lo * g.C; s_hi[1][t] = hi * g.C; s_tx[1][t] = tx;
            s_wx[t] = wx;
        }
    }
    __syncthreads();

    FlatWalk w(t, g.C, 256);                                     // over the segment's floats
    if (same) {                                                  // U's window itself, mirrored when flip
        int l0, h0;
        float ty;
        src_tap(cy, g.sy, g.lh, l0, h0, ty);
        const float* top = src + l0 * pitch;
        const float* bot = src + h0 * pitch;
        for (int i = t; i < n; i += 256, w.next()) {
            const int a = s_lo[0][w.p] + w.c, e = s_hi[0][w.p] + w.c;
            dst[i] = upsampled(top[a], top[e], bot[a], bot[e], s_tx[0][w.p], ty);
        }
        return;
    }
    int y0, y1, l0, h0, l1, h1;
    float wy, ty0, ty1;
    linear_tap(cy, g.Hs, d.th, y0, y1, wy);
    src_tap(y0, g.sy, g.lh, l0, h0, ty0);
    src_tap(y1, g.sy, g.lh, l1, h1, ty1);
    const float* top0 = src + l0 * pitch;
    const float* bot0 = src + h0 * pitch;
    const float* top1 = src + l1 * pitch;
    const float* bot1 = src + h1 * pitch;
    // the rescale loop: ua / ub = the two rows of U at the rule's two x-taps.  shared: both rows of U lie between the same two cached rows
    // (top1 == top0, bot1 == bot0), so bilerp's x-interpolated pair is formed once and serves both
    auto rescale = [&](auto shared) {
        for (int i = t; i < n; i += 256, w.next()) {
            float ua[2], ub[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int a = s_lo[k][w.p] + w.c, e = s_hi[k][w.p] + w.c;
                const float tx = s_tx[k][w.p];
                if constexpr (decltype(shared)::value) {
                    const float tl = top0[a], bl = bot0[a];
                    const float tp = __fadd_rn(tl, __fmul_rn(__fsub_rn(top0[e], tl), tx));          // bilerp's top and bot
                    const float bt = __fadd_rn(bl, __fmul_rn(__fsub_rn(bot0[e], bl), tx));
                    const float df = __fsub_rn(bt, tp);
                    const float va = __fadd_rn(tp, __fmul_rn(df, ty0)), vb = __fadd_rn(tp, __fmul_rn(df, ty1));
                    ua[k] = (tx == 0.f && ty0 == 0.f) ? tl : va;
                    ub[k] = (tx == 0.f && ty1 == 0.f) ? tl : vb;
                } else {
                    ua[k] = upsampled(top0[a], top0[e], bot0[a], bot0[e], tx, ty0);
                    ub[k] = upsampled(top1[a], top1[e], bot1[a], bot1[e], tx, ty1);
                }
            }
            dst[i] = logits_blend(ua[0], ua[1], ub[0], ub[1], s_wx[w.p], wy);
        }
    };
    if (l0 == l1 && h0 == h1) rescale(std::true_type());         // (uniform over the block)
    else rescale(std::false_type());
}

constexpr int kPackFloats = 4096;               // input floats of a run in LDS (16 KB)
constexpr int kPackRun = 128;                   // pixels per block at most; fewer when NC > 32

struct PackGeom {
    int th, tw, NC, K, run;                      // run: pixels per block, a multiple of 4 (a run's floats start on 16 bytes when the row does)
    int vec_in, vec_out;
    int idx[kMaxK];
};

__global__ __launch_bounds__(256) void replay_pack_logits_kernel(const float* __restrict__ in, PackGeom g, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float s_in[kPackFloats];
    __shared__ int s_idx[kMaxK];
    const int y = blockIdx.y, x_first = blockIdx.x * g.run, t = threadIdx.x;
    if (y >= g.th || x_first >= g.tw) return;                   // (uniform over the block)
    const int seg = g.tw - x_first < g.run ? g.tw - x_first : g.run;
    const int n_in = seg * g.NC, n_out = seg * g.K;
    const float* src = in + ((int64_t)y * g.tw + x_first) * g.NC;
    float* dst = out + ((int64_t)y * g.tw + x_first) * g.K;
#pragma unroll
    for (int k = 0; k < kMaxK; ++k)
        if (t == k) s_idx[k] = g.idx[k];                         // (constant k: the table stays in scalar registers)
    if (g.vec_in) {
        for (int i = t; i < (n_in >> 2); i += 256) *reinterpret_cast<float4*>(s_in + 4 * i) = ld4(src + 4 * i);
    } else {
        for (int i = t; i < n_in; i += 256) s_in[i] = src[i];
    }
    __syncthreads();
    if (g.vec_out) {
        for (int i = t; i < (n_out >> 2); i += 256) {
            int p = 4 * i / g.K, k = 4 * i - p * g.K;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = s_in[p * g.NC + s_idx[k]];
                if (++k == g.K) { k = 0; ++p; }
            }
            st4(dst + 4 * i, make_float4(v[0], v[1], v[2], v[3]));
        }
    } else {
        FlatWalk w(t, g.K, 256);                                 // over the run's output floats
        for (int i = t; i < n_out; i += 256, w.next()) dst[i] = s_in[w.p * g.NC + s_idx[w.c]];
    }
}

constexpr int kLabelSeg = 128;                  // pixels of an output row per block at most, one per lane
constexpr int kLabelLdsBytes = 32 * 1024;       // staged cached samples per block at most (the launcher narrows the segment until they fit)

struct LabelGeom {
    int n, lh, lw, NC, Hs, Ws;                   // items f32 [lh, lw, NC], labels Hs x Ws
    int seg;                                     // pixels of a row per block: 4 .. kLabelSeg, a power of two
    int lds_floats;                              // dynamic LDS the launch was given
    int vec;                                     // every segment of every row of every item starts on 4 bytes: packed stores
    int64_t slot_stride, out_stride;             // f32 elements / bytes from one item to the next
    float sy, sx;                                // (lh-1)/(Hs-1), (lw-1)/(Ws-1) as f32: soft_teacher_geom's scales
};

// label(Y, X) = argmax_c U(Y, X, c), U = the align-corners upsample of replay_gather_logits_lowres_kernel (Stage U).  A block owns a segment
// of one output row: the y-side (two cached rows, ty) is the same for the whole block, and the segment's pixels fall between the cached
// columns lo(first pixel) .. hi(last pixel) (src_tap is monotone in the position).  Those columns of the two rows, every class, go to LDS
// with contiguous loads (a 128-pixel segment of a 1024-wide row over a 65-wide cache: 10 columns x 2 rows x 19 floats); then each lane
// scans the classes of its own pixel out of LDS.  A pixel's stride in LDS is NC | 1 floats: odd, so that lanes on neighbouring cached
// columns (all of them where the cache has the frame's size) fall on different banks.
__global__ __launch_bounds__(kLabelSeg) void teacher_labels_kernel(const float* __restrict__ logits, LabelGeom g, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float s_stage[];
    const int b = blockIdx.z, Y = blockIdx.y, x_first = blockIdx.x * g.seg, t = threadIdx.x;
    // the launcher's checks again (uniform over the block)
    if (!(g.n >= 1 && b < g.n && g.lh >= 1 && g.lh <= g.Hs && g.lw >= 1 && g.lw <= g.Ws && g.NC >= 1 && g.NC <= 255 &&
          g.slot_stride >= (int64_t)g.lh * g.lw * g.NC && g.out_stride >= (int64_t)g.Hs * g.Ws))
        return;
    if (!(g.seg >= 1 && g.seg <= kLabelSeg) || Y >= g.Hs || x_first >= g.Ws) return;
    const int seg = g.Ws - x_first < g.seg ? g.Ws - x_first : g.seg;
    const int ld = g.NC | 1;

    int l0, h0, c_lo, c_hi, lo_last, unused;
    float ty, tx_unused;
    src_tap(Y, g.sy, g.lh, l0, h0, ty);
    src_tap(x_first, g.sx, g.lw, c_lo, unused, tx_unused);
    src_tap(x_first + seg - 1, g.sx, g.lw, lo_last, c_hi, tx_unused);
    const int ncols = c_hi - c_lo + 1;
    const int rows = h0 == l0 ? 1 : 2;
    // (src_tap keeps lo <= n_in - 1 for positions of U, see replay_gather_logits_lowres_kernel; a geometry that broke that, or a launch with
    // less LDS than the segment needs, writes nothing)
    if (l0 < 0 || l0 >= g.lh || c_lo < 0 || lo_last > c_hi || ncols < 1 || (int64_t)rows * ncols * ld > g.lds_floats) return;

    const float* src = logits + (int64_t)b * g.slot_stride;
    const int64_t pitch = (int64_t)g.lw * g.NC;
    const int n_row = ncols * g.NC;
    for (int r = 0; r < rows; ++r) {
        const float* row = src + (r ? h0 : l0) * pitch + (int64_t)c_lo * g.NC;
        float* dst = s_stage + r * ncols * ld;
        FlatWalk w(t, g.NC, kLabelSeg);                          // over the row piece's floats: class c of cached column p
        for (int i = t; i < n_row; i += kLabelSeg, w.next()) dst[w.p * ld + w.c] = row[i];
    }
    __syncthreads();

    // lanes past the segment scan its last pixel and store nothing: every lane of a wave reaches the shuffles below
    const int x = x_first + (t < seg ? t : seg - 1);
    int lo, hi;
    float tx;
    src_tap(x, g.sx, g.lw, lo, hi, tx);
    const float* top = s_stage + (lo - c_lo) * ld;
    const float* bot = top + (rows - 1) * ncols * ld;
    const int e = (hi - lo) * ld;
    // tf.argmax: the first maximum.  A strict > from class 0 keeps the lowest index of equal values (-0.0 == +0.0)
    float best = upsampled(top[0], top[e], bot[0], bot[e], tx, ty);
    int label = 0;
    for (int c = 1; c < g.NC; ++c) {
        const float v = upsampled(top[c], top[e + c], bot[c], bot[e + c], tx, ty);
        if (v > best) { best = v; label = c; }
    }

    uint8_t* dst = out + (int64_t)b * g.out_stride + (int64_t)Y * g.Ws + x_first;
    if (g.vec) {                                                 // (then Ws and seg are multiples of 4: so is every segment's length)
        // four pixels of four neighbouring lanes leave as one word
        const uint32_t l1 = (uint32_t)__shfl_down(label, 1), l2 = (uint32_t)__shfl_down(label, 2), l3 = (uint32_t)__shfl_down(label, 3);
        if ((t & 3) == 0 && t + 3 < seg) *reinterpret_cast<uint32_t*>(dst + t) = (uint32_t)label | (l1 << 8) | (l2 << 16) | (l3 << 24);
        return;
    }
    if (t < seg) dst[t] = (uint8_t)label;
}

__global__ __launch_bounds__(256) void cross_confusion_pairs_kernel(const uint8_t* __restrict__ label_slots, int64_t label_stride, int capacity,
                                                                    const int32_t* __restrict__ pairs, int64_t n, ClassTable ct, int K,
                                                                    unsigned long long* __restrict__ conf) {
    __shared__ int s_conf[kMaxK * kMaxK];
    const int p = blockIdx.z;
    const int sa = pairs[2 * p], sb = pairs[2 * p + 1];
    if (sa < 0 || sa >= capacity || sb < 0 || sb >= capacity) return;         // (the same for every thread of the block)
    cross_conf_block(label_slots + (int64_t)sa * label_stride, label_slots + (int64_t)sb * label_stride, n, ct, K, conf + (int64_t)p * K * K, s_conf);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The descriptor check on the host, over samples_host: the table the caller uploaded to samples_dev, checked before anything is launched.
// entry names the C entry in the messages.
static int check_replay_slot(const char* entry, int b, const ams_replay_sample& d, int capacity) {
    AMS_REQUIRE(d.slot >= 0 && d.slot < capacity, "%s: sample %d draws slot %d of %d", entry, b, d.slot, capacity);
    return AMS_OK;
}

static int check_replay_samples(const char* entry, const ams_replay_sample* samples_host, int B, int capacity, int H, int W) {
    for (int b = 0; b < B; ++b) {
        const ams_replay_sample& d = samples_host[b];
        RUN_RC(check_replay_slot(entry, b, d, capacity));
        AMS_REQUIRE(d.th > 0 && d.tw > 0 && d.th - H >= 0 && d.tw - W >= 0, "%s: sample %d: a %dx%d crop of a %dx%d image (negative slack)", entry, b, H, W,
                    d.th, d.tw);
        AMS_REQUIRE(d.top >= 0 && d.left >= 0 && d.top <= d.th - H && d.left <= d.tw - W, "%s: sample %d: crop origin (%d, %d) outside %dx%d", entry, b,
                    d.top, d.left, d.th, d.tw);
    }
    return AMS_OK;
}

int launch_replay_gather(const uint8_t* frame_slots, int64_t frame_stride, const uint8_t* label_slots, int64_t label_stride, int capacity, int Hs,
                         int Ws, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int B, int H, int W,
                         uint8_t* frames_out, uint8_t* labels_out, hipStream_t st) {
    AMS_REQUIRE(frame_slots && label_slots && samples_dev && samples_host && frames_out && labels_out, "replay_gather: null pointer");
    AMS_REQUIRE(capacity > 0 && Hs > 0 && Ws > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && H <= 65535, "replay_gather: bad geometry %dx%d -> %d x %dx%d, %d slots",
                Hs, Ws, B, H, W, capacity);
    AMS_REQUIRE(frame_stride >= (int64_t)Hs * Ws * 3 && label_stride >= (int64_t)Hs * Ws, "replay_gather: slot strides %lld / %lld below a %dx%d frame",
                (long long)frame_stride, (long long)label_stride, Hs, Ws);
    RUN_RC(check_replay_samples("replay_gather", samples_host, B, capacity, H, W));
    ReplayGeom g;
    g.capacity = capacity; g.Hs = Hs; g.Ws = Ws; g.H = H; g.W = W;
    g.frame_stride = frame_stride; g.label_stride = label_stride;
    g.vec = W % 16 == 0 && Ws % 16 == 0 && frame_stride % 16 == 0 && label_stride % 16 == 0 && aligned16(frame_slots) && aligned16(label_slots) &&
            aligned16(frames_out) && aligned16(labels_out);
    note_kernel("replay_gather_kernel");
    hipLaunchKernelGGL(replay_gather_kernel, dim3(cdiv(W, 256), H, B), dim3(256), 0, st, frame_slots, label_slots, samples_dev, g, frames_out,
                       labels_out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_replay_gather_rows(const float* slots, int64_t slot_stride, int capacity, int th, int tw, int C, const ams_replay_sample* samples_dev,
                              const ams_replay_sample* samples_host, int B, float* out, hipStream_t st) {
    AMS_REQUIRE(slots && samples_dev && samples_host && out, "replay_gather_f32: null pointer");
    AMS_REQUIRE(capacity > 0 && th > 0 && tw > 0 && C > 0 && B > 0 && B <= 65535, "replay_gather_f32: bad geometry %d x %dx%dx%d, %d slots", B, th, tw, C, capacity);
    const int64_t n = (int64_t)th * tw * C;
    AMS_REQUIRE(slot_stride >= n, "replay_gather_f32: slot stride %lld below %lld elements", (long long)slot_stride, (long long)n);
    for (int b = 0; b < B; ++b) {
        const ams_replay_sample& d = samples_host[b];
        RUN_RC(check_replay_slot("replay_gather_f32", b, d, capacity));
        // soft targets follow frames that are taken as they are: no rescale / crop / flip of teacher logits is defined
        AMS_REQUIRE(d.top == 0 && d.left == 0 && d.flip == 0, "replay_gather_f32: sample %d is cropped or flipped (%d, %d, %d)", b, d.top, d.left, d.flip);
    }
    const int vec = n % 4 == 0 && slot_stride % 4 == 0 && aligned16(slots) && aligned16(out) ? 1 : 0;
    int64_t gx = cdiv64(vec ? n / 4 : n, 256 * 4);
    gx = gx < 1 ? 1 : gx > 1024 ? 1024 : gx;
    note_kernel("replay_gather_rows_kernel");
    hipLaunchKernelGGL(replay_gather_rows_kernel, dim3((int)gx, 1, B), dim3(256), 0, st, slots, slot_stride, capacity, samples_dev, n, vec, out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_replay_gather_logits(const float* slots, int64_t slot_stride, int capacity, int Hs, int Ws, int C, const ams_replay_sample* samples_dev,
                                const ams_replay_sample* samples_host, int B, int H, int W, float* out, hipStream_t st) {
    AMS_REQUIRE(slots && samples_dev && samples_host && out, "replay_gather_logits: null pointer");
    AMS_REQUIRE(capacity > 0 && Hs > 0 && Ws > 0 && C > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && H <= 65535 && (int64_t)Ws * C <= INT32_MAX &&
                    (int64_t)W * C <= INT32_MAX,
                "replay_gather_logits: bad geometry %dx%dx%d -> %d x %dx%d, %d slots", Hs, Ws, C, B, H, W, capacity);
    AMS_REQUIRE(slot_stride >= (int64_t)Hs * Ws * C, "replay_gather_logits: slot stride %lld below a %dx%dx%d slot", (long long)slot_stride, Hs, Ws, C);
    RUN_RC(check_replay_samples("replay_gather_logits", samples_host, B, capacity, H, W));
    LogitsGeom g;
    g.capacity = capacity; g.Hs = Hs; g.Ws = Ws; g.C = C; g.H = H; g.W = W;
    g.slot_stride = slot_stride;
    g.vec = ((int64_t)Ws * C) % 4 == 0 && ((int64_t)W * C) % 4 == 0 && slot_stride % 4 == 0 && aligned16(slots) && aligned16(out);
    note_kernel("replay_gather_logits_kernel");
    hipLaunchKernelGGL(replay_gather_logits_kernel, dim3(cdiv(W, kLogitsSeg), H, B), dim3(256), 0, st, slots, samples_dev, g, out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_replay_gather_logits_lowres(const float* slots, int64_t slot_stride, int capacity, int lh, int lw, int C, int Hs, int Ws,
                                       const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int B, int H, int W, float* out,
                                       hipStream_t st) {
    AMS_REQUIRE(slots && samples_dev && samples_host && out, "replay_gather_logits_lowres: null pointer");
    AMS_REQUIRE(capacity > 0 && Hs > 0 && Ws > 0 && C > 0 && H > 0 && W > 0 && B > 0 && B <= 65535 && H <= 65535 && (int64_t)Ws * C <= INT32_MAX &&
                    (int64_t)W * C <= INT32_MAX,
                "replay_gather_logits_lowres: bad geometry %dx%dx%d -> %d x %dx%d, %d slots", Hs, Ws, C, B, H, W, capacity);
    AMS_REQUIRE(lh >= 1 && lh <= Hs && lw >= 1 && lw <= Ws, "replay_gather_logits_lowres: a %dx%d cache for %dx%d frames (1 <= lh <= src_h, 1 <= lw <= src_w)", lh,
                lw, Hs, Ws);
    AMS_REQUIRE(slot_stride >= (int64_t)lh * lw * C, "replay_gather_logits_lowres: slot stride %lld below a %dx%dx%d slot", (long long)slot_stride, lh, lw, C);
    RUN_RC(check_replay_samples("replay_gather_logits_lowres", samples_host, B, capacity, H, W));
    LowresGeom g;
    g.capacity = capacity; g.lh = lh; g.lw = lw; g.C = C; g.Hs = Hs; g.Ws = Ws; g.H = H; g.W = W;
    g.slot_stride = slot_stride;
    g.sy = align_corners_scale(lh, Hs);                               // as soft_teacher_geom does for a teacher grid under Hs x Ws labels
    g.sx = align_corners_scale(lw, Ws);
    note_kernel("replay_gather_logits_lowres_kernel");
    hipLaunchKernelGGL(replay_gather_logits_lowres_kernel, dim3(cdiv(W, kLogitsSeg), H, B), dim3(256), 0, st, slots, samples_dev, g, out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_replay_pack_logits(const float* in, int th, int tw, int NC, const int32_t* idx_host, int K, float* out, hipStream_t st) {
    AMS_REQUIRE(in && out && idx_host, "replay_pack_logits: null pointer");
    AMS_REQUIRE(th > 0 && tw > 0 && th <= 65535 && NC > 0 && NC <= 256 && (int64_t)tw * NC <= INT32_MAX, "replay_pack_logits: bad geometry %dx%dx%d", th, tw, NC);
    AMS_REQUIRE(K >= 1 && K <= kMaxK, "replay_pack_logits: K=%d out of range (1..%d)", K, kMaxK);
    PackGeom g;
    for (int k = 0; k < kMaxK; ++k) g.idx[k] = 0;
    for (int k = 0; k < K; ++k) {
        AMS_REQUIRE(idx_host[k] >= 0 && idx_host[k] < NC, "replay_pack_logits: channel %d of %d", idx_host[k], NC);
        g.idx[k] = idx_host[k];
    }
    g.th = th; g.tw = tw; g.NC = NC; g.K = K;
    g.run = kPackFloats / NC < kPackRun ? (kPackFloats / NC) & ~3 : kPackRun;
    // a run is a multiple of 4 pixels: with a row pitch that is a multiple of 4 floats every run of every row starts and ends on 16 bytes
    g.vec_in = aligned16(in) && ((int64_t)tw * NC) % 4 == 0;
    g.vec_out = aligned16(out) && ((int64_t)tw * K) % 4 == 0;
    note_kernel("replay_pack_logits_kernel");
    hipLaunchKernelGGL(replay_pack_logits_kernel, dim3(cdiv(tw, g.run), th), dim3(256), 0, st, in, g, out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// src_tap's lo / hi on the host (one f32 product, as __fmul_rn gives it)
static inline void src_tap_host(int dst, float scale, int n_in, int& lo, int& hi) {
    const float src = (float)dst * scale;
    lo = (int)floorf(src);
    hi = lo + 1 < n_in ? lo + 1 : n_in - 1;
}

// the most cached columns a segment of seg pixels of a Ws-wide row touches
static int label_segment_columns(int Ws, int lw, float sx, int seg) {
    int most = 1;
    for (int x_first = 0; x_first < Ws; x_first += seg) {
        const int x_last = x_first + seg < Ws ? x_first + seg - 1 : Ws - 1;
        int lo, hi, unused;
        src_tap_host(x_first, sx, lw, lo, unused);
        src_tap_host(x_last, sx, lw, unused, hi);
        if (hi - lo + 1 > most) most = hi - lo + 1;
    }
    return most;
}

int launch_teacher_labels_from_logits(const float* logits, int64_t slot_stride, int n, int lh, int lw, int NC, int Hs, int Ws, uint8_t* out,
                                      int64_t out_stride, hipStream_t st) {
    AMS_REQUIRE(logits && out, "teacher_labels_from_logits: null pointer");
    AMS_REQUIRE(n >= 1 && n <= 65535, "teacher_labels_from_logits: n=%d out of range (1..65535)", n);
    AMS_REQUIRE(Hs >= 1 && Ws >= 1 && Hs <= 65535, "teacher_labels_from_logits: bad label size %dx%d", Hs, Ws);
    AMS_REQUIRE(lh >= 1 && lh <= Hs && lw >= 1 && lw <= Ws, "teacher_labels_from_logits: %dx%d logits for %dx%d labels (1 <= lh <= Hs, 1 <= lw <= Ws)", lh, lw, Hs,
                Ws);
    AMS_REQUIRE(NC >= 1 && NC <= 255, "teacher_labels_from_logits: num_classes=%d out of range (1..255: id 255 stays \"unlabelled\")", NC);
    AMS_REQUIRE(slot_stride >= (int64_t)lh * lw * NC, "teacher_labels_from_logits: slot stride %lld below a %dx%dx%d item", (long long)slot_stride, lh, lw, NC);
    AMS_REQUIRE(out_stride >= (int64_t)Hs * Ws, "teacher_labels_from_logits: output stride %lld below a %dx%d label map", (long long)out_stride, Hs, Ws);
    LabelGeom g;
    g.n = n; g.lh = lh; g.lw = lw; g.NC = NC; g.Hs = Hs; g.Ws = Ws;
    g.slot_stride = slot_stride; g.out_stride = out_stride;
    g.sy = align_corners_scale(lh, Hs);                               // as soft_teacher_geom does for a teacher grid under Hs x Ws labels
    g.sx = align_corners_scale(lw, Ws);
    // the widest segment whose cached columns (two rows of them, every class) fit: 128 pixels unless the classes are many and the grid dense
    const int ld = NC | 1;
    int seg = kLabelSeg, cols = label_segment_columns(Ws, lw, g.sx, seg);
    while (seg > 4 && (int64_t)2 * cols * ld * (int64_t)sizeof(float) > kLabelLdsBytes) {
        seg >>= 1;
        cols = label_segment_columns(Ws, lw, g.sx, seg);
    }
    g.seg = seg;
    g.lds_floats = 2 * cols * ld;                                      // (seg = 4, NC = 255: 5 columns, 10 KB)
    g.vec = Ws % 4 == 0 && out_stride % 4 == 0 && ((uintptr_t)out & 3) == 0;
    note_kernel("teacher_labels_kernel");
    hipLaunchKernelGGL(teacher_labels_kernel, dim3(cdiv(Ws, seg), Hs, n), dim3(kLabelSeg), sizeof(float) * g.lds_floats, st, logits, g, out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

// lut: HOST pointer, 256 entries (teacher id -> subset index or -1); conf [n_pairs][K][K] overwritten
int launch_cross_confusion_pairs(const uint8_t* label_slots, int64_t label_stride, int capacity, int64_t n, const int32_t* pairs_dev,
                                 const int32_t* pairs_host, int n_pairs, const int32_t* lut, int K, int64_t* conf, hipStream_t st) {
    AMS_REQUIRE(label_slots && pairs_dev && pairs_host && conf, "cross_confusion_pairs: null pointer");
    AMS_REQUIRE(K > 0 && K <= kMaxK, "cross_confusion_pairs: K=%d out of range", K);
    AMS_REQUIRE(capacity > 0 && n > 0 && label_stride >= n && n_pairs > 0 && n_pairs <= 65535, "cross_confusion_pairs: bad geometry (%d pairs, %d slots)", n_pairs,
                capacity);
    for (int p = 0; p < 2 * n_pairs; ++p)
        AMS_REQUIRE(pairs_host[p] >= 0 && pairs_host[p] < capacity, "cross_confusion_pairs: pair %d names slot %d of %d", p / 2, pairs_host[p], capacity);
    ClassTable ct;
    for (int i = 0; i < 256; ++i) ct.lut[i] = lut[i];
    for (int k = 0; k < kMaxK; ++k) ct.idx[k] = 0;
    AMS_CHECK_HIP(hipMemsetAsync(conf, 0, sizeof(int64_t) * K * K * n_pairs, st));
    int grid = (int)cdiv64(n, 256 * 16);
    grid = grid < 1 ? 1 : grid > 2048 ? 2048 : grid;
    note_kernel("cross_confusion_pairs_kernel");
    hipLaunchKernelGGL(cross_confusion_pairs_kernel, dim3(grid, 1, n_pairs), dim3(256), 0, st, label_slots, label_stride, capacity, pairs_dev, n, ct, K,
                       (unsigned long long*)conf);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
