// The frozen head as ONE kernel (AMS_OPT_FUSE_HEAD): aspp0 (K -> 256) -> concat_projection (256 -> 256, + per-image bias) -> logits
// (256 -> <= 32 columns), every product on two fp16 parts as pw_gemm_f16x3_l forms it (k_pw_f16.hip, split_bf16.hpp).
//
// A row of the head depends on the same row of its input and on one per-image bias, so a wave keeps its 16 rows through all three layers:
//   prologue the wave's 16 x K f32 operand tile (one contiguous piece of memory) is requested at once with full-line loads, split
//            (split8_f16) and written as fp16 pairs into a wave-private LDS slab.  A block is one wave per SIMD: a register ring one stage
//            deep cannot cover the latency of an operand that comes from HBM / the Infinity Cache (measured: 3.6 k cycles per stage with
//            it), so that latency is paid once per block instead of once per stage;
//   stage A  operand fragments from the slab; 16 column tiles x (hi hi | cross terms) = 128 accumulator registers; epilogue (join, folded
//            BN, ReLU) as pw_epilogue_t writes it, then the activated tile is split again and written back into the slab, laid out the
//            way the next layer's operand fragments are read;
//   stage B  operand fragments from the slab, the same 128 accumulators; epilogue: + img_bias[row / rows_per_img] (per row: a 16-row tile
//            may straddle two images), BN, ReLU, split, back into the slab;
//   stage C  the whole logits panel is ONE weight stage (<= 32 columns x 256 k x 2 parts = 32 KB), two column tiles, result [rows][32] f32.
// The 256-wide f32 tensors between the three GEMMs (2 x 4 M N bytes written and read back) never exist.
//
// Per output element the k order (32 k per MFMA, stages ascending), the split, the order of the three MFMAs of a stage (wl xh, wh xl into
// the cross accumulator, wh xh into the main one), their join and the epilogue expressions are those of the three launches: same bits.
//
// Weight stages (32 k x 256 columns x 2 parts = 32 KB) are shared by the block's four waves, double-buffered in the XOR-swizzled 64-byte
// rows of pw_gemm_f16x3_l; one block barrier per stage.  The slab needs no block barrier: only its own wave reads it.
// LDS: 64 KB of weight stages + 4 slabs of 16 x (4 K + 16) bytes (20.25 KB at K = 320) + 4.1 KB of vectors: one block (four waves, one
// per SIMD) per CU.  Five waves would put two on one SIMD, and a wave's 48 MFMAs per stage (768 cycles) already outweigh the block's
// fragment reads (128 KB at 256 B/clk).
#include "pw_common.hpp"
#include "split_bf16.hpp"
#include "block_call.hpp"

namespace ams {

namespace {

constexpr int HC_N = 256;                            // width of aspp0's and concat_projection's results
constexpr int HC_NT = HC_N / 16;                     // column tiles of stages A and B
constexpr int HC_NW = 4, HC_NTH = 64 * HC_NW;
constexpr int HC_STAGE_HALVES = 2 * HC_N * 32;       // one weight stage: [part][256 n][32 k] fp16
constexpr int HC_KA_MAX = 352;                       // widest aspp0 input whose slabs fit beside the weight stages
// bytes per slab row: K (hi, lo) pairs + 16, so that rows lie 4 banks apart; K = max(aspp0's input, 256)
static inline int hc_slab_pitch(int KA) { return (KA > HC_N ? KA : HC_N) * 4 + 16; }
constexpr int HC_VEC_FLOATS = 4 * HC_N + 32;         // scale | shift of A, scale | shift of B, bias of C
static inline size_t hc_lds(int KA) { return (size_t)2 * HC_STAGE_HALVES * 2 + (size_t)HC_NW * 16 * hc_slab_pitch(KA) + (size_t)HC_VEC_FLOATS * 4; }

struct HeadChainArgs {
    const float* x; int64_t M; int KA;               // [M][KA] f32 (dense rows), KA % 32 == 0
    int pitch;                                       // hc_slab_pitch(KA)
    const unsigned short *wA, *wB, *wC;              // fp16 panels [part][N][Kp]: Kp = KA | 256 | 256
    int64_t planeA, planeB, planeC;
    const float *scA, *shA, *scB, *shB, *biasC;      // folded BN of A and B (256 each); the logits' biases (NC)
    const float* img_bias; int64_t rows_per_img;     // [M / rows_per_img][256]
    int actA, actB, actC, NC;                        // NC <= 32 logits columns
    float* y;                                        // [M][32]
};

__device__ __forceinline__ f32x4 hc_mma(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// one 32-k stage of a 256-column layer: bw = this lane's fragment of column tile 0, part hi, in the current weight stage.
// Four column tiles at a time, the next four's fragments (8 ds_read_b128) requested before this four's 12 MFMAs: a block is one wave per
// SIMD, so nothing else hides the LDS latency — left to itself the compiler keeps ONE read in flight (two fragment registers, a wait after
// every read: 4 k cycles a stage instead of < 1 k).  The scheduling barriers pin that order, and with it the stage's global loads (the
// weights of the next stage; the operand comes from the slab), which are issued before the first of them.
constexpr int HC_G = 4;
__device__ __forceinline__ void hc_load_frags(const unsigned short* bw, int t0, u32x4 (&qh)[HC_G], u32x4 (&ql)[HC_G]) {
#pragma unroll
    for (int g = 0; g < HC_G; ++g) {
        qh[g] = *reinterpret_cast<const u32x4*>(bw + (t0 + g) * 16 * 32);
        ql[g] = *reinterpret_cast<const u32x4*>(bw + HC_N * 32 + (t0 + g) * 16 * 32);
    }
}
__device__ __forceinline__ void hc_stage_tiles(const unsigned short* bw, const u32x4& xh, const u32x4& xl, f32x4 (&acc)[HC_NT], f32x4 (&accx)[HC_NT]) {
    u32x4 qh[2][HC_G], ql[2][HC_G];
    hc_load_frags(bw, 0, qh[0], ql[0]);
#pragma unroll
    for (int grp = 0; grp < HC_NT / HC_G; ++grp) {
        const int cur = grp & 1, t0 = grp * HC_G;
        if (grp + 1 < HC_NT / HC_G) hc_load_frags(bw, t0 + HC_G, qh[cur ^ 1], ql[cur ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
        // fixed order per accumulator pair: cross terms (wl xh, then wh xl), then the main term
#pragma unroll
        for (int g = 0; g < HC_G; ++g) accx[t0 + g] = hc_mma(ql[cur][g], xh, accx[t0 + g]);
#pragma unroll
        for (int g = 0; g < HC_G; ++g) accx[t0 + g] = hc_mma(qh[cur][g], xl, accx[t0 + g]);
#pragma unroll
        for (int g = 0; g < HC_G; ++g) acc[t0 + g] = hc_mma(qh[cur][g], xh, acc[t0 + g]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// join, (+ per-row bias), BN, activation, split; the tile goes into the wave's slab as the next layer's operand:
// logical group g = 4 s + q of 8 channels (the 8 k of lane quarter q in stage s) lies at position 8 q + s of the row — 32 bytes, hi then
// lo — so the four quarters of a fragment read hit the same banks and rows 16 bytes apart never collide (pitch + 16)
template <bool BIAS>
__device__ __forceinline__ void hc_handover(f32x4 (&acc)[HC_NT], f32x4 (&accx)[HC_NT], const float* sSc, const float* sSh, int act, const float* bias_row,
                                            unsigned char* slab, int pitch, int l15, int q) {
    float4 bv[BIAS ? HC_NT : 1];
    if constexpr (BIAS) {
#pragma unroll
        for (int t = 0; t < HC_NT; ++t) bv[t] = ld4(bias_row + 16 * t + 4 * q);
    }
#pragma unroll
    for (int t = 0; t < HC_NT; ++t) {
        const f32x4 j = combine_f16(acc[t], accx[t]);
        float4 v = make_float4(j[0], j[1], j[2], j[3]);
        if constexpr (BIAS) { v.x += bv[t].x; v.y += bv[t].y; v.z += bv[t].z; v.w += bv[t].w; }      // before scale / shift, as EPI_BIAS
        const int c4 = 16 * t + 4 * q;
        const float4 bn = muladd4_pk(v, ld4(sSc + c4), ld4(sSh + c4));                                  // packed, two roundings
        v = make_float4(apply_act(bn.x, act), apply_act(bn.y, act), apply_act(bn.z, act), apply_act(bn.w, act));
        unsigned h[2], l[2];
        split4_f16(v, h, l);
        const int g = 2 * t + (q >> 1), pos = (g & 3) * 8 + (g >> 2);
        unsigned char* p = slab + l15 * pitch + pos * 32 + (q & 1) * 8;
        *reinterpret_cast<uint2*>(p) = make_uint2(h[0], h[1]);
        *reinterpret_cast<uint2*>(p + 16) = make_uint2(l[0], l[1]);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(HC_NTH, 1) void head_chain_kernel(HeadChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned short* sW = reinterpret_cast<unsigned short*>(smem);                         // [2][HC_STAGE_HALVES]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, q = lane >> 4;
    const int pitch = a.pitch;
    unsigned char* slab = smem + (size_t)2 * HC_STAGE_HALVES * 2 + wave * (16 * pitch);
    float* sVec = reinterpret_cast<float*>(smem + (size_t)2 * HC_STAGE_HALVES * 2 + HC_NW * (16 * pitch));
    const int nA = a.KA / 32, nB = HC_N / 32;                                             // weight stages: A's, B's, then the logits panel

    // ---- weight stages: 2048 16-byte pieces, 8 per thread -------------------------------------------------------------------------------
    // A, B: piece e = tid + 256 u -> part u / 4, column tid / 4 + 64 (u % 4), 8 k at (tid % 4) * 8
    const int wn = tid >> 2, wp = tid & 3;
    const int dstAB = wn * 32 + (wp ^ (((wn >> 3) & 1) << 1)) * 8;
    // C: piece -> k stage u, part tid / 128, column (tid % 128) / 4 (clamped to the last real column: the tiles' surplus columns are never stored)
    const int cpart = tid >> 7, cn = (tid & 127) >> 2;
    const int dstC = cpart * (32 * 32) + cn * 32 + (wp ^ (((cn >> 3) & 1) << 1)) * 8;
    const unsigned short* srcA = a.wA + (int64_t)wn * a.KA + wp * 8;
    const unsigned short* srcB = a.wB + (int64_t)wn * HC_N + wp * 8;
    const unsigned short* srcC = a.wC + cpart * a.planeC + (int64_t)(cn < a.NC ? cn : a.NC - 1) * HC_N + wp * 8;
    u32x4 wreg[8];
    auto load_w = [&](int g) {                       // block-uniform
        if (g < nA + nB) {
            const bool isA = g < nA;
            const unsigned short* src = isA ? srcA + g * 32 : srcB + (g - nA) * 32;
            const int64_t plane = isA ? a.planeA : a.planeB, col64 = isA ? (int64_t)64 * a.KA : (int64_t)64 * HC_N;
#pragma unroll
            for (int u = 0; u < 8; ++u) wreg[u] = *reinterpret_cast<const u32x4*>(src + (u >> 2) * plane + (u & 3) * col64);
        } else if (g == nA + nB) {
#pragma unroll
            for (int u = 0; u < 8; ++u) wreg[u] = *reinterpret_cast<const u32x4*>(srcC + u * 32);
        }
    };
    auto store_w = [&](int g) {
        unsigned short* base = sW + (g & 1) * HC_STAGE_HALVES;
        if (g < nA + nB) {
#pragma unroll
            for (int u = 0; u < 8; ++u) *reinterpret_cast<u32x4*>(base + (u >> 2) * (HC_N * 32) + (u & 3) * (64 * 32) + dstAB) = wreg[u];
        } else if (g == nA + nB) {
#pragma unroll
            for (int u = 0; u < 8; ++u) *reinterpret_cast<u32x4*>(base + u * (2 * 32 * 32) + dstC) = wreg[u];
        }
    };

    const int64_t m0 = (int64_t)blockIdx.x * (16 * HC_NW) + wave * 16, m_lane = m0 + l15;
    const int64_t m_ld = m_lane < a.M ? m_lane : a.M - 1;
    load_w(0);
    // ---- prologue: the wave's operand tile -> slab, group (8 k) 4 s + q of a row at byte 32 (4 s + q): hi, then lo.  Lane -> group
    // lane + 64 it of the tile: 32 contiguous bytes per lane, 2 KB per request, five requests in flight
    for (int it0 = 0; it0 < nA; it0 += 5) {
        float4 u[5][2];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const int it = it0 + i < nA ? it0 + i : nA - 1;
            const int gi = it * 64 + lane, row = gi / (4 * nA), grp = gi - row * (4 * nA);
            const int64_t m = m0 + row < a.M ? m0 + row : a.M - 1;
            const float* p = a.x + m * a.KA + grp * 8;
            u[i][0] = ld4(p); u[i][1] = ld4(p + 4);
        }
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            if (it0 + i < nA) {
                const int gi = (it0 + i) * 64 + lane, row = gi / (4 * nA), grp = gi - row * (4 * nA);
                f16x8 h, l;
                split8_f16(u[i][0], u[i][1], h, l);
                unsigned char* p = slab + row * pitch + grp * 32;
                *reinterpret_cast<u32x4*>(p) = __builtin_bit_cast(u32x4, h);
                *reinterpret_cast<u32x4*>(p + 16) = __builtin_bit_cast(u32x4, l);
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int e = tid; e < HC_VEC_FLOATS; e += HC_NTH) {
        const int which = e >> 8, c = e & 255;
        float v;
        if (which == 0) v = a.scA ? a.scA[c] : 1.f;
        else if (which == 1) v = a.shA ? a.shA[c] : 0.f;
        else if (which == 2) v = a.scB ? a.scB[c] : 1.f;
        else if (which == 3) v = a.shB ? a.shB[c] : 0.f;
        else v = (a.biasC && c < a.NC) ? a.biasC[c] : 0.f;
        sVec[e] = v;
    }
    f32x4 acc[HC_NT], accx[HC_NT];
#pragma unroll
    for (int t = 0; t < HC_NT; ++t) { acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; accx[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    store_w(0);
    __syncthreads();

    const int frag = l15 * 32 + 8 * (q ^ ((l15 >> 3) << 1));                              // this lane's fragment inside a 16-column tile
    // ---- stage A ------------------------------------------------------------------------------------------------------------------------
    {
        const unsigned char* xa = slab + l15 * pitch + q * 32;                             // + 128 s: stage s
        u32x4 xh = *reinterpret_cast<const u32x4*>(xa), xl = *reinterpret_cast<const u32x4*>(xa + 16);
        for (int s = 0; s < nA; ++s) {
            const int sn = s + 1 < nA ? s + 1 : s;
            load_w(s + 1);
            const u32x4 xh1 = *reinterpret_cast<const u32x4*>(xa + sn * 128), xl1 = *reinterpret_cast<const u32x4*>(xa + sn * 128 + 16);
            hc_stage_tiles(sW + (s & 1) * HC_STAGE_HALVES + frag, xh, xl, acc, accx);
            xh = xh1; xl = xl1;
            store_w(s + 1);
            __syncthreads();
        }
    }
    hc_handover<false>(acc, accx, sVec, sVec + HC_N, a.actA, nullptr, slab, pitch, l15, q);

    // ---- stage B ------------------------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int t = 0; t < HC_NT; ++t) { acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; accx[t] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    const unsigned char* xfrag = slab + l15 * pitch + q * 8 * 32;                 // + 32 s: stage s
    u32x4 xh = *reinterpret_cast<const u32x4*>(xfrag), xl = *reinterpret_cast<const u32x4*>(xfrag + 16);
    for (int s = 0; s < nB; ++s) {
        const int g = nA + s, sn = s + 1 < nB ? s + 1 : s;
        load_w(g + 1);
        const u32x4 xh1 = *reinterpret_cast<const u32x4*>(xfrag + sn * 32), xl1 = *reinterpret_cast<const u32x4*>(xfrag + sn * 32 + 16);
        hc_stage_tiles(sW + (g & 1) * HC_STAGE_HALVES + frag, xh, xl, acc, accx);
        xh = xh1; xl = xl1;
        store_w(g + 1);
        __syncthreads();
    }
    hc_handover<true>(acc, accx, sVec + 2 * HC_N, sVec + 3 * HC_N, a.actB, a.img_bias + (m_ld / a.rows_per_img) * HC_N, slab, pitch, l15, q);

    // ---- stage C: the panel is one weight stage, [k stage][part][32 n][32 k] -------------------------------------------------------------
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0, cx0 = c0, cx1 = c0;
    const unsigned short* cw = sW + ((nA + nB) & 1) * HC_STAGE_HALVES + frag;
    // two k stages at a time, the next two's fragments (12 reads) requested before this two's 12 MFMAs
    constexpr int CS = 2, NCG = HC_N / 32 / CS;
    u32x4 fx[2][CS][2], fw[2][CS][4];          // [buffer][k stage]: (xh, xl) | (hi 0, hi 1, lo 0, lo 1)
    auto load_c = [&](int grp, u32x4 (&x)[CS][2], u32x4 (&w)[CS][4]) {
#pragma unroll
        for (int i = 0; i < CS; ++i) {
            const int s = grp * CS + i;
            const unsigned short* bw = cw + s * (2 * 32 * 32);
            x[i][0] = *reinterpret_cast<const u32x4*>(xfrag + s * 32); x[i][1] = *reinterpret_cast<const u32x4*>(xfrag + s * 32 + 16);
            w[i][0] = *reinterpret_cast<const u32x4*>(bw); w[i][1] = *reinterpret_cast<const u32x4*>(bw + 16 * 32);
            w[i][2] = *reinterpret_cast<const u32x4*>(bw + 32 * 32); w[i][3] = *reinterpret_cast<const u32x4*>(bw + 32 * 32 + 16 * 32);
        }
    };
    load_c(0, fx[0], fw[0]);
#pragma unroll
    for (int grp = 0; grp < NCG; ++grp) {
        const int cur = grp & 1;
        if (grp + 1 < NCG) load_c(grp + 1, fx[cur ^ 1], fw[cur ^ 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < CS; ++i) {         // k stages ascending; per accumulator pair: wl xh, wh xl, then wh xh
            cx0 = hc_mma(fw[cur][i][2], fx[cur][i][0], cx0); cx1 = hc_mma(fw[cur][i][3], fx[cur][i][0], cx1);
            cx0 = hc_mma(fw[cur][i][0], fx[cur][i][1], cx0); cx1 = hc_mma(fw[cur][i][1], fx[cur][i][1], cx1);
            c0 = hc_mma(fw[cur][i][0], fx[cur][i][0], c0); c1 = hc_mma(fw[cur][i][1], fx[cur][i][0], c1);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (m_lane < a.M) {
        const float4 one = make_float4(1.f, 1.f, 1.f, 1.f);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const f32x4 j = combine_f16(t == 0 ? c0 : c1, t == 0 ? cx0 : cx1);
            const int n4 = 16 * t + 4 * q;
            const float4 bn = muladd4_pk(make_float4(j[0], j[1], j[2], j[3]), one, ld4(sVec + 4 * HC_N + n4));
            const float o[4] = {apply_act(bn.x, a.actC), apply_act(bn.y, a.actC), apply_act(bn.z, a.actC), apply_act(bn.w, a.actC)};
            float* yp = a.y + m_lane * 32 + n4;
            if (n4 + 3 < a.NC) st4(yp, make_float4(o[0], o[1], o[2], o[3]));
            else {
#pragma unroll
                for (int i = 0; i < 4; ++i) if (n4 + i < a.NC) yp[i] = o[i];
            }
        }
    }
}

}  // namespace

// the three head layers have the shapes the chained kernel is built for
bool head_chain_supported(int KA, int NA, int KB, int NB, int KC, int NC) {
    return KA >= 32 && KA % 32 == 0 && KA <= HC_KA_MAX && NA == HC_N && KB == HC_N && NB == HC_N && KC == HC_N && NC >= 1 && NC <= 32;
}

// logits[M][32] = C(B(A(x))) with A = aspp0, B = concat_projection (+ img_bias per image), C = logits; panels as launch_pointwise_split_f16 takes them
int launch_head_chain(const float* x, int64_t M, int KA, const ConvLayer& A, const ConvLayer& B, const ConvLayer& C, const float* img_bias,
                      int64_t rows_per_img, int NC, float* y, hipStream_t st) {
    AMS_REQUIRE(M > 0 && rows_per_img > 0 && x && A.panels && B.panels && C.panels && img_bias && y && head_chain_supported(KA, HC_N, HC_N, HC_N, HC_N, NC),
                "head_chain: bad problem (M %lld KA %d NC %d)", (long long)M, KA, NC);
    HeadChainArgs a;
    a.x = x; a.M = M; a.KA = KA; a.pitch = hc_slab_pitch(KA);
    const size_t lds = hc_lds(KA);
    a.wA = A.panels; a.wB = B.panels; a.wC = C.panels; a.planeA = A.plane; a.planeB = B.plane; a.planeC = C.plane;
    a.scA = A.scale; a.shA = A.shift; a.scB = B.scale; a.shB = B.shift; a.biasC = C.shift;
    a.img_bias = img_bias; a.rows_per_img = rows_per_img;
    a.actA = A.act; a.actB = B.act; a.actC = C.act; a.NC = NC;
    a.y = y;
    RUN_RC(func_allow_lds((const void*)head_chain_kernel, lds));
    note_kernel("head_chain_kernel");
    hipLaunchKernelGGL(head_chain_kernel, dim3((unsigned)cdiv64(M, 16 * HC_NW)), dim3(HC_NTH), lds, st, a);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
