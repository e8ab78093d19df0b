// One frozen inverted-residual block as the host describes it to the block launchers (k_block, k_first_block, k_expand_dw, k_xdw_stream, k_xdw_wreg,
// k_dw_project; k_head_chain takes three layers), and the one check those launchers and their ams_k_* entries go through first.  Host code only.
#pragma once
#include "kernels.hpp"

namespace ams {

// A conv layer as a frozen kernel reads it: f32 weights, folded BN, activation; optionally its part panels [part][cout][Kp], part p at
// panels + p * plane: np = 1 .. 3 bf16 parts or AMS_NP_F16 (two fp16 parts, hi | lo 2^11); np = 0: the layer runs on w
struct ConvLayer {
    const float *w = nullptr, *scale = nullptr, *shift = nullptr;
    int act = AMS_ACT_NONE;
    const uint16_t* panels = nullptr; int64_t plane = 0; int np = 0, Kp = 0;
};

// The call: [expand ->] depthwise -> [project (+ block input)] on one input.  Each launcher reads the part it needs.
struct BlockCall {
    const float* x = nullptr;                  // f32 [B][H][W][Cin] (dw_project: the expanded tensor [B][H][W][Cexp]), or, first block,
    const void* frames = nullptr; int dtype = AMS_DT_F32; float pixel_scale = 0.f;      // frames [B][H][W][3], AMS_DT_U8 | AMS_DT_F32, normalised as v * pixel_scale - 1
    const uint16_t* x_parts = nullptr; int64_t x_plane = 0;      // optional (streaming forms): x as part planes [part][B*H*W][Cin], x_plane apart, in expand.np's format
    int B = 0, H = 0, W = 0, Cin = 0;
    ConvLayer expand, dw, project;             // expand: the stem in the first block
    int Cexp = 0, stride = 1, rate = 1, Cout = 0;
    bool residual = false; const float* res = nullptr;      // the project layer adds the block input: x itself, or `res` where x is the expanded tensor (dw_project)
    float* y = nullptr; int y_fmt = 0;         // y_fmt 1 (fp16 streaming forms): fp16 pairs interleaved per 8 channels (PwArgs::x_fmt 1) instead of f32
    const float* vecs = nullptr;               // optional [13][Cexp] table of launch_block_pack (tile-per-wave kernels)
};

// What an ams_k_* entry adds: the scratch into which it splits the panels itself, the product form it was asked for by number, and its own
// narrowing of the launcher's shape rule
struct EntryScratch { const uint16_t* panels = nullptr; size_t elems = 0, need = 0; int form = 0, n_forms = 1; bool shape_ok = true; };

enum BlockKernel { BK_WHOLE, BK_FIRST, BK_FIRST_TILES, BK_FIRST_PLAN /* the plan query: no tensors */, BK_TILED, BK_STREAM, BK_WREG, BK_DW_PROJECT };

// Refused in this order: the frame dtype (first block); no pixels; an unknown form, kernel k's shape rule or parts out of range; the scratch too
// small or panels missing; the output format; a null pointer among what kernel k reads.  The launcher's own conditions (LDS geometry, grid) follow.
static inline int block_call_check(const char* who, BlockKernel k, const BlockCall& c, const EntryScratch* e = nullptr) {
    const ConvLayer &ex = c.expand, &pj = c.project;
    AMS_REQUIRE(k < BK_FIRST || k > BK_FIRST_PLAN || c.dtype == AMS_DT_U8 || c.dtype == AMS_DT_F32, "%s: frames must be uint8 or float32", who);
    AMS_REQUIRE(c.B > 0 && c.H > 0 && c.W > 0, "%s: no pixels: B=%d, %d x %d", who, c.B, c.H, c.W);
    AMS_REQUIRE(!e || (e->form >= 0 && e->form < e->n_forms), "%s: unknown form %d", who, e ? e->form : 0);
    const auto reads = [](const ConvLayer& l) { return l.w && l.scale && l.shift; };
    const bool f32 = c.Cin <= 32;              // streaming: the exact-f32 form, no panels
    const bool np_ok = (ex.np >= 1 && ex.np <= 3) || ex.np == AMS_NP_F16;
    // tile-per-block forms: exact f32 | expand on three bf16 parts | expand and project on two fp16 parts
    const bool pair_ok = (ex.np == 0 || ex.np == 3 || ex.np == AMS_NP_F16) && pj.np == (ex.np == AMS_NP_F16 ? AMS_NP_F16 : 0);
    const bool pair_panels = (!ex.np || ex.panels) && (!pj.np || pj.panels);
    bool shape = true, panels = true, ptrs = c.y && reads(c.dw);
    switch (k) {
        case BK_WHOLE:
            shape = block_fused_supported(c.Cin, c.Cexp, c.Cout, c.stride, c.rate, c.residual) && pair_ok;
            panels = pair_panels; ptrs = ptrs && c.x && reads(ex) && reads(pj);
            break;
        case BK_FIRST: case BK_FIRST_TILES:
            shape = c.Cin == 3 && c.Cexp == 32 && c.Cout == 16 && c.stride == 1 && c.rate == 1 && !c.residual && pair_ok && (k == BK_FIRST || ex.np == 0);
            panels = pair_panels; ptrs = ptrs && c.frames && reads(ex) && reads(pj);
            break;
        case BK_FIRST_PLAN: ptrs = true; break;
        case BK_TILED: shape = expand_dw_supported(c.Cin, c.Cexp, c.stride, c.rate); ptrs = ptrs && c.x && reads(ex); break;
        case BK_STREAM:
            shape = expand_dw_stream_supported(c.Cin, c.Cexp, c.stride, c.rate) && (f32 || np_ok);
            panels = f32 || ex.panels; ptrs = ptrs && c.x && reads(ex);
            break;
        case BK_WREG:
            shape = expand_dw_stream_supported(c.Cin, c.Cexp, 1, c.rate) && c.stride == 1 && c.Cin >= 64 && np_ok;
            panels = ex.panels != nullptr; ptrs = ptrs && c.x_parts && reads(ex);
            break;
        case BK_DW_PROJECT:
            shape = dw_project_supported(c.Cexp, c.Cout, c.stride, c.rate) && pj.np == 2 && pj.Kp == c.Cexp;
            panels = pj.panels != nullptr; ptrs = ptrs && c.x && reads(pj) && (!c.residual || c.res);
            break;
    }
    AMS_REQUIRE(shape && (!e || e->shape_ok), "%s: unsupported shape Cin=%d Cexp=%d Cout=%d stride=%d rate=%d parts=%d|%d", who, c.Cin, c.Cexp, c.Cout,
                c.stride, c.rate, ex.np, pj.np);
    AMS_REQUIRE(!e || e->need == 0 || (e->panels && e->elems >= e->need), "%s: panel scratch too small (need %zu)", who, e ? e->need : (size_t)0);
    AMS_REQUIRE(panels, "%s: panels missing", who);
    AMS_REQUIRE(c.y_fmt == 0 || (c.y_fmt == 1 && (k == BK_STREAM || k == BK_WREG) && !f32 && ex.np == AMS_NP_F16 && c.Cexp % 8 == 0 && c.stride == 1),
                "%s: the fp16-pair output needs the fp16 form and Cexp %% 8 == 0", who);
    AMS_REQUIRE(ptrs, "%s: null pointer", who);
    return AMS_OK;
}

}  // namespace ams
