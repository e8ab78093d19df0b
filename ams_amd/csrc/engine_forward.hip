// The student engine, part 2 of 4: frozen inference (BN folded; what the edge device runs), its multi-stream plans, and the live
// forward with training-mode BN (reference SemanticNetwork.py:170-182 predict_input, utils/graph_utils.py:373-402 the training graph).
#include "engine.hpp"

namespace ams {

// Split-bf16 pays where the exact-f32 kernels are matrix-pipe bound (f32-input MFMA = 157 TFLOP/s against ~5 TB/s of HBM:
// ~31 FLOP per byte): few rows (the streaming kernel needs >= 32768), a weight panel too large for the streaming kernel,
// or an arithmetic intensity 2KN / 4(K+N) of 20 FLOP/B and more (64 -> 384 and wider, at any batch size).
bool split_pays(const PwArgs& a) {
    if (a.K < 32 || a.K % 8 != 0 || a.M < 256) return false;
    return a.M < 32768 || !pointwise_stream_applies(a) || (int64_t)a.K * a.N >= 40 * (int64_t)(a.K + a.N);
}

// live (training) 1x1 layer or its input gradient: same split-bf16 rule as the frozen path, the weights are split right
// before the launch because they change every step (one small kernel; the panels live in one shared scratch buffer)
int live_pointwise(ams_student* s, const PwArgs& a, hipStream_t st) {
    const bool split = s->matmul_mode != AMS_MATMUL_F32 && s->panel_scratch && split_pays(a) && a.Kw == a.K && a.ldx % 4 == 0;
    if (!split) return launch_pointwise(a, st);
    // three-part split (6 MFMAs, f32-level products): gradients amplify product error ~1e5 x on this graph, the two-part
    // split of the frozen path would put the step outside the f32 error class
    const int Kp = (a.K + 31) / 32 * 32;
    const size_t plane = (size_t)a.N * Kp;
    if (s->tp_fresh) {                                  // split once per step (forward_live) instead of once per launch
        auto it = s->tp_index.find({a.w, a.w_sk == 1 ? 1 : 0});
        if (it != s->tp_index.end()) {
            const SplitJob& j = s->tp_jobs[it->second];
            if (j.K == a.K && j.N == a.N && j.sk == a.w_sk && j.sn == a.w_sn) {
                if (s->tp_wait) { AMS_CHECK_HIP(hipStreamWaitEvent(st, s->ev_tp, 0)); s->tp_wait = false; }      // the split ran on the side stream
                // forward products of the step on two fp16 parts (3 MFMAs): activations and weights are O(1) there; the input-gradient GEMMs
                // (red_mode 2, transposed panels: no fp16 planes) keep three bf16 parts — gradients span a range fp16 cannot hold
                if (s->matmul_mode == AMS_MATMUL_SPLIT_F16 && s->train_fwd_f16 && j.f16 && pointwise_f16_applies(a))
                    return launch_pointwise_split_f16(a, j.p0 + 3 * j.plane, j.plane, j.Kp, st);
                return launch_pointwise_split3(a, j.p0, j.p0 + j.plane, j.p0 + 2 * j.plane, j.Kp, st);
            }
        }
    }
    AMS_REQUIRE(3 * plane <= s->panel_elems, "live_pointwise: panel scratch too small");
    uint16_t* p0 = s->panel_scratch;
    int rc = launch_split_weights3(a.w, a.w_sk, a.w_sn, a.K, a.N, Kp, p0, p0 + plane, p0 + 2 * plane, st);
    if (rc) return rc;
    return launch_pointwise_split3(a, p0, p0 + plane, p0 + 2 * plane, Kp, st);
}

// =======================================================================================================
// frozen inference (BN folded; what the edge device runs)
// =======================================================================================================
// The buffers one pass may use: the whole student's, or frames b0 .. b0 + bp - 1 of each (all are sized for max_batch frames).
struct FrozenView {
    float* act[4];                             // ping-pong pool
    uint16_t* xsplit; size_t xsplit_plane;     // parts of a stride-16 block's input, and the elements one part plane holds here
    float *pooled, *pool_a, *img_bias, *logits, *scratch;
    const void* frames; int B;                 // the frames of the pass
    int reserved;                              // act[reserved] holds the late section's input for ALL sub-batches: never a target (-1: none)
};
static FrozenView view_whole(const ams_student* s, const void* frames, int B) {
    return {{s->act[0], s->act[1], s->act[2], s->act[3]}, s->xsplit, s->xsplit_plane, s->pooled, s->pool_a, s->img_bias, s->logits, s->scratch, frames, B, -1};
}
// frames b0 .. b0 + bp - 1 of the late section: the same activation buffers for every sub-batch (the input of all of them in
// act[input_i]), the head's outputs in their place
static FrozenView view_late(const ams_student* s, FrozenView v, int b0, int bp, int input_i) {
    v.pooled += (size_t)b0 * s->L[s->iPool].d.cin;
    v.pool_a += (size_t)b0 * s->L[s->iPool].d.cout;
    v.img_bias += (size_t)b0 * s->L[s->iProj].d.cout;
    v.logits += (size_t)b0 * s->h * s->w * 32;
    v.B = bp; v.reserved = input_i;
    return v;
}
// frames b0 .. b0 + bp - 1 of `frames` in their own slice of every buffer (one part of forward_frozen_dual)
static FrozenView view_slice(const ams_student* s, const void* frames, int dtype, int b0, int bp) {
    const ams_student_config& c = s->cfg;
    FrozenView v = view_late(s, view_whole(s, (const char*)frames + (size_t)b0 * c.height * c.width * 3 * (dtype == AMS_DT_U8 ? 1 : 4), bp), b0, bp, -1);
    for (int k = 0; k < 4; ++k) v.act[k] += (size_t)b0 * (s->act_elems / c.max_batch);
    if (v.xsplit) { v.xsplit += 3 * (s->xsplit_plane / c.max_batch) * b0; v.xsplit_plane = (s->xsplit_plane / c.max_batch) * bp; }
    v.scratch += image_colsum_scratch(b0, s->L[s->iPool].d.cin);
    return v;
}

// bf16 / fp16 parts of a block input in FrozenView::xsplit, as the project GEMM in front of a streamed block leaves them
struct PartsFmt { int np = 0, fmt = 0; };      // np 0: none; PwArgs::ysplit_np / ysplit_fmt
// where a pass stands: the next layer, its input (in act[cur_i]) and what else exists of that input
// cur_f32: act[cur_i] really holds that input as f32 (false: the project GEMM before wrote the part planes only, BlockPlan::out_parts_only)
struct Cursor { int i; const float* cur; int cur_i; PartsFmt parts; bool cur_f32 = true; };

static int other(const FrozenView& v, int avoid0, int avoid1) {
    for (int k = 0; k < 4; ++k) if (k != avoid0 && k != avoid1 && k != v.reserved) return k;
    return -1;
}

// ---- the plan of one inverted-residual block: decided before any launch of that block, by plan_block alone ----------------------------
enum PwForm { PW_F32, PW_BF16_1, PW_BF16_2, PW_BF16_3, PW_F16 };      // products of a 1x1 layer: exact f32 | 1, 2, 3 bf16 parts | two fp16 parts
enum BlockForm { BLOCK_WHOLE,                  // k_block.hip
                 BLOCK_TILED,                  // k_expand_dw.hip, then the project GEMM
                 BLOCK_STREAM, BLOCK_WREG,     // k_xdw_stream.hip | k_xdw_wreg.hip, then the project GEMM
                 BLOCK_LAYERS };               // layer by layer
struct BlockPlan {
    BlockForm form = BLOCK_LAYERS;
    bool expand = false;                       // the block opens with an expand layer (the first block does not)
    bool h16 = false, x6 = false;              // whole block: expand + project on fp16 parts | expand on three bf16 parts
    int np = 0; const uint16_t* wparts = nullptr; int64_t wplane = 0;      // streamed: the expand layer's product form and panels
    PartsFmt in;                               // streamed: the block input also comes as parts
    PwForm expand_form = PW_F32;               // layer by layer
    bool dw_project = false;                   // layer by layer: depthwise + project as launch_dw_project
    bool d_h2i = false;                        // the depthwise result reaches the project GEMM as fp16 pairs (PwArgs::x_fmt 1)
    PwForm project_form = PW_F32;
    PartsFmt out;                              // what the project GEMM leaves in xsplit for the next block
    bool out_parts_only = false;               // ... and nothing else: the next block reads the planes and adds no residual (PwArgs::y_skip_f32)
};

// arguments of the backbone's 1x1 layer `layer` over B frames; `res`: the block input, where the layer adds it.  The planner asks with
// null tensors: the kernel choice depends on the shape and on whether a residual is added, not on where anything lies
static PwArgs layer_args(const ams_student* s, int layer, int B, const float* x, float* y, const float* res) {
    const LayerRt& l = s->L[layer];
    PwArgs a = pw_args(x, (int64_t)B * l.px_in, l.d.cin, l.d.cin, s->fparams + l.d.w_off, l.d.cout, y, l.d.cout);
    a.scale = l.fscale; a.shift = l.fshift; a.act = l.d.act;
    if (l.d.role == AMS_ROLE_PROJECT && l.d.residual_from) { a.res = res; a.ldr = l.d.cout; }
    return a;
}

// Layer l as a block kernel reads it (block_call.hpp): weights in `params`, BN as scale / shift, and the panels picked for it: np = 0 none,
// 1 .. 3 the bf16 parts, AMS_NP_F16 the two fp16 parts
static ConvLayer conv_layer(const LayerRt& l, const float* params, const float* scale, const float* shift, int np = 0) {
    ConvLayer c;
    c.w = params + l.d.w_off; c.scale = scale; c.shift = shift; c.act = l.d.act;
    c.np = np; c.Kp = l.Kp;
    if (np == AMS_NP_F16) { c.panels = l.whf; c.plane = (int64_t)l.d.cout * l.Kp; }
    else if (np) { c.panels = l.whi; c.plane = (int64_t)(l.wlo - l.whi); }
    return c;
}
static ConvLayer frozen_layer(const ams_student* s, int i, int np = 0) { return conv_layer(s->L[i], s->fparams, s->L[i].fscale, s->L[i].fshift, np); }
// the block call of expand (or stem) layer ie, depthwise layer ie + 1 and, with_project, project layer ie + 2, over the B frames of x
static BlockCall frozen_block(const ams_student* s, int ie, int np, bool with_project, int B, const float* x, float* y) {
    const LayerRt &le = s->L[ie], &ld = s->L[ie + 1];
    BlockCall c;
    c.x = x; c.B = B; c.H = le.Hin; c.W = le.Win; c.Cin = le.d.cin; c.Cexp = le.d.cout; c.stride = ld.d.stride; c.rate = ld.d.rate; c.y = y; c.vecs = le.blk_vecs;
    c.expand = frozen_layer(s, ie, np);
    c.dw = frozen_layer(s, ie + 1);
    if (!with_project) return c;
    c.project = frozen_layer(s, ie + 2, np == AMS_NP_F16 ? np : 0); c.Cout = s->L[ie + 2].d.cout; c.residual = s->L[ie + 2].d.residual_from != 0;
    return c;
}

// frozen 1x1 layer: late layers (few rows, wide K/N: matrix-pipe bound) go through the split kernels, in the matmul mode's form; a layer
// whose fp16 panels did not survive the freeze's range check runs three bf16 parts.  `streamable`: see plan_block
static PwForm pointwise_form(const ams_student* s, int layer, const PwArgs& a, bool streamable) {
    const LayerRt& l = s->L[layer];
    if (s->matmul_mode == AMS_MATMUL_F32 || !l.whi || !(split_pays(a) || (streamable && a.K % 8 == 0 && a.K >= 32))) return PW_F32;
    switch (s->matmul_mode) {
        case AMS_MATMUL_SPLIT_F16: return l.whf && pointwise_f16_applies(a) ? PW_F16 : PW_BF16_3;
        case AMS_MATMUL_SPLIT_BF16_X6: return PW_BF16_3;
        case AMS_MATMUL_BF16: return PW_BF16_1;
        default: return PW_BF16_2;
    }
}

// layer k starts a block whose expand + depthwise run as the streaming kernel (stride-16 blocks, split-bf16 modes, a few
// frames: below that the launch cannot fill the chip)
static bool stream_ok(const ams_student* s, int B, int k) {
    if (!(s->fuse_expand_dw_stream && k + 1 <= s->n_backbone && s->L[k].d.role == AMS_ROLE_EXPAND && s->L[k + 1].d.role == AMS_ROLE_DEPTHWISE &&
          (int64_t)B * s->L[k].px_in >= s->stream_min_rows && (int64_t)s->L[k + 1].px_out * s->L[k + 1].d.cout * 4 < 0x7fffffffLL &&
          expand_dw_stream_supported(s->L[k].d.cin, s->L[k].d.cout, s->L[k + 1].d.stride, s->L[k + 1].d.rate)))
        return false;
    // stride 2 on the streaming kernel is correct and tested but measured no faster than the tiled kernel (the expand runs at
    // full resolution either way: 412 vs 376 us on the first such block) — only with option value 2
    if (s->L[k + 1].d.stride != 1 && s->fuse_expand_dw_stream < 2) return false;
    if (s->L[k].d.cin <= 32) return true;                        // exact-f32 form: any matmul mode
    return s->matmul_mode != AMS_MATMUL_F32 && s->L[k].whi && s->L[k].Kp == s->L[k].d.cin;
}
// `np` of the streaming launchers for expand layer k
// (Cin <= 32 streams on the exact-f32 form whatever the mode: no fp16 parts there, so no fp16-pair hand-over of d either)
static int stream_np(const ams_student* s, int k) {
    if (s->matmul_mode == AMS_MATMUL_SPLIT_F16 && s->L[k].whf && s->L[k].d.cin > 32) return AMS_NP_F16;
    return s->matmul_mode == AMS_MATMUL_SPLIT_BF16_X6 || s->matmul_mode == AMS_MATMUL_SPLIT_F16 ? 3 : s->matmul_mode == AMS_MATMUL_BF16 ? 1 : 2;
}
// ... and the parts of its input it can take ready-made.  The format is the consumer's: fp16 pairs only where that expand layer runs the fp16
// form (its panels survived the freeze's range check, Cin > 32).  An expand layer moved off the fp16 form gets no parts: the streaming kernel
// then splits f32 `x` itself, and a 160-channel block takes the unfused path (rare; its speed does not matter).
static PartsFmt stream_parts(const ams_student* s, int k) {
    PartsFmt f;
    const int np = stream_np(s, k);
    if (np == AMS_NP_F16) { f.np = 2; f.fmt = 1; }
    else if (s->matmul_mode != AMS_MATMUL_SPLIT_F16) f.np = np;
    return f;
}

// The plan of the block that starts at layer i, for the frames of view v, when the block before it left `in` in xsplit.  Launches nothing.
static BlockPlan plan_block(const ams_student* s, const FrozenView& v, int i, PartsFmt in) {
    BlockPlan p;
    const int B = v.B, nb = s->n_backbone;
    const auto role = [&](int k) { return k <= nb ? s->L[k].d.role : -1; };
    p.expand = role(i) == AMS_ROLE_EXPAND;
    const int id = i + (p.expand ? 1 : 0), ij = id + 1;       // the depthwise and the project layer
    const LayerRt& le = s->L[i];
    const LayerRt& ld = s->L[id];
    const LayerRt& lj = s->L[ij];
    if (s->fuse_block && p.expand && role(id) == AMS_ROLE_DEPTHWISE && role(ij) == AMS_ROLE_PROJECT &&
        (!lj.d.residual_from || lj.d.residual_from == i - 1) &&
        block_fused_supported(le.d.cin, le.d.cout, lj.d.cout, ld.d.stride, ld.d.rate, lj.d.residual_from != 0)) {
        // early blocks: only the block input and output touch HBM (k_block.hip)
        p.form = BLOCK_WHOLE;
        // three-part split products for the expand layer when K >= 24 (not in the exact-f32 mode; the one- and two-part modes
        // concern the late layers only: the early blocks keep f32-level products there too)
        // fp16 form (AMS_MATMUL_SPLIT_F16): expand (any K, 16 included) and project products as 3 fp16 MFMAs each
        p.h16 = s->block_x6 && s->matmul_mode == AMS_MATMUL_SPLIT_F16 && le.whf && lj.whf && le.Kp == 32;
        p.x6 = !p.h16 && s->block_x6 && s->matmul_mode != AMS_MATMUL_F32 && le.whi && le.Kp == 32 && le.d.cin > 16;
        return p;
    }
    // a 160-channel block streams only on ready-made parts (k_xdw_wreg.hip), or with option value 2
    if (stream_ok(s, B, i) && (le.d.cin <= 96 || in.np || s->fuse_expand_dw_stream >= 2)) {
        // stride-16 blocks: expand + depthwise streamed through an LDS ring, split-bf16 products (bit-identical to the two
        // kernels it replaces); the 6x-expanded tensor is never written
        // 160 -> 960: expand weights in registers, the operand staged once per block in LDS (k_xdw_wreg.hip); with 30 channel
        // chunks the LDS-weight form is bound by its passes over the operand
        p.form = le.d.cin > 96 && in.np ? BLOCK_WREG : BLOCK_STREAM;
        p.in = in;
        p.np = stream_np(s, i);
        p.h16 = p.np == AMS_NP_F16;
        p.wparts = p.h16 ? le.whf : le.whi;
        p.wplane = p.h16 ? (int64_t)le.d.cout * le.Kp : (int64_t)(le.wlo - le.whi);
    } else if (s->fuse_expand_dw && p.expand && role(id) == AMS_ROLE_DEPTHWISE &&
               expand_dw_supported(le.d.cin, le.d.cout, ld.d.stride, ld.d.rate) &&
               (s->fuse_expand_dw >= 2 || le.d.cin <= 24 || ld.d.stride == 2)) {
        // expand + depthwise in one kernel: the 6x-expanded tensor stays in LDS
        p.form = BLOCK_TILED;
    } else {
        if (p.expand) {
            // an expand layer the streaming kernel can take forms its products the same way when it runs alone (split bf16), so
            // that the result does not depend on batch size or on AMS_OPT_FUSE_EXPAND_DW_STREAM
            const bool streamable = role(id) == AMS_ROLE_DEPTHWISE && le.Kp == le.d.cin && le.d.cin >= 64 &&
                                    expand_dw_stream_supported(le.d.cin, le.d.cout, ld.d.stride, ld.d.rate);
            p.expand_form = pointwise_form(s, i, layer_args(s, i, B, nullptr, nullptr, nullptr), streamable);
        }
        if (s->fuse_dw_project && s->matmul_mode == AMS_MATMUL_SPLIT_BF16 &&   /* two-part split only */ role(id) == AMS_ROLE_DEPTHWISE &&
            role(ij) == AMS_ROLE_PROJECT && lj.whi && (int64_t)B * ld.px_out < 32768 && (int64_t)B * ld.px_out >= 256 &&
            lj.Kp == ld.d.cin && dw_project_supported(ld.d.cin, lj.d.cout, ld.d.stride, ld.d.rate)) {
            // depthwise + project in one kernel (split-bf16 GEMM that computes its own operand): d never reaches HBM
            p.dw_project = true;
            return p;
        }
    }
    if (role(ij) != AMS_ROLE_PROJECT) return p;                  // a malformed table: the launch code reports it
    const PwArgs a = layer_args(s, ij, B, nullptr, nullptr, s->fparams);
    p.project_form = pointwise_form(s, ij, a, false);
    // fp16 form: the depthwise result goes to the project GEMM as fp16 pairs (PwArgs::x_fmt 1) when that GEMM runs the fp16 product
    p.d_h2i = (p.form == BLOCK_STREAM || p.form == BLOCK_WREG) && p.h16 && p.project_form == PW_F16 && ld.d.cout % 8 == 0 && !s->emulate_bf16_storage;
    // the next block streams: its expand GEMM takes this result as parts, written here once instead of being split by every
    // channel-chunk block there — when the GEMM chosen has the vector epilogue that writes them, and they fit
    if (stream_ok(s, B, ij + 1) && v.xsplit && (size_t)a.M * a.N <= v.xsplit_plane && p.project_form != PW_F32 && pointwise_split_writes_parts(a) &&
        !(s->emulate_bf16_storage && lj.px_out == (int64_t)s->h * s->w))       // (the parts would be those of the unrounded result)
        p.out = stream_parts(s, ij + 1);
    // The f32 copy of that result is read again only as the next block's residual or by a streaming kernel that was not given parts.  The
    // next block (expand ij + 1, depthwise, project ij + 3) streams on the planes (stream_ok above, and in.np admits every width); without a
    // residual there nothing reads the f32 form: 4 M N bytes the fp16 GEMM's vector epilogue does not store
    // (not across the boundary between the early section and a sub-batched late one: the late passes start without parts)
    if ((s->fuse_head & 2) && p.out.np && p.project_form == PW_F16 && !s->emulate_bf16_storage && !(s->late_subbatch > 0 && B > s->late_subbatch) && ij + 3 <= nb && role(ij + 3) == AMS_ROLE_PROJECT &&
        !s->L[ij + 3].d.residual_from && !(s->fuse_block && block_fused_supported(s->L[ij + 1].d.cin, s->L[ij + 1].d.cout, s->L[ij + 3].d.cout,
                                                                                  s->L[ij + 2].d.stride, s->L[ij + 2].d.rate, false)))
        p.out_parts_only = true;
    return p;
}

// one frozen 1x1 layer in the form planned for it
static int frozen_pointwise(ams_student* s, int layer, const PwArgs& a, PwForm form, hipStream_t st) {
    const LayerRt& l = s->L[layer];
    if (a.x_fmt != 0 && form != PW_F16) { set_error("frozen_pointwise: layer %d was handed fp16 pairs but does not run the fp16 product", layer); return AMS_E_STATE; }
    switch (form) {
        case PW_F16: RUNK(layer, pw_bytes(a), launch_pointwise_split_f16(a, l.whf, (int64_t)l.d.cout * l.Kp, l.Kp, st)); break;
        case PW_BF16_3: RUNK(layer, pw_bytes(a), launch_pointwise_split3(a, l.whi, l.wlo, l.wlo3, l.Kp, st)); break;
        case PW_BF16_2: RUNK(layer, pw_bytes(a), launch_pointwise_split(a, l.whi, l.wlo, l.Kp, st)); break;
        case PW_BF16_1: RUNK(layer, pw_bytes(a), launch_pointwise_split1(a, l.whi, l.Kp, st)); break;
        case PW_F32: RUNK(layer, pw_bytes(a), launch_pointwise(a, st)); break;
    }
    return AMS_OK;
}

// ---- the launches: each form builds its arguments from the plan and advances the cursor ------------------------------------------------
static int run_first_block(ams_student* s, const FrozenView& v, int dtype, Cursor& c, hipStream_t st) {
    const ams_student_config& cf = s->cfg;
    const int B = v.B;
    float* y = v.act[0];
    const LayerRt& l = s->L[1];
    const LayerRt& ld = s->L[2];
    const LayerRt& lj = s->L[3];
    const double in_bytes = (double)B * cf.height * cf.width * 3 * (dtype == AMS_DT_U8 ? 1 : 4);
    c.i = 2;
    if (s->fuse_first_block && s->n_backbone >= 3 && l.d.cout == 32 && ld.d.role == AMS_ROLE_DEPTHWISE && ld.d.cin == 32 &&
        ld.d.stride == 1 && ld.d.rate == 1 && lj.d.role == AMS_ROLE_PROJECT && lj.d.cin == 32 && lj.d.cout == 16 &&
        !lj.d.residual_from) {
        // stem + depthwise + project of the first block in one kernel: the 32-channel half-resolution tensor stays in LDS
        const double bytes = in_bytes + 4.0 * B * lj.px_out * lj.d.cout + 4.0 * (27 * 32 + 9 * 32 + 32 * 16);
        const bool h16 = s->fuse_first_block < 2 && s->block_x6 && s->matmul_mode == AMS_MATMUL_SPLIT_F16 && l.whf && lj.whf && lj.Kp == 32;
        const bool x6 = s->fuse_first_block < 2 && !h16 && s->block_x6 && s->matmul_mode != AMS_MATMUL_F32 && l.whi;
        BlockCall b = frozen_block(s, 1, h16 ? AMS_NP_F16 : x6 ? 3 : 0, true, B, nullptr, y);
        b.frames = v.frames; b.dtype = dtype; b.pixel_scale = cf.pixel_scale; b.H = cf.height; b.W = cf.width; b.Cin = 3;
        if (s->fuse_first_block >= 2) RUNK(3, bytes, launch_first_block_tiles(b, st));
        else RUNK(3, bytes, launch_first_block(b, st));
        c.i = 4;
    } else {
        const double bytes = in_bytes + 4.0 * B * l.px_out * l.d.cout;
        RUNK(1, bytes, launch_stem(v.frames, dtype, B, cf.height, cf.width, s->fparams + l.d.w_off, l.d.cout, l.fscale, l.fshift, l.d.act,
                                   cf.pixel_scale, y, st));
    }
    c.cur = y; c.cur_i = 0; c.parts = PartsFmt();
    return AMS_OK;
}

// the project GEMM (+ block input) on the depthwise result d = act[d_i]; the block is done
static int run_project(ams_student* s, const FrozenView& v, Cursor& c, const BlockPlan& p, int ij, const float* d, int d_i, hipStream_t st) {
    const LayerRt& l = s->L[ij];
    AMS_REQUIRE(l.d.role == AMS_ROLE_PROJECT, "engine: expected project at layer %d", ij);
    const int o = other(v, c.cur_i, d_i);
    PwArgs a = layer_args(s, ij, v.B, d, v.act[o], c.cur);
    a.x_fmt = p.d_h2i ? 1 : 0;
    AMS_REQUIRE(!a.res || c.cur_f32, "engine: layer %d adds a block input that was left as part planes only", ij);
    if (p.out.np) { a.ysplit = v.xsplit; a.ysplit_plane = a.M * a.N; a.ysplit_np = p.out.np; a.ysplit_fmt = p.out.fmt; a.y_skip_f32 = p.out_parts_only ? 1 : 0; }
    RUN(frozen_pointwise(s, ij, a, p.project_form, st));
    if (s->emulate_bf16_storage && l.px_out == (int64_t)s->h * s->w)
        RUN(launch_round_bf16(v.act[o], (int64_t)v.B * l.px_out * l.d.cout, st));            // block input as bf16 storage would hold it
    c.cur = v.act[o]; c.cur_i = o; c.i = ij + 1; c.parts = p.out; c.cur_f32 = !p.out_parts_only;
    return AMS_OK;
}

static int run_block_whole(ams_student* s, const FrozenView& v, Cursor& c, const BlockPlan& p, hipStream_t st) {
    const int B = v.B, i = c.i;
    const LayerRt& le = s->L[i];
    const LayerRt& ld = s->L[i + 1];
    const LayerRt& lj = s->L[i + 2];
    const int o = other(v, c.cur_i, -1);
    const bool res = lj.d.residual_from != 0;
    const double bytes = 4.0 * ((double)B * (le.px_in * le.d.cin * (res ? 2 : 1) + lj.px_out * lj.d.cout) + (double)le.d.cin * le.d.cout +
                                9.0 * ld.d.cin + (double)lj.d.cin * lj.d.cout);
    // algorithmic FLOPs (no halo, no padding): the kernel is bound by the exact-f32 matrix pipe, not by HBM
    const double fl_e = 2.0 * B * (double)le.px_in * le.d.cin * le.d.cout, fl_p = 2.0 * B * (double)lj.px_out * lj.d.cin * lj.d.cout;
    s->prof_flops = 2.0 * B * (double)ld.px_out * 9.0 * ld.d.cin + (p.h16 ? 0.0 : fl_p) + (p.x6 || p.h16 ? 0.0 : fl_e);
    s->prof_flops_x6 = p.h16 ? fl_e + fl_p : p.x6 ? fl_e : 0.0;
    RUNK(i + 2, bytes, launch_block_fused(frozen_block(s, i, p.h16 ? AMS_NP_F16 : p.x6 ? 3 : 0, true, B, c.cur, v.act[o]), st));
    c.cur = v.act[o]; c.cur_i = o; c.i = i + 3; c.parts = PartsFmt();
    return AMS_OK;
}

// expand + depthwise in one kernel (tiled or streamed), then the project GEMM
static int run_block_expand_dw(ams_student* s, const FrozenView& v, Cursor& c, const BlockPlan& p, hipStream_t st) {
    const int B = v.B, i = c.i;
    const LayerRt& le = s->L[i];
    const LayerRt& ld = s->L[i + 1];
    const int o = other(v, c.cur_i, -1);
    const double bytes = 4.0 * ((double)B * (le.px_in * le.d.cin + ld.px_out * ld.d.cout) + (double)le.d.cin * le.d.cout + 9.0 * ld.d.cin);
    const uint16_t* x_parts = p.in.np ? v.xsplit : nullptr;
    const int64_t xplane = (int64_t)B * le.px_in * le.d.cin;
    // a block input left as part planes only (BlockPlan::out_parts_only): c.cur names its buffer, but only the planes may be read
    AMS_REQUIRE(c.cur_f32 || (x_parts && (p.form == BLOCK_WREG || (p.form == BLOCK_STREAM && le.d.cin > 32))),
                "engine: block at layer %d reads an f32 input that was left as part planes only", i);
    BlockCall b = frozen_block(s, i, 0, false, B, c.cur, v.act[o]);
    if (p.form == BLOCK_TILED) RUNK(i + 1, bytes, launch_expand_dw(b, st));
    else {
        b.expand.panels = p.wparts; b.expand.plane = p.wplane; b.expand.np = p.np;      // the plan's choice
        b.x_parts = x_parts; b.x_plane = xplane; b.y_fmt = p.d_h2i ? 1 : 0;
        if (p.form == BLOCK_WREG) RUNK(i + 1, bytes, launch_expand_dw_wreg(b, st));
        else RUNK(i + 1, bytes, launch_expand_dw_stream(b, st));
    }
    if (p.form != BLOCK_TILED && s->emulate_bf16_storage && ld.px_out == (int64_t)s->h * s->w)
        RUN(launch_round_bf16(v.act[o], (int64_t)B * ld.px_out * ld.d.cout, st));          // d as bf16 storage would hold it
    return run_project(s, v, c, p, i + 2, v.act[o], o, st);
}

static int run_block_layers(ams_student* s, const FrozenView& v, Cursor& c, const BlockPlan& p, hipStream_t st) {
    const float* P = s->fparams;
    const int B = v.B;
    int i = c.i;
    const float* x = c.cur;
    int x_i = c.cur_i;
    if (p.expand) {
        const int o = other(v, c.cur_i, -1);
        RUN(frozen_pointwise(s, i, layer_args(s, i, B, x, v.act[o], nullptr), p.expand_form, st));
        x = v.act[o]; x_i = o; ++i;
    }
    const LayerRt& l = s->L[i];
    AMS_REQUIRE(l.d.role == AMS_ROLE_DEPTHWISE, "engine: expected depthwise at layer %d", i);
    const int o = other(v, c.cur_i, x_i);
    if (p.dw_project) {
        const LayerRt& lpj = s->L[i + 1];
        BlockCall b;
        b.x = x; b.B = B; b.H = l.Hin; b.W = l.Win; b.Cexp = l.d.cin; b.stride = l.d.stride; b.rate = l.d.rate; b.Cout = lpj.d.cout; b.y = v.act[o];
        b.dw = frozen_layer(s, i);
        b.project = frozen_layer(s, i + 1, 2); b.residual = lpj.d.residual_from != 0; b.res = c.cur;
        const double bytes = 4.0 * ((double)B * (l.px_in * l.d.cin + lpj.px_out * lpj.d.cout * (b.residual ? 2 : 1)) +
                                    (double)lpj.d.cin * lpj.d.cout + 9.0 * l.d.cin);
        RUNK(i + 1, bytes, launch_dw_project(b, st));
        c.cur = v.act[o]; c.cur_i = o; c.i = i + 2; c.parts = PartsFmt();
        return AMS_OK;
    }
    RUNK(i, dw_bytes(l, B), launch_depthwise(x, B, l.Hin, l.Win, l.d.cin, P + l.d.w_off, l.d.stride, l.d.rate, l.fscale,
                                             l.fshift, l.d.act, v.act[o], st));
    if (s->emulate_bf16_storage && l.px_out == (int64_t)s->h * s->w)
        RUN(launch_round_bf16(v.act[o], (int64_t)B * l.px_out * l.d.cout, st));
    return run_project(s, v, c, p, i + 1, v.act[o], o, st);
}

// blocks from the cursor up to layer i_stop: [expand] -> depthwise -> project (+ block input) each
static int run_blocks(ams_student* s, const FrozenView& v, Cursor& c, int i_stop, hipStream_t st) {
    while (c.i <= s->n_backbone && c.i < i_stop) {
        const BlockPlan p = plan_block(s, v, c.i, c.parts);
        AMS_REQUIRE(c.cur_f32 || p.form == BLOCK_STREAM || p.form == BLOCK_WREG, "engine: block at layer %d reads an f32 input that was left as part planes only", c.i);
        switch (p.form) {
            case BLOCK_WHOLE: RUN(run_block_whole(s, v, c, p, st)); break;
            case BLOCK_TILED: case BLOCK_STREAM: case BLOCK_WREG: RUN(run_block_expand_dw(s, v, c, p, st)); break;
            case BLOCK_LAYERS: RUN(run_block_layers(s, v, c, p, st)); break;
        }
    }
    return AMS_OK;
}

// the head on the backbone's result c.cur (the frames of the view)
static int run_head(ams_student* s, const FrozenView& v, const Cursor& c, hipStream_t st) {
    const float* P = s->fparams;
    const LayerRt& lp = s->L[s->iPool]; const LayerRt& la = s->L[s->iAspp]; const LayerRt& lc = s->L[s->iProj]; const LayerRt& ll = s->L[s->iLogits];
    const int B = v.B;
    AMS_REQUIRE(c.cur_f32, "engine: the head reads an f32 input that was left as part planes only");
    const int64_t HW = (int64_t)s->h * s->w, M = (int64_t)B * HW;
    // The image-pooling branch (global mean -> 1x1 + BN + ReLU -> its share of concat_projection as a per-image bias) is three
    // latency-bound launches on a handful of rows (58 us at 32 frames, 22 us at one).  With overlap_head it runs on the side stream
    // beside the aspp0 GEMM and joins before concat_projection (off by default, see the flag).
    const bool fork = s->overlap_head && !s->prof.on;
    hipStream_t ps = st;
    if (fork) {
        if (!s->side) RUN(create_side_stream(&s->side));
        if (!s->ev_fork) RUN(create_sync_event(&s->ev_fork));
        if (!s->ev_head) RUN(create_sync_event(&s->ev_head));
        AMS_CHECK_HIP(hipEventRecord(s->ev_fork, st));
        AMS_CHECK_HIP(hipStreamWaitEvent(s->side, s->ev_fork, 0));
        ps = s->side;
    }
    RUNK(s->iPool, 4.0 * M * lp.d.cin, launch_global_mean(c.cur, B, HW, lp.d.cin, v.pooled, v.scratch, ps));
    {   // image_pooling conv + BN + ReLU on the pooled vector
        PwArgs a = pw_args(v.pooled, B, lp.d.cin, lp.d.cin, P + lp.d.w_off, lp.d.cout, v.pool_a, lp.d.cout);
        a.scale = lp.fscale; a.shift = lp.fshift; a.act = lp.d.act;
        RUNK(s->iPool, pw_bytes(a), launch_pointwise(a, ps));
        // the broadcast pool branch enters concat_projection as a per-image bias: W_proj[0:256]^T . pool
        PwArgs b = pw_args(v.pool_a, B, lp.d.cout, lp.d.cout, P + lc.d.w_off, lc.d.cout, v.img_bias, lc.d.cout);
        RUNK(s->iProj, pw_bytes(b), launch_pointwise(b, ps));
    }
    if (fork) AMS_CHECK_HIP(hipEventRecord(s->ev_head, s->side));
    const int o1 = other(v, c.cur_i, -1), o2 = other(v, c.cur_i, o1);
    PwArgs a = pw_args(c.cur, M, la.d.cin, la.d.cin, P + la.d.w_off, la.d.cout, v.act[o1], la.d.cout);
    a.scale = la.fscale; a.shift = la.fshift; a.act = la.d.act;
    PwArgs b = pw_args(v.act[o1], M, la.d.cout, la.d.cout, P + lc.d.w_off + (int64_t)lp.d.cout * lc.d.cout, lc.d.cout,
                       v.act[o2], lc.d.cout);
    b.img_bias = v.img_bias; b.rows_per_img = HW; b.scale = lc.fscale; b.shift = lc.fshift; b.act = lc.d.act;
    PwArgs d = pw_args(v.act[o2], M, lc.d.cout, lc.d.cout, P + ll.d.w_off, ll.d.cout, v.logits, 32);
    d.shift = P + ll.d.gamma_off;      // biases
    const PwForm fa = pointwise_form(s, s->iAspp, a, false), fb = pointwise_form(s, s->iProj, b, false), fd = pointwise_form(s, s->iLogits, d, false);
    // The three GEMMs as one chained kernel (k_head_chain.hip): only where each of them would run the two-fp16-part product — a layer the
    // freeze moved off it (whf == nullptr), another matmul mode or too few rows for the split forms keep the three launches, whose bits
    // the chain reproduces
    // (a sub-batched late section, AMS_OPT_LATE_SUBBATCH, keeps them too: the option is off by default and its passes are told apart by their GEMMs)
    if ((s->fuse_head & 1) && !s->emulate_bf16_storage && !(s->late_subbatch > 0) && fa == PW_F16 && fb == PW_F16 && fd == PW_F16 && la.Kp == la.d.cin && lc.Kp == la.d.cout &&
        ll.Kp == lc.d.cout && head_chain_supported(la.d.cin, la.d.cout, la.d.cout, lc.d.cout, lc.d.cout, ll.d.cout)) {
        if (fork) AMS_CHECK_HIP(hipStreamWaitEvent(st, s->ev_head, 0));
        // bytes: the operand, the three panels (two fp16 parts), the vectors and the 32-column logits
        const double bytes = 4.0 * M * (la.d.cin + 32) + 4.0 * ((double)la.Kp * la.d.cout + (double)lc.Kp * lc.d.cout + (double)ll.Kp * ll.d.cout) +
                             4.0 * (2.0 * la.d.cout + 2.0 * lc.d.cout + ll.d.cout + (double)B * lc.d.cout);
        s->prof_flops_x6 = 2.0 * M * ((double)la.d.cin * la.d.cout + (double)la.d.cout * lc.d.cout + (double)lc.d.cout * ll.d.cout);
        ConvLayer lg = frozen_layer(s, s->iLogits, AMS_NP_F16);
        lg.scale = nullptr; lg.shift = d.shift; lg.act = d.act;      // biases
        RUNK(s->iLogits, bytes, launch_head_chain(c.cur, M, la.d.cin, frozen_layer(s, s->iAspp, AMS_NP_F16), frozen_layer(s, s->iProj, AMS_NP_F16), lg,
                                                  v.img_bias, HW, ll.d.cout, v.logits, st));
        return AMS_OK;
    }
    RUN(frozen_pointwise(s, s->iAspp, a, fa, st));
    if (fork) AMS_CHECK_HIP(hipStreamWaitEvent(st, s->ev_head, 0));
    RUN(frozen_pointwise(s, s->iProj, b, fb, st));
    RUN(frozen_pointwise(s, s->iLogits, d, fd, st));
    return AMS_OK;
}

// One pass over the frames of view v.  Of the student it writes the profiler's records and the side stream / events that overlap_head
// creates on first use; every buffer comes from the view.
static int forward_frozen(ams_student* s, const FrozenView& v, int dtype, hipStream_t st) {
    Cursor c;
    RUN(run_first_block(s, v, dtype, c, st));
    // The output-stride-16 section (blocks 7-16 and the head) can run in sub-batches: its largest tensor, the depthwise result of
    // the 960-channel blocks, is 264 MB at 32 frames — written by one kernel, read by the next, and larger than the 256 MB Infinity
    // Cache.  At 16 frames the writer/reader pairs of that section meet in the cache (and every sub-batch reuses the same addresses).
    int i_late = s->n_backbone + 1;
    for (int k = 2; k <= s->n_backbone; ++k)
        if (s->L[k].d.role == AMS_ROLE_EXPAND && s->L[k].px_in == (int64_t)s->h * s->w) { i_late = k; break; }
    if (!(s->late_subbatch > 0 && v.B > s->late_subbatch && i_late <= s->n_backbone)) {
        RUN(run_blocks(s, v, c, s->n_backbone + 1, st));
        return run_head(s, v, c, st);
    }
    RUN(run_blocks(s, v, c, i_late, st));      // early section: the whole batch
    const int64_t late_in_frame = s->L[i_late].px_in * s->L[i_late].d.cin;
    for (int b0 = 0; b0 < v.B; b0 += s->late_subbatch) {
        const int bp = v.B - b0 < s->late_subbatch ? v.B - b0 : s->late_subbatch;
        const FrozenView lv = view_late(s, v, b0, bp, c.cur_i);
        AMS_REQUIRE(c.cur_f32, "engine: the late section's input was left as part planes only");
        Cursor lc = {i_late, c.cur + (int64_t)b0 * late_in_frame, c.cur_i, PartsFmt()};
        RUN(run_blocks(s, lv, lc, s->n_backbone + 1, st));
        RUN(run_head(s, lv, lc, st));
    }
    return AMS_OK;
}

// =======================================================================================================
// live forward: training-mode BN.  z = raw conv output, batch statistics -> (scale, shift), a = act(z*scale+shift)(+res)
// =======================================================================================================
// layer i opens an early block whose fine-tune step runs without the expanded tensors (k_xdw_train.hip)
bool train_recompute_block(const ams_student* s, int i) {
    if (!s->train_recompute || !s->xt_scratch || i < 2 || i + 1 > s->n_backbone) return false;
    const LayerRt& l = s->L[i];
    const LayerRt& ld = s->L[i + 1];
    return l.xx_g0 && l.d.role == AMS_ROLE_EXPAND && ld.d.role == AMS_ROLE_DEPTHWISE && xdw_train_supported(l.d.cin, l.d.cout, ld.d.stride, ld.d.rate) &&
           expand_dw_supported(l.d.cin, l.d.cout, ld.d.stride, ld.d.rate) && l.d.cout <= 1024 &&
           xdw_train_scratch(s->cfg.max_batch, l.Hin, l.Win, l.d.cin, l.d.cout) != (size_t)-1 &&      // too large for 32-bit offsets: layer-by-layer
           xdw_train_scratch(s->cfg.max_batch, l.Hin, l.Win, l.d.cin, l.d.cout) <= s->xt_floats;
}

// Stride-1 depthwise layer i of a block that keeps its tensors: its backward is ONE kernel that recomputes the expand layer's activation
// from z_e (backward(), k_conv.hip dw3x3_dgrad_bn_kernel) — so nothing in backward reads a_e, and at fuse_dgrad_bn >= 2 the forward
// does not write it either (dw3x3_fwd_bn_kernel applies the expand layer's BN + activation on its tap loads).
bool dw_fused_train(const ams_student* s, int i, int B) {
    if (i < 3 || i > s->n_backbone || !s->fuse_dgrad_bn || train_recompute_block(s, i - 1)) return false;
    const LayerRt& l = s->L[i];
    const LayerRt& prev = s->L[i - 1];
    return l.d.role == AMS_ROLE_DEPTHWISE && l.d.stride == 1 && prev.d.role == AMS_ROLE_EXPAND && prev.d.cout == l.d.cin && l.d.cin <= 1024 &&
           depthwise_dgrad_bn_scratch(B, l.Hin, l.Win, l.d.cin) <= s->scratch_floats;
}
// First block: the stem is the "expand" layer of depthwise layer 2, and the backward of the pair is one pass over dz and the frames that
// never reads the stem's activation either (backward(), launch_xdw_bwd_reduce_stem).
bool stem_fused_train(const ams_student* s) {
    const ams_student_config& c = s->cfg;
    return s->n_backbone >= 2 && s->train_recompute && s->L[1].d.role == AMS_ROLE_STEM && s->L[1].d.cout == 32 && s->L[2].d.role == AMS_ROLE_DEPTHWISE &&
           s->L[2].d.stride == 1 && s->L[2].d.rate == 1 && s->xt_scratch && xdw_stem_scratch(c.max_batch, c.height, c.width) != (size_t)-1 &&
           xdw_stem_scratch(c.max_batch, c.height, c.width) <= s->xt_floats;
}
bool dw_fused_train_fwd(const ams_student* s, int i, int B) {
    if (s->fuse_dgrad_bn < 2 || i < 2 || i > s->n_backbone) return false;
    if (!(i == 2 ? stem_fused_train(s) : dw_fused_train(s, i, B))) return false;
    return depthwise_fwd_bn_scratch(B, s->L[i].Hin, s->L[i].Win, s->L[i].d.cin, s->L[i].d.rate) <= s->scratch_floats;
}

// depthwise layer i feeds a project layer: with AMS_OPT_FUSE_OPERAND_BN bit 0 its activation a = act(z scale + shift) is never written — the
// project GEMM (forward) and the project weight gradient (backward) apply it on their operand loads (PwArgs / WgArgs x_mode 1)
bool operand_bn_act(const ams_student* s, int i) {
    if (!(s->fuse_operand_bn & 1) || i < 2 || i + 1 > s->n_backbone) return false;
    const LayerRt& l = s->L[i];
    const LayerRt& lj = s->L[i + 1];
    return l.d.role == AMS_ROLE_DEPTHWISE && lj.d.role == AMS_ROLE_PROJECT && lj.d.cin == l.d.cout && l.d.cout % 4 == 0 && l.d.cout <= 1024;
}

// most partial rows a GEMM with a fused column reduction can leave behind (PwArgs::red_mode): one per 64-row strip of the tiled split kernel
// (it also takes layers of >= 32768 rows when the panel is too large for the streaming kernel), one per block of the persistent streaming
// kernel (<= 8 per CU).  Sizing only: the launchers compare the exact row count with PwArgs::red_part_floats and drop the fusion when the
// rows would not fit (the caller then runs the separate reduction pass).
size_t red_rows_bound(int64_t M) {
    const size_t tiled = (size_t)(M / 64 + 8), streaming = M >= 32768 ? 8 * 512 : 0;
    return tiled > streaming ? tiled : streaming;
}

// what finishing a training-mode BN layer takes besides its sums: their centre (shifted sums: moving_mean is a good, rank-identical
// centre), 1 - decay and the moving statistics to update
struct BnEma { const float* center; float omd; float *mm, *mv; };
static BnEma bn_ema(const ams_student* s, const LayerRt& l, bool update_ema) {
    return {s->stats + l.d.mean_off, 1.0f - s->cfg.bn_decay, update_ema ? s->stats + l.d.mean_off : nullptr, update_ema ? s->stats + l.d.var_off : nullptr};
}
// (scale, shift, mean, rstd) of layer l from the partial rows [rows][stride] a kernel left (sum | sum of squares first in each row): one
// launch on a single rank, through the cross-rank sum of l.fsums otherwise
static int bn_from_partials(ams_student* s, LayerRt& l, const BnEma& e, const float* part, int rows, int64_t stride, double n_global,
                            const SyncCtx* sc, hipStream_t st) {
    const float *gamma = s->params + l.d.gamma_off, *beta = s->params + l.d.beta_off;
    if (!sc || !sc->cb)
        return launch_bn_fwd_finalize_partials(part, rows, stride, l.d.cout, l.fsums, n_global, e.center, gamma, beta, l.d.bn_eps, e.omd, e.mm, e.mv,
                                               l.scale, l.shift, l.mean, l.rstd, st);
    RUN(launch_partials_to_sums(part, rows, stride, l.d.cout, l.fsums, st));
    RUN(sync_doubles(sc, l.fsums, 2 * (size_t)l.d.cout, st));
    return launch_bn_finalize(l.fsums, n_global, l.d.cout, e.center, gamma, beta, l.d.bn_eps, e.omd, e.mm, e.mv, l.scale, l.shift, l.mean, l.rstd, st);
}

// pre_rows > 0: the kernel that wrote l.z already left the statistics' partial rows [pre_rows][2][C] in s->scratch
static int bn_train(ams_student* s, LayerRt& l, int64_t M_local, double n_global, bool update_ema, const SyncCtx* sc,
                    const float* res, hipStream_t st, int pre_rows = 0, bool act_pass = true, bool f64_sums = false) {
    const BnEma e = bn_ema(s, l, update_ema);
    if (pre_rows > 0) {
        RUN(bn_from_partials(s, l, e, s->scratch, pre_rows, 2 * (int64_t)l.d.cout, n_global, sc, st));
    } else if (f64_sums) {
        // a layer of a few rows: the sums in f64 throughout (k_elementwise.hip colstats_f64_kernel), the same launches with and without ranks
        RUN(launch_colstats_f64(l.z, M_local, l.d.cout, e.center, l.fsums, st));
        RUN(sync_doubles(sc, l.fsums, 2 * (size_t)l.d.cout, st));
        RUN(launch_bn_finalize(l.fsums, n_global, l.d.cout, e.center, s->params + l.d.gamma_off, s->params + l.d.beta_off, l.d.bn_eps, e.omd,
                               e.mm, e.mv, l.scale, l.shift, l.mean, l.rstd, st));
    } else if (!sc || !sc->cb) {
        // no cross-rank sum between the statistics and their use: the reduction's second stage finishes the BN arithmetic
        RUNK(0, 4.0 * M_local * l.d.cout,
             launch_colstats_bn(l.z, M_local, l.d.cout, e.center, l.fsums, s->scratch, n_global, s->params + l.d.gamma_off,
                                s->params + l.d.beta_off, l.d.bn_eps, e.omd, e.mm, e.mv, l.scale, l.shift, l.mean, l.rstd, st));
    } else {
        RUNK(0, 4.0 * M_local * l.d.cout, launch_colstats(l.z, M_local, l.d.cout, e.center, l.fsums, s->scratch, st));
        RUN(sync_doubles(sc, l.fsums, 2 * (size_t)l.d.cout, st));
        RUN(launch_bn_finalize(l.fsums, n_global, l.d.cout, e.center, s->params + l.d.gamma_off, s->params + l.d.beta_off, l.d.bn_eps, e.omd,
                               e.mm, e.mv, l.scale, l.shift, l.mean, l.rstd, st));
    }
    if (!act_pass) return AMS_OK;              // the consumer applies scale / shift / activation on its own loads of z
    RUNK(0, 4.0 * M_local * l.d.cout * (res ? 3 : 2), launch_bn_act(l.z, M_local, l.d.cout, l.scale, l.shift, l.d.act, res, l.a, st));
    return AMS_OK;
}

int forward_live(ams_student* s, const void* frames, int dtype, int B, int global_B, bool update_ema, const SyncCtx* sc,
                        hipStream_t st) {
    const ams_student_config& c = s->cfg;
    AMS_REQUIRE(c.trainable, "live forward needs a trainable student (activations are not allocated)");
    const float* P = s->params;
    // the parameters may have changed since the last call (Adam, restore): all live weight panels in one launch
    s->tp_fresh = false;
    s->tp_wait = false;
    if (s->matmul_mode != AMS_MATMUL_F32 && !s->tp_jobs.empty()) {
        // the first GEMM that reads a panel is a millisecond away (the early blocks run exact f32): the split runs on the side stream beside
        // the stem and the first blocks, and that GEMM waits for its event (live_pointwise)
        hipStream_t ts = st;
        if (s->overlap_wgrad && !s->prof.on && s->scratch2) {
            if (!s->side) RUN(create_side_stream(&s->side));
            if (!s->ev_fork) RUN(create_sync_event(&s->ev_fork));
            if (!s->ev_tp) RUN(create_sync_event(&s->ev_tp));
            AMS_CHECK_HIP(hipEventRecord(s->ev_fork, st));
            AMS_CHECK_HIP(hipStreamWaitEvent(s->side, s->ev_fork, 0));
            ts = s->side;
        }
        RUNK(0, 0.0, launch_split_batch(s->tp_jobs_dev, (int)s->tp_jobs.size(), s->tp_blocks, ts,
                                        s->train_fwd_f16 && s->matmul_mode == AMS_MATMUL_SPLIT_F16));
        if (ts != st) { AMS_CHECK_HIP(hipEventRecord(s->ev_tp, ts)); s->tp_wait = true; }
        s->tp_fresh = true;
    }
    {
        LayerRt& l = s->L[1];
        RUN(launch_stem(frames, dtype, B, c.height, c.width, P + l.d.w_off, l.d.cout, nullptr, nullptr, AMS_ACT_NONE,
                        c.pixel_scale, l.z, st));
        RUN(bn_train(s, l, (int64_t)B * l.px_out, (double)global_B * l.px_out, update_ema, sc, nullptr, st, 0, !dw_fused_train_fwd(s, 2, B)));
    }
    for (int i = 2; i <= s->n_backbone; ++i) {
        LayerRt& l = s->L[i];
        const float* x = s->L[i - 1].a;
        if (train_recompute_block(s, i)) {
            // early block: neither z_e nor a_e is written.  Statistics of z_e = x . W_e straight from x, then the inference kernel
            // expand + BN + ReLU6 + depthwise with the batch statistics -> the depthwise layer's raw output
            LayerRt& ld = s->L[i + 1];
            const BnEma e = bn_ema(s, l, update_ema);
            const double n_e = (double)global_B * l.px_out;
            if (s->train_recompute >= 2 && l.xx64 && s->xx_scratch && l.d.cin <= 32 &&
                xx_stats_scratch_doubles((int64_t)B * l.px_in, l.d.cin) <= s->xx_scratch_doubles) {
                // z_e is linear in x: its sums follow from XX = x^T x and g0 = sum x, formed in f64 in ONE cheap pass over x (k_xx_stats.hip);
                // the float copy is what the expand weight gradient reads (this rank's pixels), the doubles are summed over the ranks first
                const int KP = (l.d.cin + 15) / 16 * 16;
                RUNK(i, 4.0 * B * l.px_in * l.d.cin, launch_xx_gram(x, (int64_t)B * l.px_in, l.d.cin, s->xx_scratch, l.xx64, l.xx_g0, st));
                RUN(sync_doubles(sc, l.xx64, (size_t)KP * KP + KP, st));
                RUN(launch_expand_stats(l.xx64, l.d.cin, P + l.d.w_off, l.d.cout, n_e, e.center, s->params + l.d.gamma_off, s->params + l.d.beta_off,
                                        l.d.bn_eps, e.omd, e.mm, e.mv, l.scale, l.shift, l.mean, l.rstd, l.fsums, st));
            } else {
            int rows = 0;
            int64_t fstride = 0;
            RUNK(i, 4.0 * B * l.px_in * l.d.cin,
                 launch_xdw_fwd_stats(x, B, l.Hin, l.Win, l.d.cin, P + l.d.w_off, l.d.cout, e.center, s->xt_scratch, &rows, &fstride, st));
            {   // sums of x and x x^T over this rank's pixels, kept for the expand weight gradient
                const int KP = (l.d.cin + 15) / 16 * 16;
                RUN(launch_reduce_splits(s->xt_scratch + 2 * (int64_t)l.d.cout, rows, (int64_t)KP * KP + KP, l.xx_g0, st, fstride));
            }
            RUN(bn_from_partials(s, l, e, s->xt_scratch, rows, fstride, n_e, sc, st));
            }
            // ... which leaves the statistics of that raw output behind as one partial row per tile (no separate pass over z_d)
            int d_rows = 0;
            const bool d_stats = (s->fuse_gemm_red & 1) && expand_dw_stats_scratch(B, l.Hin, l.Win, l.d.cout, ld.d.stride) <= s->scratch_floats;
            BlockCall xdw;                       // the live weights with the batch statistics; the depthwise layer's raw output
            xdw.x = x; xdw.B = B; xdw.H = l.Hin; xdw.W = l.Win; xdw.Cin = l.d.cin; xdw.Cexp = l.d.cout; xdw.stride = ld.d.stride; xdw.rate = ld.d.rate; xdw.y = ld.z;
            xdw.expand = conv_layer(l, P, l.scale, l.shift);
            xdw.dw = conv_layer(ld, P, s->vec_ones, s->vec_zeros); xdw.dw.act = AMS_ACT_NONE;
            RUNK(i + 1, 4.0 * ((double)B * (l.px_in * l.d.cin + ld.px_out * ld.d.cout)),
                 launch_expand_dw(xdw, st, d_stats ? s->stats + ld.d.mean_off : nullptr, d_stats ? s->scratch : nullptr, d_stats ? &d_rows : nullptr));
            RUN(bn_train(s, ld, (int64_t)B * ld.px_out, (double)global_B * ld.px_out, update_ema, sc, nullptr, st, d_rows, !operand_bn_act(s, i + 1)));
            ++i;
            continue;
        }
        int pre_rows = 0;
        if (l.d.role == AMS_ROLE_DEPTHWISE && dw_fused_train_fwd(s, i, B)) {
            // BN + activation of the expand layer on the tap loads (its `a` was not written), the statistics of the result on the way out
            const LayerRt& le = s->L[i - 1];
            // (from 64 channels on in the LDS-tile form of k_dw_train.hip: BN + activation once per element instead of once per tap load)
            if (s->fuse_dgrad_bn >= 3 && l.d.cin % 64 == 0 && depthwise_fwd_bn2_scratch(B, l.Hin, l.Win, l.d.cin, l.d.rate) <= s->scratch_floats)
                RUNK(i, dw_bytes(l, B), launch_depthwise_fwd_bn2(le.z, B, l.Hin, l.Win, l.d.cin, P + l.d.w_off, l.d.rate, le.scale, le.shift, le.d.act,
                                                                 s->stats + l.d.mean_off, l.z, s->scratch, &pre_rows, st));
            else
            RUNK(i, dw_bytes(l, B), launch_depthwise_fwd_bn(le.z, B, l.Hin, l.Win, l.d.cin, P + l.d.w_off, l.d.rate, le.scale, le.shift, le.d.act,
                                                            s->stats + l.d.mean_off, l.z, s->scratch, &pre_rows, st));
        } else if (l.d.role == AMS_ROLE_DEPTHWISE) {
            RUNK(i, dw_bytes(l, B), launch_depthwise(x, B, l.Hin, l.Win, l.d.cin, P + l.d.w_off, l.d.stride, l.d.rate, nullptr, nullptr,
                                                     AMS_ACT_NONE, l.z, st));
        } else {
            PwArgs a = pw_args(x, (int64_t)B * l.px_in, l.d.cin, l.d.cin, P + l.d.w_off, l.d.cout, l.z, l.d.cout);
            if (l.d.role == AMS_ROLE_PROJECT && operand_bn_act(s, i - 1)) {
                // the depthwise layer's activation was not written: BN + activation on this GEMM's loads of its raw output
                const LayerRt& ld = s->L[i - 1];
                a.x = ld.z; a.x_mode = 1; a.x_act = ld.d.act; a.x_v0 = ld.scale; a.x_v1 = ld.shift; a.x_tmp = ld.a;
            }
            // the BN statistics of the result in this GEMM's epilogue, where the kernel chosen can do it
            if (s->fuse_gemm_red & 1) {
                a.red_mode = 1; a.red_center = s->stats + l.d.mean_off; a.red_part = s->scratch; a.red_part_floats = s->scratch_floats; a.red_rows_out = &pre_rows;
            }
            RUNK(0, pw_bytes(a), live_pointwise(s, a, st));
        }
        const float* res = l.d.residual_from ? s->L[l.d.residual_from].a : nullptr;
        const bool act_pass = !(l.d.role == AMS_ROLE_EXPAND && dw_fused_train_fwd(s, i + 1, B)) && !operand_bn_act(s, i);
        RUN(bn_train(s, l, (int64_t)B * l.px_out, (double)global_B * l.px_out, update_ema, sc, res, st, pre_rows, act_pass));
    }
    LayerRt& lp = s->L[s->iPool]; LayerRt& la = s->L[s->iAspp]; LayerRt& lc = s->L[s->iProj]; LayerRt& ll = s->L[s->iLogits];
    const float* feat = s->L[s->n_backbone].a;
    const int64_t HW = (int64_t)s->h * s->w, M = (int64_t)B * HW;
    RUN(launch_global_mean(feat, B, HW, lp.d.cin, s->pooled, s->scratch, st));
    {
        PwArgs a = pw_args(s->pooled, B, lp.d.cin, lp.d.cin, P + lp.d.w_off, lp.d.cout, lp.z, lp.d.cout);
        RUNK(0, pw_bytes(a), live_pointwise(s, a, st));
        RUN(bn_train(s, lp, B, (double)global_B, update_ema, sc, nullptr, st, 0, true, /*f64_sums=*/true));     // statistics over the batch only
        PwArgs b = pw_args(lp.a, B, lp.d.cout, lp.d.cout, P + lc.d.w_off, lc.d.cout, s->img_bias, lc.d.cout);
        RUNK(0, pw_bytes(b), live_pointwise(s, b, st));
    }
    {
        PwArgs a = pw_args(feat, M, la.d.cin, la.d.cin, P + la.d.w_off, la.d.cout, la.z, la.d.cout);
        RUNK(0, pw_bytes(a), live_pointwise(s, a, st));
        RUN(bn_train(s, la, M, (double)global_B * HW, update_ema, sc, nullptr, st));
        PwArgs b = pw_args(la.a, M, la.d.cout, la.d.cout, P + lc.d.w_off + (int64_t)lp.d.cout * lc.d.cout, lc.d.cout, lc.z, lc.d.cout);
        b.img_bias = s->img_bias; b.rows_per_img = HW;
        RUNK(0, pw_bytes(b), live_pointwise(s, b, st));
        RUN(bn_train(s, lc, M, (double)global_B * HW, update_ema, sc, nullptr, st));
        PwArgs d = pw_args(lc.a, M, lc.d.cout, lc.d.cout, P + ll.d.w_off, ll.d.cout, s->logits, 32);
        d.shift = P + ll.d.gamma_off;
        RUNK(0, pw_bytes(d), live_pointwise(s, d, st));
    }
    if (s->tp_wait) { AMS_CHECK_HIP(hipStreamWaitEvent(st, s->ev_tp, 0)); s->tp_wait = false; }      // no GEMM used a panel (tiny frames): join anyway
    return AMS_OK;
}

int check_call(const ams_student* s, const void* frames, int dtype, int batch) {
    AMS_REQUIRE(s && frames, "null student or frames");
    AMS_REQUIRE(dtype == AMS_DT_U8 || dtype == AMS_DT_F32, "frames must be uint8 or float32");
    AMS_REQUIRE(batch > 0 && batch <= s->cfg.max_batch, "batch %d outside 1..%d", batch, s->cfg.max_batch);
    return AMS_OK;
}

// Frozen inference as two to four parts on as many streams: the parts run the same layer sequence side by side (part 0 on the caller's
// stream, the others on streams the student owns; one fork and one join per step), each in its own slice of every activation buffer.
// A launch of this network rarely fills the chip to the end — tails of 1.05- or 2.1-round grids, latency-bound chains on a few blocks
// per CU — and the other parts' kernels fill those gaps.  Every frame is computed exactly as in a batch of the part's size.
// Whatever happens inside, every part stream is joined back into `st` before this returns.
// the part streams of an n-part plan exist (created on first use, outside any graph capture); false: run the one-stream plan instead
static bool ensure_part_streams(ams_student* s, int nparts, hipStream_t st) {
    bool missing = false;
    for (int p = 1; p < nparts; ++p) missing = missing || !s->part_stream[p - 1];
    if (!missing) return true;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return false;      // nothing is created inside a capture
    for (int p = 1; p < nparts; ++p)
        if (!s->part_stream[p - 1] && hipStreamCreateWithFlags(&s->part_stream[p - 1], hipStreamNonBlocking) != hipSuccess) return false;
    return true;
}

// nparts <= 1: the one-stream plan
static int forward_frozen_dual(ams_student* s, const void* frames, int dtype, int batch, hipStream_t st, int nparts) {
    if (nparts > 4) nparts = 4;
    if (nparts > batch) nparts = batch;
    if (nparts < 2 || !ensure_part_streams(s, nparts, st)) return forward_frozen(s, view_whole(s, frames, batch), dtype, st);
    AMS_REQUIRE(s->ev_fork_dual && s->part_stream[nparts - 2] && s->part_done[nparts - 2], "dual plan: part streams were not created");
    AMS_CHECK_HIP(hipEventRecord(s->ev_fork_dual, st));
    int rc = AMS_OK;
    int b0 = 0, forked = 0;
    for (int p = 0; p < nparts && !rc; ++p) {
        const int bp = batch / nparts + (p < batch % nparts ? 1 : 0);
        hipStream_t ps = p == 0 ? st : s->part_stream[p - 1];
        if (p > 0) {
            if (hipStreamWaitEvent(ps, s->ev_fork_dual, 0) != hipSuccess) { set_error("dual plan: fork failed"); rc = AMS_E_HIP; break; }
            forked = p;
        }
        rc = forward_frozen(s, view_slice(s, frames, dtype, b0, bp), dtype, ps);
        b0 += bp;
    }
    // join every stream that was forked, error or not: no part may still be writing the student's buffers after the return
    for (int p = 1; p <= forked; ++p) {
        if (hipEventRecord(s->part_done[p - 1], s->part_stream[p - 1]) != hipSuccess ||
            hipStreamWaitEvent(st, s->part_done[p - 1], 0) != hipSuccess) {
            (void)hipStreamSynchronize(s->part_stream[p - 1]);        // last resort: a host wait keeps the guarantee
            if (!rc) { set_error("dual plan: join failed"); rc = AMS_E_HIP; }
        }
    }
    return rc;
}

// Parts of the static rule (AMS_OPT_DUAL_STREAM = 1).  Round-5 sweep on MI355X at 512 x 1024 (tools/sweep_parts.py, 1 / 2 / 3 / 4 parts at 8 .. 64
// frames): two parts are 1-8 % ahead of one stream at every size from 8 frames on (0.94 vs 0.98 ms at 8, 1.81 vs 1.96 at 20, 2.56 vs 2.78 at 32,
// 3.28 vs 3.52 at 40, 5.12 vs 5.36 at 64), three at 12, 24 and 48 (1.27 vs 1.29, 2.11 vs 2.22, 3.91 vs 4.00 against two).  A fixed function
// of the batch size: the same call always runs the same plan, and nothing is timed inside a call.
static int dual_parts_static(int batch) {
    if (batch < 8) return 1;
    if (batch == 12 || batch == 24 || batch == 48) return 3;
    return 2;
}

int run_forward(ams_student* s, const void* frames, int dtype, int batch, int mode, hipStream_t st) {
    if (mode == AMS_MODE_FROZEN) {
        if (!s->frozen_ready) { set_error("predict: ams_student_freeze has not been called"); return AMS_E_STATE; }
        if (s->dual_stream == 0 || s->prof.on || s->late_subbatch != 0 || batch < 2) return forward_frozen_dual(s, frames, dtype, batch, st, 1);
        if (s->dual_stream >= 2) return forward_frozen_dual(s, frames, dtype, batch, st, batch >= s->dual_stream ? s->dual_parts : 1);
        if (!s->dual_autotune) return forward_frozen_dual(s, frames, dtype, batch, st, dual_parts_static(batch));
        if (batch < 16) return forward_frozen_dual(s, frames, dtype, batch, st, 1);
        auto it = s->dual_choice.find(batch);
        if (it == s->dual_choice.end()) {
            // AMS_OPT_DUAL_AUTOTUNE (opt-in; this branch synchronises the host): the first call with this batch size times the one-stream
            // plan and the 2- to 4-part plans on these very frames — median of three timed passes each, after a warm-up pass — keeps a
            // multi-part plan only when it wins by more than the timing noise, and finishes with a pass of the chosen plan
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            (void)hipStreamIsCapturing(st, &cap);
            if (cap != hipStreamCaptureStatusNone) return forward_frozen_dual(s, frames, dtype, batch, st, 1);      // no timing inside a capture
            hipEvent_t e0 = nullptr, e1 = nullptr;
            AMS_CHECK_HIP(hipEventCreate(&e0));
            if (hipEventCreate(&e1) != hipSuccess) { (void)hipEventDestroy(e0); set_error("autotune: hipEventCreate failed"); return AMS_E_HIP; }
            float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};          // ms[n]: the batch in n parts (n = 1: one stream)
            int rc = AMS_OK;
            hipError_t he = hipSuccess;
            const int max_parts = batch >= 32 ? 4 : batch >= 24 ? 3 : 2;       // parts of at least 8 frames
            for (int n = 1; n <= max_parts && !rc && he == hipSuccess; ++n) {
                float t[3] = {0.f, 0.f, 0.f};
                rc = forward_frozen_dual(s, frames, dtype, batch, st, n);      // warm-up
                for (int rep = 0; rep < 3 && !rc && he == hipSuccess; ++rep) {
                    he = hipEventRecord(e0, st);
                    rc = forward_frozen_dual(s, frames, dtype, batch, st, n);
                    if (he == hipSuccess) he = hipEventRecord(e1, st);
                    if (he == hipSuccess) he = hipEventSynchronize(e1);
                    if (he == hipSuccess) he = hipEventElapsedTime(&t[rep], e0, e1);
                }
                const float lo = t[0] < t[1] ? t[0] : t[1], hi = t[0] < t[1] ? t[1] : t[0];
                ms[n] = t[2] < lo ? lo : (t[2] > hi ? hi : t[2]);                                  // median of three
            }
            (void)hipEventDestroy(e0);
            (void)hipEventDestroy(e1);
            if (rc) return rc;
            if (he != hipSuccess) { set_error("autotune: event timing failed: %s", hipGetErrorString(he)); return AMS_E_HIP; }
            int best = 1;
            for (int n = 2; n <= max_parts; ++n)
                if (ms[n] < 0.985f * ms[1] && (best == 1 || ms[n] < ms[best])) best = n;
            it = s->dual_choice.emplace(batch, best).first;
        }
        return forward_frozen_dual(s, frames, dtype, batch, st, it->second);
    }
    if (mode == AMS_MODE_LIVE) return forward_live(s, frames, dtype, batch, batch, /*update_ema=*/false, nullptr, st);
    set_error("predict: unknown mode %d", mode);
    return AMS_E_INVALID;
}

}  // namespace ams
