// Launcher prototypes shared by the engine (engine.hip) and the kernel-level C ABI (api.hip).
#pragma once
#include <vector>

#include "common.hpp"

struct ams_comm;

namespace ams {

// block_call.hpp: a frozen conv layer and a frozen block as the host describes them, and block_call_check, which every launcher that takes
// a BlockCall goes through first (one order of refusal)
struct ConvLayer;
struct BlockCall;

// ---- runtime.hip : per-device launch bookkeeping, environment knobs (read once) --------------------------
// allow `lds` bytes of dynamic LDS for kernel `fn` on the CURRENT device (no-op up to 64 KB; set once per device and size)
int func_allow_lds(const void* fn, size_t lds);
// resident blocks per CU of `fn` on the current device (cached per device / block size / LDS)
int func_blocks_per_cu(const void* fn, int threads, size_t lds, int* per_cu);
int device_cus(int* cus);
// pure bookkeeping behind func_allow_lds (CPU-testable): true the first time (device, kernel) needs a limit >= lds
bool launch_table_needs_attr(int device, const void* fn, size_t lds);
struct Knobs {                   // tuning knobs of tools/*: environment variables, read at first use, never on the launch path
    int blk_th = 0, blk_tw = 0;                  // AMS_BLK_TILE=<th>x<tw>
    int fb_walk = -1;                            // AMS_FB_WALK=<0|-2|n>: first block of the frozen path as one tile per block (0) / only the border tiles so (-2) / at most n tiles per walking block
    int fb_abl = 0;                              // AMS_FB_ABL=<bits>: measurement-only ablations of the walking first block (wrong results)
    int xwr_timed = 0;                           // AMS_XWR_TIMED=1: xdw_wreg_kernel sums per-role cycles (ams_debug_phase_cycles(2, ..))
    int blk_timed = 0;                           // AMS_BLK_TIMED=1: block_kernel sums per-phase cycles (ams_debug_phase_cycles)
    int blk_hp = -1;                             // AMS_BLK_HP=<0|1>: fp16 whole-block kernels with exact-f32 (0) / fp16 (1) project products
    char pw_force = 0; int pw_rm = 0, pw_nt = 0; // AMS_PW_FORCE=<s|l>,<RM>,<NT>
    int pw_percu = 0;                            // AMS_PW_PERCU
    bool pwx_no_tail = false;                    // AMS_PWX_NO_TAIL
    int pwx_rm = 0, pwx_nt = 0;                  // AMS_PWX_FORCE=<RM>,<NT>
    int xwr_abl = 0;                             // AMS_XWR_ABL=<bits>: the same for the weight-register streaming kernel
    int pwh_abl = 0;                             // AMS_PWH_ABL=<bits>: measurement-only ablations of the fp16 GEMM's stage loop (wrong results)
    bool pwh_set = false; int pwh_nw = 4, pwh_d = 2;                   // AMS_PWH_VARIANT=<waves per block>,<operand stages in flight>: experiment switch of the fp16 GEMM
    bool xds_set = false; int xds[6] = {0, 0, 0, 0, 0, 0};      // AMS_XDS_FORCE
    bool xwr_set = false; int xwr[5] = {0, 0, 0, 0, 0};         // AMS_XWR_FORCE
    bool wg6_eight_waves = false;                // AMS_WG6_EIGHT_WAVES: the wide tiles of the six-product weight gradient with eight waves, split 4 (k) x 2 (n)
    int wg6_split_cap = 0;                       // AMS_WG6_SPLITS: most pixel splits of the six-product weight gradient (default 32)
    int event_flags = -1;                        // AMS_EVENT_FLAGS=<hex>: flags of the stream-ordering events (default: hipEventDisableTiming)
    unsigned side_cu_mask = 0;                   // AMS_SIDE_CU_MASK=<hex word>: the fine-tune step's side stream only on the CUs whose bit is set (word repeated over the chip)
};
const Knobs& knobs();
int blk_phase_cycles(unsigned long long* h);      // k_block.hip (tools/ only)
int xwr_phase_cycles(unsigned long long* h);      // k_xdw_wreg.hip (tools/ only)
int xds_phase_cycles(unsigned long long* h);      // k_xdw_stream.hip (tools/ only)
int create_side_stream(hipStream_t* out);        // non-blocking stream for the weight gradients (runtime.hip)
int create_sync_event(hipEvent_t* out);          // event that orders streams of ONE device (runtime.hip)

// ---- comm.hip : RCCL communicator (resolved at run time) ------------------------------------------------
int comm_allreduce(ams_comm* c, void* p, size_t n, int dtype, hipStream_t st);

// ---- k_pointwise.hip : 1x1 convolutions as f32-MFMA GEMMs ---------------------------------------------
struct PwArgs {
    const float* x;        // [M, ldx]
    int64_t M;
    int K;                 // contraction length (multiple of 4)
    int Kw;                // rows of w that exist (<= K); x columns in [Kw, K) must hold finite values (they meet zeros)
    int ldx;               // row stride of x in floats (multiple of 4)
    const float* w;        // element (k, n) at w[k*w_sk + n*w_sn]
    int64_t w_sk, w_sn;
    int N;
    const float* img_bias; // [M/rows_per_img, N] added before scale/shift, or nullptr
    int64_t rows_per_img;
    const float* scale;    // [N] or nullptr
    const float* shift;    // [N] or nullptr (bias when scale == nullptr)
    int act;
    const float* res;      // [M, ldr] added after the activation, or nullptr
    int ldr;
    float* y;              // [M, ldy]
    int ldy;
    // optional second form of the result (split-bf16 kernel, vector epilogues only): bf16 parts [part][M][N], part p at
    // ysplit + p * ysplit_plane, ysplit_np = 2 | 3 parts — the operand format of the next block's expand GEMM
    uint16_t* ysplit;
    int64_t ysplit_plane;
    int ysplit_np;
    int ysplit_fmt;        // 0: bf16 parts; 1: two fp16 parts (hi | lo 2^11; ysplit_np = 2), the operand format of the fp16 streaming kernels
    int y_skip_f32;        // with ysplit, vector epilogues: the part planes are the ONLY form of the result — y is not written (nothing may read it)
    // operand storage (launch_pointwise_split_f16 only): 0 = f32; 1 = "H2I", fp16 (hi | lo 2^11) pairs interleaved per 8 channels — 16 bytes
    // of hi, 16 bytes of lo — at the same 4 K bytes per row as f32 (requires ldx == K)
    int x_fmt;
    // optional column reduction fused into the epilogue (fine-tune step; plain epilogues only: no scale / shift / bias; a residual
    // operand only in mode 2 of the tiled split-bf16 kernel, where it joins the product before the mask and the sums):
    //   red_mode 1  forward BN statistics of y:  sum(y - red_center), sum((y - red_center)^2)
    //   red_mode 2  y is the gradient wrt the ACTIVATED output of a BN layer whose raw output is red_z [M, ldy]: y is multiplied by the
    //               activation's derivative act'(red_z red_scale + red_shift) before it is stored, and sum(y), sum(y xhat) are formed
    //               (xhat = (red_z - red_mean) red_rstd): the first half of that layer's BN backward
    // partial rows [rows][2][N] go to red_part, the row count to *red_rows_out (HOST pointer; 0 = the kernel chosen cannot fuse: the caller
    // runs the separate reduction)
    int red_mode;
    const float* red_center;
    const float* red_z; const float* red_scale; const float* red_shift; const float* red_mean; const float* red_rstd;
    int red_act;
    float* red_part;
    size_t red_part_floats;    // capacity of red_part: a launch whose partial rows would not fit runs WITHOUT the fused reduction (*red_rows_out = 0)
    int* red_rows_out;
    // set by the split-bf16 launcher only (mode 2 with a residual operand: the residual moves here and the plain epilogue runs)
    const float* red_res; int red_ldr;
    // optional per-element transform of the OPERAND x as it is loaded (fine-tune step: the elementwise BN passes between two layers
    // disappear into the consumer; same IEEE operations in the same order as the pass it replaces, so the product is bit-identical):
    //   x_mode 1  x' = act(x * x_v0[k] + x_v1[k])                    BN + activation of the layer that produced x (bn_act_kernel)
    //   x_mode 2  x' = x_v0[k] * x + x_v1[k] + x_v2[k] * x2[m, k]    second half of BN backward: x = gradient wrt the BN output, x2 = the
    //                                                                 layer's raw output z [M, ldx], (x_v0, x_v1, x_v2) = (A, B, C) (bn_bwd_apply_kernel, act none)
    // A kernel that cannot apply the transform materialises x' into x_tmp [M, K] (dense) first and runs on that; without x_tmp it fails.
    int x_mode; int x_act;
    const float* x_v0; const float* x_v1; const float* x_v2; const float* x2;
    float* x_tmp;
};
// dense [M][K] x [K][N] -> [M][ldy], no epilogue: the starting point of every PwArgs
static inline PwArgs pw_args(const float* x, int64_t M, int K, int ldx, const float* w, int N, float* y, int ldy) {
    PwArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.M = M; a.K = K; a.Kw = K; a.ldx = ldx; a.w = w; a.w_sk = N; a.w_sn = 1; a.N = N;
    a.rows_per_img = 1; a.act = AMS_ACT_NONE; a.y = y; a.ldy = ldy;
    return a;
}
int launch_pointwise(const PwArgs& a, hipStream_t st);
// x' of PwArgs::x_mode written to a.x_tmp by the elementwise kernels the transform replaces; on return *b is `a` without the transform
int pointwise_materialize_x(const PwArgs& a, PwArgs* b, hipStream_t st);
bool pointwise_stream_applies(const PwArgs& a);     // the persistent streaming variant (small K x N) can take this problem
bool pointwise_transforms_on_load(const PwArgs& a);         // launch_pointwise applies a.x_mode on the operand loads (no x_tmp pass)
bool pointwise_split3_transforms_on_load(const PwArgs& a);  // the same for launch_pointwise_split3

// split-bf16 (hi + lo) late-layer variant: weights pre-split into [N][Kp] bf16 panels, Kp = K rounded up to 32
int launch_split_weights(const float* w, int64_t sk, int64_t sn, int K, int N, int Kp, uint16_t* hi, uint16_t* lo, hipStream_t st);
int launch_pointwise_split(const PwArgs& a, const uint16_t* whi, const uint16_t* wlo, int Kp, hipStream_t st);
int launch_split_weights3(const float* w, int64_t sk, int64_t sn, int K, int N, int Kp, uint16_t* hi, uint16_t* mid, uint16_t* lo,
                          hipStream_t st);
int launch_pointwise_split3(const PwArgs& a, const uint16_t* whi, const uint16_t* wmid, const uint16_t* wlo, int Kp, hipStream_t st);
// all live weight panels of a student in one launch (three-part split): job j splits w (element (k, n) at w[k*sk + n*sn]) into
// p0 | p0 + plane | p0 + 2*plane as [N][Kp]; it owns the 256-thread blocks [first_block, first_block + ceil(N*Kp / 256))
// f16 != 0: the job ALSO leaves the two fp16 parts (hi | lo 2^11) at p0 + 3 * plane | p0 + 4 * plane (forward orientation: the fine-tune
// step's forward products run on them under AMS_MATMUL_SPLIT_F16)
struct SplitJob { const float* w; int64_t sk, sn; int K, N, Kp; uint16_t* p0; int64_t plane; int64_t first_block; int f16; };
int launch_split_batch(const SplitJob* jobs_dev, int njobs, int64_t total_blocks, hipStream_t st, int write_f16);
int launch_pointwise_split1(const PwArgs& a, const uint16_t* whi, int Kp, hipStream_t st);      // one part: plain bf16 products
// two fp16 parts (k_pw_f16.hip; AMS_MATMUL_SPLIT_F16): panels [part][N][Kp] fp16, hi at whi, lo 2^11 at whi + plane; 3 MFMAs per 32 k
int launch_split_weights_f16(const float* w, int64_t sk, int64_t sn, int K, int N, int Kp, uint16_t* hi, uint16_t* lo, hipStream_t st);
bool pointwise_f16_applies(const PwArgs& a);
int launch_pointwise_split_f16(const PwArgs& a, const uint16_t* whi, int64_t plane, int Kp, hipStream_t st);
int launch_pack_h2i(const float* x, int64_t M, int C, float* out, hipStream_t st);      // f32 [M][C] -> H2I (PwArgs::x_fmt 1)
bool pointwise_split_writes_parts(const PwArgs& a);      // the split kernels will honour a.ysplit (vector epilogue)
// the frozen head's three GEMMs (aspp0 -> concat_projection + per-image bias -> logits) as one kernel on the same fp16 panels, bit-identical to
// the three launch_pointwise_split_f16 calls it replaces (k_head_chain.hip); y [M][32], NC <= 32 columns written
bool head_chain_supported(int KA, int NA, int KB, int NB, int KC, int NC);
// A, B, C: the layers' fp16 panels, planes, BN vectors (C: shift = its bias, no scale) and activations
int launch_head_chain(const float* x, int64_t M, int KA, const ConvLayer& A, const ConvLayer& B, const ConvLayer& C, const float* img_bias,
                      int64_t rows_per_img, int NC, float* y, hipStream_t st);

// dw[K,N] = x[M,K]^T @ dy[M,N];  scratch holds the per-split partial products.
struct WgArgs {
    const float* x;  int ldx;  int K;
    const float* dy; int ldy;  int N;
    int64_t M;
    float* dw;             // [K, N] dense
    float* scratch; size_t scratch_floats;
    int allow_split;       // != 0: layers where the f32 MFMA kernel is matrix-pipe bound may use the 3-part bf16 kernel
    // operand transforms on load (see PwArgs::x_mode; both wgrad kernels apply them, nothing is materialised):
    //   x_mode 1   x'  = act(x * x_v0[k] + x_v1[k])
    //   dy_mode 2  dy' = dy_v0[n] * dy + dy_v1[n] + dy_v2[n] * dy2[m, n]      (dy2 [M, ldy])
    int x_mode = 0, x_act = 0; const float* x_v0 = nullptr; const float* x_v1 = nullptr;
    int dy_mode = 0; const float* dy_v0 = nullptr; const float* dy_v1 = nullptr; const float* dy_v2 = nullptr; const float* dy2 = nullptr;
};
// fused depthwise 3x3 (+BN+act) -> project 1x1 (+BN, +residual), frozen inference, split-bf16 GEMM (k_dw_project.hip)
bool dw_project_supported(int C, int N, int stride, int rate);
// c.x: the expanded tensor [B][H][W][Cexp]; the project layer's two-part bf16 panels [Cout][Cexp]; c.res with c.residual
int launch_dw_project(const BlockCall& c, hipStream_t st);
bool pointwise_wgrad_x6_applies(int64_t M, int K, int N, int ldx, int ldy);
int wgrad_x6_splits(int64_t M, int K, int N);
int wgrad_f32_splits(int64_t M, int K, int N);             // the exact-f32 kernel's row splits (K, N > 0)
int launch_pointwise_wgrad_x6(const WgArgs& a, int splits, hipStream_t st);
size_t pointwise_wgrad_scratch(int64_t M, int K, int N);
int launch_pointwise_wgrad(const WgArgs& a, hipStream_t st);

// ---- k_first_block.hip : stem + depthwise + project of the first block in one kernel (frozen inference; 3 -> 32 -> 32 -> 16)
// What launch_first_block launches for a batch (ams_first_block_plan of include/ams_hip.h is this, field by field): the output grid and its
// 8 x 16 tiles, the rectangle of interior tiles, and the tiles and blocks of the two launches.  interior_tiles = 0: the walking form does not
// run, and the border launch is the one-tile kernel over every tile.
struct FirstBlockPlan {
    int Ho, Wo, pt, pl;                     // stem output size and its SAME padding on the 127.5-padded frame
    int tiles_y, tiles_x;
    int ity0, itx0, niy, nix;               // interior tiles [ity0, ity0 + niy) x [itx0, itx0 + nix); niy * nix = 0: none
    int interior_tiles, interior_grid;      // first_block_walk_kernel<0>: tiles over the batch, blocks
    int border_tiles, border_grid;          // every other tile: tiles over the batch, blocks
    int border_walks;                       // 1: the border launch is first_block_walk_kernel<0, true>, 0: first_block_kernel (a tile per block)
};
// occupancy: null = ask the device (blocks per CU of the two walking kernels, CUs); else {interior blocks per CU, border blocks per CU, CUs}:
// pure host arithmetic, no device call
int first_block_plan(int dtype, int B, int H, int W, bool h16, const int* occupancy, FirstBlockPlan* plan);
int launch_first_block(const BlockCall& c, hipStream_t st, FirstBlockPlan* plan_out = nullptr);
// c.expand = the stem.  Panels of the stem and the project layer as fp16 parts (hi | lo 2^11; [part][32][32] and [part][16][32]): the stem's and
// the project layer's products run as 3 fp16 MFMAs each (AMS_MATMUL_SPLIT_F16)
// three-part bf16 panels [part][32][32] of the stem alone (k = tap * 3 + channel, zero-padded 27 -> 32): with them and uint8 frames the
// stem's products run as six bf16 MFMAs, operands from a 258-entry table of the normalised byte values (f32-level)

// ---- k_ingest.hip : frame / label resize on the device (run.py:179-183)
int launch_resize_u8(const uint8_t* src, int Hs, int Ws, int C, int mode, int swap_rb, uint8_t* dst, int H, int W, hipStream_t st);

// ---- k_conv.hip : stem and depthwise ------------------------------------------------------------------
int launch_stem(const void* frames, int dtype, int B, int H, int W, const float* w, int cout, const float* scale,
                const float* shift, int act, float pixel_scale, float* y, hipStream_t st);
// im2col of the normalised, padded frame for the stem's weight gradient: out [B*Ho*Wo, 32] (27 taps + 5 zeros)
int launch_stem_im2col(const void* frames, int dtype, int B, int H, int W, float pixel_scale, float* out, hipStream_t st);
int launch_depthwise(const float* x, int B, int H, int W, int C, const float* w, int stride, int rate,
                     const float* scale, const float* shift, int act, float* y, hipStream_t st);
int launch_depthwise_dgrad(const float* dy, int B, int H, int W, int C, const float* w, int stride, int rate,
                           float* dx, hipStream_t st);
// stride-1 input gradient fused with the mask and the BN-backward sums of the layer in front (see k_conv.hip); C <= 1024
// training forward of the same layers: BN + activation of the layer in front on the tap loads, BN statistics of the result as partial rows
size_t depthwise_fwd_bn_scratch(int B, int H, int W, int C, int rate);
int launch_depthwise_fwd_bn(const float* ze, int B, int H, int W, int C, const float* w, int rate, const float* scale, const float* shift, int act,
                            const float* center, float* zd, float* scratch, int* rows_out, hipStream_t st);
size_t depthwise_dgrad_bn_scratch(int B, int H, int W, int C);
int launch_depthwise_dgrad_bn(const float* dy, int B, int H, int W, int C, const float* w, int rate, const float* z, const float* scale,
                              const float* shift, int act, const float* mean, const float* rstd, float* out, float* scratch, int* rows_out,
                              hipStream_t st);
// k_dw_train.hip: the same with the depthwise layer's own BN-backward apply pass folded in — dz_d = cA dy + cB + cC zd is formed once per
// element on the way into an LDS ring (bit-identical to bn_bwd_apply_kernel followed by the kernel above; partial rows in a different split)
size_t depthwise_dgrad_bn2_scratch(int B, int H, int W, int C, int rate);
int launch_depthwise_dgrad_bn2(const float* dy, const float* zd, const float* cA, const float* cB, const float* cC, int B, int H, int W, int C,
                               const float* w, int rate, const float* ze, const float* scale, const float* shift, int act, const float* mean,
                               const float* rstd, float* out, float* scratch, int* rows_out, hipStream_t st);
// ... and the training forward in the same tile form (a_e formed once per element on its way into LDS; z_d bit-identical to launch_depthwise_fwd_bn)
size_t depthwise_fwd_bn2_scratch(int B, int H, int W, int C, int rate);
int launch_depthwise_fwd_bn2(const float* ze, int B, int H, int W, int C, const float* w, int rate, const float* scale, const float* shift, int act,
                             const float* center, float* zd, float* scratch, int* rows_out, hipStream_t st);
size_t depthwise_wgrad_scratch(int B, int H, int W, int C, int stride, int rate);
int launch_depthwise_wgrad(const float* x, const float* dy, int B, int H, int W, int C, int stride, int rate,
                           float* dw, float* scratch, size_t scratch_floats, hipStream_t st);

// ---- k_expand_dw.hip : fused expand (1x1+BN+ReLU6) -> depthwise 3x3 (+BN+ReLU6), frozen inference ------------
bool expand_dw_supported(int Cin, int Cexp, int stride, int rate);
// stats_part != nullptr (fine-tune forward; c.dw's scale / shift / act then describe what is WRITTEN, normally the identity): partial rows
// [*stats_rows][2][Cexp] of sum(y - center), sum((y - center)^2) of the written values, expand_dw_stats_scratch floats
size_t expand_dw_stats_scratch(int B, int H, int W, int Cexp, int stride);
int launch_expand_dw(const BlockCall& c, hipStream_t st, const float* stats_center = nullptr, float* stats_part = nullptr, int* stats_rows = nullptr);

// ---- k_xdw_train.hip : fine-tune step of the early blocks (Cin <= 32) without the 6x-expanded tensors: every consumer recomputes
// z_e = x . W_e from the block input (see the file header)
bool xdw_train_supported(int Cin, int Cexp, int stride, int rate);
size_t xdw_train_scratch(int B, int H, int W, int Cin, int Cexp);      // floats: partial rows of the passes below + one reduced row
int xdw_train_blocks(int B, int H, int W, int Cexp);
// forward statistics: partial rows  S [2][Cexp] (sum(z - center), sum((z - center)^2)) | XX [KP][KP] = x^T x | g0 [KP] = sum x
// (KP = Cin rounded up to 16) -> scratch
int launch_xdw_fwd_stats(const float* x, int B, int H, int W, int Cin, const float* w_exp, int Cexp, const float* center, float* scratch,
                         int* rows_out, int64_t* stride_out, hipStream_t st);
// backward pass 1 (given dz_d): partial rows  S [2][Cexp] | dWd [9][Cexp] | G1 [KP][Cexp]
int launch_xdw_bwd_reduce(const float* x, int B, int H, int W, int Cin, const float* w_exp, int Cexp, const float* sc_e, const float* sh_e,
                          const float* mean_e, const float* rstd_e, int act_e, const float* w_dw, int stride, const float* dz_d, float* scratch,
                          int* rows_out, int64_t* stride_out, hipStream_t st);
// first block: stem conv (as a 1x1 conv over its 27-tap patch of the frame) + first depthwise conv; partial rows
// S [2][32] | dWd [9][32] | G1 [32][32] | XX [32][32] | g0 [32]
size_t xdw_stem_scratch(int B, int fH, int fW);
int launch_xdw_bwd_reduce_stem(const void* frames, int dtype, int B, int fH, int fW, float pixel_scale, const float* w_stem, const float* sc_e,
                               const float* sh_e, const float* mean_e, const float* rstd_e, int act_e, const float* w_dw, const float* dz_d,
                               float* scratch, int* rows_out, int64_t* stride_out, hipStream_t st);
// backward pass 2: dx = (cA dy_e + cB + cC z_e) . W_e^T (+ res)
int launch_xdw_bwd_dx(const float* x, int B, int H, int W, int Cin, const float* w_exp, int Cexp, const float* sc_e, const float* sh_e,
                      int act_e, const float* w_dw, int stride, const float* dz_d, const float* cA, const float* cB, const float* cC,
                      const float* res, float* dx, hipStream_t st, const float* red_z = nullptr, const float* red_mean = nullptr,
                      const float* red_rstd = nullptr, float* red_part = nullptr, int* red_rows_out = nullptr);
// dW_e from the reduced G1 [KP][Cexp], the forward pass's (XX | g0) and the BN-backward coefficients
int launch_xdw_dwe(const float* G1, const float* xx_g0, int Cin, int Cexp, const float* w_exp, const float* cA, const float* cB, const float* cC,
                   float* dw, hipStream_t st);

// ---- k_xx_stats.hip : BN statistics of an early block's expand layer from the Gram matrix of the block input (f64 matrix pipe)
int xx_stats_blocks(int64_t M);
size_t xx_stats_scratch_doubles(int64_t M, int Cin);
int launch_xx_gram(const float* x, int64_t M, int Cin, double* scratch, double* xx64, float* xx32, hipStream_t st);
int launch_expand_stats(const double* xx64, int Cin, const float* w_exp, int Cexp, double n, const float* center, const float* gamma,
                        const float* beta, float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale, float* shift,
                        float* save_mean, float* save_rstd, double* sums, hipStream_t st);

// ---- k_block.hip : a whole early inverted-residual block (expand -> depthwise -> project [+ input]) in one kernel ----
bool block_fused_supported(int Cin, int Cexp, int Cout, int stride, int rate, bool residual);
int launch_block_fused(const BlockCall& c, hipStream_t st);
// fp16 panels (hi | lo 2^11) of the expand layer [part][Cexp][32] and the project layer [part][Cout][Kp]: the expand and the project
// products run as 3 fp16 MFMAs each (AMS_MATMUL_SPLIT_F16)
// three-part bf16 panels [part][Cexp][32] of the expand layer alone: the expand products of a block with Cin 24 / 32 run as six bf16 MFMAs
// (f32-level) instead of eight exact-f32 MFMAs
// c.vecs: optional [13][Cexp] table (sc_e | sh_e | sc_d | sh_d | w_dw[9]) built once by launch_block_pack (the engine: at freeze)
int launch_first_block_tiles(const BlockCall& c, hipStream_t st);
int launch_block_pack(const float* sc_e, const float* sh_e, const float* sc_d, const float* sh_d, const float* w_dw, int Cexp, float* out, hipStream_t st);

constexpr int AMS_NP_F16 = 4;   // ConvLayer::np: the two fp16 parts of split_bf16.hpp
// ---- k_xdw_stream.hip : the same fusion for the stride-16 blocks (Cin 64 / 96 / 160, stride 1, rate 1 | 2): raster-order
// streaming through an LDS ring, split-bf16 products from the expand layer's bf16 panels (np = 2 | 3 parts, `plane` apart)
bool expand_dw_stream_supported(int Cin, int Cexp, int stride, int rate);
int launch_expand_dw_stream(const BlockCall& c, hipStream_t st);

// ---- k_xdw_wreg.hip : the streaming fusion with the expand weights in registers and the operand staged in LDS (160 -> 960)
int launch_expand_dw_wreg(const BlockCall& c, hipStream_t st);
// The geometry the two streaming launchers pick for a call (AMS_XDS_FORCE / AMS_XWR_FORCE honoured) — the launchers take it from these
// functions, and so does expand_dw_steps: step = pixels per step, items = work items per chunk / channel group (cgroups of them), groups =
// blocks per chunk.  np: parts as staged (0: the exact-f32 form, 2 for the fp16 form).  false: nothing fits LDS.
struct XdwGeom { int step, SH, SW, Wp, T, ring, nsy, nsx, cgroups, items, groups, nt, nwe, nwd, nrg; size_t lds; };
bool expand_dw_stream_geom(int B, int H, int W, int Cin, int Cexp, int rate, int np, XdwGeom* g);
bool expand_dw_wreg_geom(int B, int H, int W, int Cin, int Cexp, int rate, int np, XdwGeom* g);
// The steps of every item of such a launch by the rule of xdw_steps.hpp (what the kernels' step loops execute), no GPU call.  out[0 .. 9]: step,
// Wp, SH, T, items; summed over the items: steps executed, E compute steps, E zero steps, active D-steps, steps (loop index) with an E compute and
// an active D-step.  n >= 10 + 5 * items: then per item T_item and its four counts; n >= 10 + (5 + T) * items: then per item and step t < T the
// code E class (0 idle, 1 zero, 2 compute) + 4 * (D-step active) + 8 * (t < T_item).  H x W: the input (rate 1 | 2, stride 1 or 2).
void expand_dw_steps(const XdwGeom& g, int H, int W, int rate, int32_t* out, size_t n);
// c.expand.np of the two streaming launchers: 1 .. 3 bf16 parts, or AMS_NP_F16 = the two fp16 parts of split_bf16.hpp (hi | lo 2^11; planes as
// for np = 2).  c.y_fmt 1 (fp16 form only): the result as fp16 pairs interleaved per 8 channels (PwArgs::x_fmt 1) instead of f32


// ---- k_elementwise.hip : BN pieces, pooling, reductions, Adam ------------------------------------------
// per-image column reductions; scratch >= image_colsum_scratch(B, C) floats
size_t image_colsum_scratch(int B, int C);
int launch_global_mean(const float* x, int B, int64_t HW, int C, float* y, float* scratch, hipStream_t st);
// column sums per image: out[b, c] = sum_hw x[b, hw, c]
int launch_image_colsum(const float* x, int B, int64_t HW, int C, int ldx, float* out, float* scratch, hipStream_t st);

// per-channel shifted sums over rows: sums[0][c] = sum(z - center[c]), sums[1][c] = sum((z-center[c])^2)  (f64)
size_t colstats_scratch(int64_t M, int C);
size_t colsum_scratch(int C);           // launch_colsum's scratch, floats
// the geometry the column reductions launch with: out = {CG, slots, chunks, rows_per_chunk}
int col_plan(int64_t rows_per_group, int groups, int C, int32_t out[4]);
int launch_colstats(const float* z, int64_t M, int C, const float* center, double* sums /*[2][C]*/, float* scratch,
                    hipStream_t st);
// ... formed in f64 throughout by one thread per channel: for layers of a few rows whose variance is small against the centre's distance
int launch_colstats_f64(const float* z, int64_t M, int C, const float* center, double* sums /*[2][C]*/, hipStream_t st);
// BN forward coefficients from the sums; updates the moving statistics when moving_mean != nullptr.
//   scale = gamma*rstd, shift = beta - mean*scale; save_mean, save_rstd for the backward pass.
int launch_bn_finalize(const double* sums, double n, int C, const float* center, const float* gamma, const float* beta,
                       float eps, float one_minus_decay, float* moving_mean, float* moving_var, float* scale,
                       float* shift, float* save_mean, float* save_rstd, hipStream_t st);
// frozen coefficients: scale = gamma*rsqrt(var+eps), shift = beta - mean*scale
int launch_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int C,
                   float* scale, float* shift, hipStream_t st);
// a = act(z*scale + shift) (+ res)
int launch_bn_act(const float* z, int64_t M, int C, const float* scale, const float* shift, int act, const float* res,
                  float* a, hipStream_t st);
// backward reductions: sums[0][c] = sum(dy), sums[1][c] = sum(dy * xhat), dy = da * act'(z*scale+shift)
int launch_bn_bwd_reduce(const float* da, const float* z, int64_t M, int C, const float* scale, const float* shift,
                         int act, const float* mean, const float* rstd, double* sums, float* scratch, hipStream_t st);
// per-channel (A,B,C) with dz = A*dy + B + C*z; also writes dgamma, dbeta
int launch_bn_bwd_coef(const double* sums, double n, int C, const float* gamma, const float* mean, const float* rstd,
                       float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, hipStream_t st);
int launch_bn_param_grads(const double* sums, int C, float* dgamma, float* dbeta, hipStream_t st);
// single-GPU fusions of the above: the second reduction stage also does the per-channel arithmetic
int launch_colstats_bn(const float* z, int64_t M, int C, const float* center, double* sums, float* scratch, double n,
                       const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean,
                       float* moving_var, float* scale, float* shift, float* save_mean, float* save_rstd, hipStream_t st);
int launch_bn_bwd_reduce_coef(const float* da, const float* z, int64_t M, int C, const float* scale, const float* shift, int act,
                              const float* mean, const float* rstd, double* sums, float* scratch, double n, const float* gamma,
                              float* coefA, float* coefB, float* coefC, float* dgamma, float* dbeta, hipStream_t st);
int launch_bn_bwd_apply(const float* da, const float* z, int64_t M, int C, const float* scale, const float* shift, int act,
                        const float* coefA, const float* coefB, const float* coefC, float* dz, hipStream_t st);
// plain column sums over rows (bias gradient): out[c] = sum_m x[m, c]
int launch_colsum(const float* x, int64_t M, int C, int ldx, float* out, float* scratch, hipStream_t st);
int launch_adam(float* p, const float* g, float* m, float* v, const uint8_t* mask, int64_t n, float lr_t, float b1,
                float b2, float eps, hipStream_t st);
// out[i] = sum_k part[k*n + i], k ascending (deterministic second stage of split reductions)
// stride: floats between the partial rows (0 = n: dense)
// up to 32 split reductions in one launch: out[j][i] = sum_k part[j][k * stride[j] + i], i < count[j], k < splits[j]
struct ReduceJobs {
    static constexpr int kMax = 32;
    int n = 0;
    const float* part[kMax]; float* out[kMax]; int splits[kMax]; int64_t count[kMax]; int64_t stride[kMax]; int first_block[kMax];
    bool add(const float* p, int splits_, int64_t count_, float* o, int64_t stride_) {
        if (n >= kMax) return false;
        part[n] = p; splits[n] = splits_; count[n] = count_; out[n] = o; stride[n] = stride_ > 0 ? stride_ : count_; ++n;
        return true;
    }
};
int launch_reduce_batch(ReduceJobs& jobs, hipStream_t st);
int launch_reduce_splits(const float* part, int splits, int64_t n, float* out, hipStream_t st, int64_t stride = 0);
// the second (per-channel) stages of the BN reductions over partial rows [rows][2][C] produced elsewhere, row_stride floats apart
int launch_bn_fwd_finalize_partials(const float* part, int rows, int64_t row_stride, int C, double* sums, double n, const float* center,
                                    const float* gamma, const float* beta, float eps, float one_minus_decay, float* moving_mean,
                                    float* moving_var, float* scale, float* shift, float* save_mean, float* save_rstd, hipStream_t st);
int launch_bn_bwd_finalize_partials(const float* part, int rows, int64_t row_stride, int C, double* sums, double n, const float* gamma,
                                    const float* mean, const float* rstd, float* coefA, float* coefB, float* coefC, float* dgamma,
                                    float* dbeta, hipStream_t st);
int launch_partials_to_sums(const float* part, int rows, int64_t row_stride, int C, double* sums, hipStream_t st);
int launch_fill(float* p, int64_t n, float v, hipStream_t st);
int launch_round_bf16(float* p, int64_t n, hipStream_t st);       // x <- float(bf16(x)) in place (bf16-storage study)
int launch_copy(float* dst, const float* src, int64_t n, hipStream_t st);
size_t pack_fp16_scratch(int64_t n);
int launch_pack_fp16(const float* p, const uint8_t* mask, int64_t n, uint16_t* out, int64_t* n_out, int64_t* counts, hipStream_t st);
// k_delta.hip: the downlink delta decoded into params / stats (ams_student_apply_delta)
int64_t delta_segments(int64_t mask_bytes);
int launch_apply_delta(const uint8_t* payload, int64_t payload_bytes, const ams_delta_var* vars_dev, int n_vars, int64_t mask_bytes,
                       float* params, int64_t n_params, float* stats, int64_t n_stats, int64_t* counts, int64_t* n_applied, int32_t* status,
                       hipStream_t st);
int launch_delta_count(const uint8_t* payload, int64_t readable, int nseg, int64_t* counts, hipStream_t st);
// k_delta_q8.hip: the same delta as int8 codes of (current - base) with one f32 scale per variable, encoded and decoded
// (ams_student_encode_delta_q8 / ams_student_apply_delta_q8).  Segments are delta_segments() on both sides.
// table_dev (int64): [descriptors: 4 per variable][element starts: n_vars + 1][per-variable maxima, uint32, zeroed by the table copy];
// work (int64): [payload size][segment counts -> offsets]
size_t q8_encode_table_words(int n_vars);
int launch_encode_delta_q8(const uint8_t* mask, int64_t* table_dev, int n_vars, int64_t mask_bytes, const float* params, const float* stats,
                           float* base_params, float* base_stats, int advance_base, int64_t* work, uint8_t* payload, int64_t cap,
                           int64_t* payload_bytes, int32_t* status, hipStream_t st);
int launch_apply_delta_q8(const uint8_t* payload, int64_t payload_bytes, const ams_delta_var* vars_dev, int n_vars, int64_t mask_bytes,
                          float* params, int64_t n_params, float* stats, int64_t n_stats, int64_t* counts, int64_t* n_applied, int32_t* status,
                          hipStream_t st);
// k_uplink.hip: the uplink frame codec AUC1 (ams_uplink_*).  Blocks and slices of the planes Y, Cb, Cr of an H x W frame; the scratch
// layouts are stated at the top of k_uplink.hip.  The launchers take sizes uplink_shape_ok accepts and 16-byte aligned scratch.
struct UplinkGeom { int H, W, nb[3], ns[3], nblocks, nslices; };
bool uplink_shape_ok(int H, int W);
UplinkGeom uplink_geom(int H, int W);
int64_t uplink_max_bytes(int H, int W);
size_t uplink_encode_scratch_bytes(int H, int W);
size_t uplink_decode_scratch_bytes(int H, int W);
int launch_uplink_transform(const uint8_t* frame, int H, int W, void* scratch, hipStream_t st);
int launch_uplink_size_table(void* scratch, int H, int W, int64_t* sizes, hipStream_t st);
int launch_uplink_encode(void* scratch, int H, int W, int q, uint8_t* payload, int64_t cap, int64_t* bytes_out, int32_t* status, hipStream_t st);
int launch_uplink_decode(const uint8_t* payload, int64_t bytes, int H, int W, uint8_t* frame, int32_t* status, void* scratch, hipStream_t st);

// k_uplink_inter.hip: the predicted frame AUP1 (ams_uplink_inter_*): one vector per macroblock against a reference frame of the same size,
// the residual through AUC1's transform and block code (uplink_common.hpp), motion slices in front of the residual slices.  Scratch layouts
// at the top of k_uplink_inter.hip.
int64_t uplink_inter_max_bytes(int H, int W);
size_t uplink_inter_encode_scratch_bytes(int H, int W);
size_t uplink_inter_decode_scratch_bytes(int H, int W);
int launch_uplink_inter_transform(const uint8_t* frame, const uint8_t* ref, int H, int W, void* scratch, hipStream_t st);
int launch_uplink_inter_size_table(void* scratch, int H, int W, int64_t* sizes, hipStream_t st);
int launch_uplink_inter_encode(void* scratch, int H, int W, int q, uint8_t* payload, int64_t cap, int64_t* bytes_out, int32_t* status, hipStream_t st);
int launch_uplink_inter_decode(const uint8_t* payload, int64_t bytes, const uint8_t* ref, int H, int W, uint8_t* frame, int32_t* status, void* scratch,
                               hipStream_t st);
// k_select.hip: the server half of a model update: coordinates chosen by their change, the roll-back, the downlink delta encoded
size_t select_scratch();
int launch_select_changed(const float* after, const float* before, int64_t n, int64_t k, ams_select_result* result, int64_t* scratch,
                          hipStream_t st);
int launch_select_apply(float* params, const float* before, int64_t n, float cut, uint8_t* mask, int64_t* n_kept, hipStream_t st);
int64_t encode_segments(int64_t mask_bytes);
int launch_encode_delta(const uint8_t* mask, const int64_t* table_dev, int n_vars, int64_t mask_bytes, const float* params, const float* stats,
                        int64_t* work, uint8_t* payload, int64_t cap, int64_t* payload_bytes, hipStream_t st);

// ---- k_head.hip : fused upsample + argmax + metrics, CE gradient, phi-score confusion --------------------
// what is computed on which tensors: HeadCall and LossObjective, head_common.hpp.  Every launcher below that takes a HeadCall goes through
// head_call_check first (one order of refusal), then its own conditions, then the null checks of what it reads
struct HeadCall;
struct LossObjective;
// per_frame != 0: conf [B][K][K] and loss [B][2] (one confusion matrix / loss pair per frame) instead of the batch totals
int launch_upsample_argmax(const HeadCall& c, int32_t* labels, int64_t* conf, double* loss, hipStream_t st, int per_frame = 0,
                           int labels_u8 = 0 /* labels as uint8 [B][H][W] through the same pointer */);
int launch_ce_grad(const HeadCall& c, const double* loss_and_count, float* dlogits, int ldd, hipStream_t st, float empty_val = 0.f);
// loss + gradient in one pass (fine-tune step): pass 1 leaves the CE sum / valid count in loss[2] and the unnormalised gradient in
// scratch (ce_loss_grad_scratch floats); pass 2 scales by 1 / count (after its cross-rank sum) and writes dlogits [B*h*w, ldd]
bool ce_loss_grad_supported(int w, int W);
size_t ce_loss_grad_scratch(int B, int h, int w, int K);
int launch_ce_loss_grad(const HeadCall& c, const LossObjective& o, double* loss, float* scratch, hipStream_t st);
// empty_val: every selected class's gradient when NO pixel of the (global) batch is valid: 0, or NaN = the reference's 0 / 0
// (utils/graph_utils.py:408: loss = sum(w ce) / sum(w))
int launch_ce_combine(const HeadCall& c, const double* loss_and_count, const float* scratch, float* dlogits, int ldd, hipStream_t st,
                      float empty_val = 0.f);
// freeze-time range check of the fp16 product form: over_host[j] = 1 when any |w| of job j is > limit or not finite, or when no |w| of job j
// reaches `low` (every weight so small that its fp16 parts are subnormal: split1_f16 keeps 22 bits only for normal parts).  Synchronises `st`.
struct WeightRange { const float* w; int64_t n; };
int weights_beyond(const std::vector<WeightRange>& jobs, float limit, float low, int* flags_dev /*>= jobs.size() ints + the job table*/, int* over_host,
                   hipStream_t st);
int launch_l2_regularizer(const float* p, float* g, const uint8_t* mask, int64_t n, int n_vars, float coef, double* part_scratch /*256 doubles*/,
                          double* loss, hipStream_t st);
int launch_cross_confusion(const uint8_t* a, const uint8_t* b, int64_t n, const int32_t* lut /*[256] -> subset idx or -1*/,
                           int K, int64_t* conf, hipStream_t st);

// ---- k_confidence.hip : the student's per-pixel certainty (max softmax) and its statistics, the same walk as upsample_argmax ----
// conf_u8 [B][H][W], conf_f32 [B][H][W], stats [B][confidence_stats_len()] (layout: include/ams_hip.h); each may be null
int confidence_stats_len();
int launch_upsample_confidence(const HeadCall& c, uint8_t* conf_u8, float* conf_f32, int64_t* stats, hipStream_t st);

// ---- k_soft_metric.hip : the soft-teacher loss and the probabilistic confusion matrices (prob_confmat, prob_confmat_star), the same walk ----
// c.teacher uint8 [B][H][W] or null (every pixel valid); of o, teacher_logits f32 [B][th][tw][NC] (th <= H, tw <= W; layout AMS_TLOGITS_SELECTED:
// [B][th][tw][K]); stats [B][soft_metric_stats_len(K)], p_f32 [B][H][W][K], ce_f32 [B][H][W] (layout: include/ams_hip.h); each output may be null
int soft_metric_stats_len(int K);
int launch_upsample_soft_metric(const HeadCall& c, const LossObjective& o, int64_t* stats, float* p_f32, float* ce_f32, hipStream_t st);

// ---- k_loss_mining.hip : hard-pixel mining for the fine-tune loss: the key map, the key of rank k from the top, the mined label map ----
// keys f32 [B][H][W], labels uint8 [B][H][W] (the mined map), hist: three histograms and the state words, result: 8-byte aligned; all on the device
struct MiningBuffers { float* keys = nullptr; uint8_t* labels = nullptr; uint32_t* hist = nullptr; ams_mining_result* result = nullptr; };
size_t loss_mining_scratch(int B, int H, int W);                        // bytes of a block that holds all four
MiningBuffers loss_mining_buffers(void* scratch, int B, int H, int W);  // the four inside such a block (16-byte aligned)
int mining_top_k_check(const char* who, float top_k);
// c.teacher: the labels the map is mined from; o: the objective whose per-pixel value is the key.  Steps 1 - 3 of a mined step (the fourth is
// launch_ce_loss_grad / launch_ce_combine on m.labels); the step's profiler times them one by one
int launch_mining_keys(const HeadCall& c, const LossObjective& o, float top_k, const MiningBuffers& m, hipStream_t st);
int launch_mining_select(int64_t n, float top_k, const MiningBuffers& m, hipStream_t st);
int launch_mining_relabel(const uint8_t* labels, int64_t n, const MiningBuffers& m, hipStream_t st);
int launch_loss_mining(const HeadCall& c, const LossObjective& o, float top_k, const MiningBuffers& m, hipStream_t st);

// ---- k_replay.hip : the replay memory on the device: a mini-batch in one launch, cached teacher logits, the phi-score pairs ----
// samples_host / pairs_host: the host copies of the device tables, checked before anything is launched
int launch_replay_gather(const uint8_t* frame_slots, int64_t frame_stride, const uint8_t* label_slots, int64_t label_stride, int capacity, int Hs,
                         int Ws, const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int B, int H, int W,
                         uint8_t* frames_out, uint8_t* labels_out, hipStream_t st);
int launch_replay_gather_rows(const float* slots, int64_t slot_stride, int capacity, int th, int tw, int C, const ams_replay_sample* samples_dev,
                              const ams_replay_sample* samples_host, int B, float* out, hipStream_t st);
int launch_replay_gather_logits(const float* slots, int64_t slot_stride, int capacity, int Hs, int Ws, int C, const ams_replay_sample* samples_dev,
                                const ams_replay_sample* samples_host, int B, int H, int W, float* out, hipStream_t st);
// slots f32 [lh][lw][C] with lh <= Hs, lw <= Ws: launch_replay_gather_logits' rule applied to the slot's align-corners upsample to Hs x Ws
int launch_replay_gather_logits_lowres(const float* slots, int64_t slot_stride, int capacity, int lh, int lw, int C, int Hs, int Ws,
                                       const ams_replay_sample* samples_dev, const ams_replay_sample* samples_host, int B, int H, int W, float* out,
                                       hipStream_t st);
// in f32 [th][tw][NC] -> out f32 [th][tw][K], out channel k = in channel idx_host[k] (the selected layout of a replay slot); idx_host: HOST pointer
int launch_replay_pack_logits(const float* in, int th, int tw, int NC, const int32_t* idx_host, int K, float* out, hipStream_t st);
// logits f32 [n][lh][lw][NC] (item stride in elements) -> out uint8 [n][Hs][Ws] (item stride in bytes): the argmax over every class, first
// maximum, of the items' align-corners upsample to Hs x Ws
int launch_teacher_labels_from_logits(const float* logits, int64_t slot_stride, int n, int lh, int lw, int NC, int Hs, int Ws, uint8_t* out,
                                      int64_t out_stride, hipStream_t st);
int launch_cross_confusion_pairs(const uint8_t* label_slots, int64_t label_stride, int capacity, int64_t n, const int32_t* pairs_dev,
                                 const int32_t* pairs_host, int n_pairs, const int32_t* lut /*[256] -> subset idx or -1*/, int K, int64_t* conf,
                                 hipStream_t st);

// ---- k_render.hip : the edge's pictures on the device: up to six RGB views of a batch in one launch ----
// student: uint8 or int32 [B,H,W] (AMS_DT_U8 / AMS_DT_I32); tables: the device block of AMS_RENDER_TABLE_BYTES; out: NULL = view not wanted
int launch_render_views(const uint8_t* frames, const void* student, int student_dtype, const uint8_t* teacher, int B, int H, int W, int K,
                        const uint8_t* tables, const ams_render_out* out, hipStream_t st);

}  // namespace ams
