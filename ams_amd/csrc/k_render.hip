// The edge's pictures on the device (reference SemanticNetwork.py:719-755 colorize / colorize_teacher / cross_ignore, run.py:441-454): up to
// six RGB uint8 planes [B, H, W, 3] of a batch in one launch, each equal to the host helper of ams_amd/semantic_network.py bit for bit.
//
//   render_views_kernel   per pixel: the student's colour (reduced palette), the teacher's colour (full palette), their 50/50 overlays on
//                         the frame, the ignore mask (white where take[teacher] == 0) and the disagreement mask (the teacher's reduced
//                         colour where not ignored and take[teacher] != student).  A view whose pointer is NULL costs nothing: the
//                         branch on it is uniform per launch and no store is issued.
//
// Integer arithmetic only.  The blend is _overlay's: t = f + c; h = t >> 1; h += (t & 1) & (h & 1)  (half to even, as cv2.addWeighted
// rounds the float sum).  The wide path forms it on four bytes of a word at once: floor((f + c) / 2) = (f & c) + (((f ^ c) >> 1) & 0x7f),
// t & 1 = (f ^ c) & 1, and the increment cannot carry out of a byte (t odd and h odd means h <= 253).
//
// The three tables (full palette 256 x 3, reduced palette 32 x 3, take table 256, AMS_RENDER_TABLE_BYTES in all; ams_amd/render.py builds
// them) are staged in LDS per block, the palettes as one word per colour.  Every lookup is bounded: a teacher id is a byte and both 256-row
// tables are whole, a student label outside [0, K) paints black, and a take entry that is not below K paints black too, so nothing is read
// outside a table whatever the labels or the table block hold.
//
// Two paths, uniform per launch and chosen by the launcher: a lane owns 16 consecutive pixels of a row (16-byte loads of frame and labels,
// three 16-byte stores per requested view) when W % 16 == 0 and every base is 16-byte aligned; one pixel per lane otherwise.
#include "common.hpp"
#include "kernels.hpp"

namespace ams {

constexpr int kRenderPalette = 0, kRenderReduced = 768, kRenderTake = 864;          // byte offsets inside the table block
static_assert(kRenderTake + 256 == AMS_RENDER_TABLE_BYTES, "table block layout");

struct RenderGeom {
    int B, H, W, K;
    int s32;                 // student labels are int32 (else uint8)
    int wide;                // 16 pixels per lane
    int tab_words;           // the table block is 4-byte aligned: staged by words
};

struct RenderTables {
    uint32_t pal[256];       // r | g << 8 | b << 16
    uint32_t red[32];
    uint8_t take[256];
};

__device__ __forceinline__ void render_stage_tables(const uint8_t* __restrict__ tables, int tab_words, RenderTables& s, uint32_t* s_raw) {
    // the block's bytes into LDS first (s_raw: AMS_RENDER_TABLE_BYTES / 4 words), then one word per colour
    if (tab_words) {
        for (int i = threadIdx.x; i < AMS_RENDER_TABLE_BYTES / 4; i += blockDim.x) s_raw[i] = reinterpret_cast<const uint32_t*>(tables)[i];
    } else {
        uint8_t* raw = reinterpret_cast<uint8_t*>(s_raw);
        for (int i = threadIdx.x; i < AMS_RENDER_TABLE_BYTES; i += blockDim.x) raw[i] = tables[i];
    }
    __syncthreads();
    const uint8_t* raw = reinterpret_cast<const uint8_t*>(s_raw);
    for (int i = threadIdx.x; i < 256 + 32; i += blockDim.x) {
        const uint8_t* p = raw + (i < 256 ? kRenderPalette + 3 * i : kRenderReduced + 3 * (i - 256));
        const uint32_t c = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
        if (i < 256) s.pal[i] = c;
        else s.red[i - 256] = c;
    }
    for (int i = threadIdx.x; i < 256; i += blockDim.x) s.take[i] = raw[kRenderTake + i];
    __syncthreads();
}

// what one pixel paints, as 24-bit colours
struct RenderPixel {
    uint32_t student, teacher, ignore, cross;
};

__device__ __forceinline__ RenderPixel render_pixel(const RenderTables& s, int K, int sl, bool has_s, uint32_t tl, bool has_t) {
    RenderPixel p;
    p.student = (has_s && sl >= 0 && sl < K) ? s.red[sl] : 0u;
    p.teacher = p.ignore = p.cross = 0u;
    if (has_t) {
        tl &= 255u;
        p.teacher = s.pal[tl];
        const int tk = s.take[tl];
        if (tk == 0) p.ignore = 0xffffffu;
        else if (has_s && tk != sl && tk < K) p.cross = s.red[tk];
    }
    return p;
}

// four pixels (24-bit colours) -> the three words they fill
__device__ __forceinline__ void pack4(const uint32_t* c, uint32_t* w) {
    w[0] = c[0] | (c[1] << 24);
    w[1] = (c[1] >> 8) | (c[2] << 16);
    w[2] = (c[2] >> 16) | (c[3] << 8);
}

// _overlay on the four bytes of a word
__device__ __forceinline__ uint32_t blend4(uint32_t f, uint32_t c) {
    const uint32_t x = f ^ c;
    const uint32_t h = (f & c) + ((x >> 1) & 0x7f7f7f7fu);
    return h + (x & h & 0x01010101u);
}

__device__ __forceinline__ uint8_t blend1(int f, int c) {
    const int t = f + c;
    int h = t >> 1;
    h += (t & 1) & (h & 1);
    return (uint8_t)h;
}

__device__ __forceinline__ void store_rgb(uint8_t* p, uint32_t c) {
    p[0] = (uint8_t)c; p[1] = (uint8_t)(c >> 8); p[2] = (uint8_t)(c >> 16);
}

__device__ __forceinline__ void store48(uint8_t* dst, const uint32_t* w) {
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(w[0], w[1], w[2], w[3]);
    d[1] = make_uint4(w[4], w[5], w[6], w[7]);
    d[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

__global__ __launch_bounds__(256) void render_views_kernel(const uint8_t* __restrict__ frames, const void* __restrict__ student,
                                                           const uint8_t* __restrict__ teacher, const uint8_t* __restrict__ tables, RenderGeom g,
                                                           ams_render_out out) {
    __shared__ RenderTables s;
    __shared__ uint32_t s_raw[AMS_RENDER_TABLE_BYTES / 4];
    render_stage_tables(tables, g.tab_words, s, s_raw);

    const int64_t row = (int64_t)blockIdx.z * g.H + blockIdx.y;          // row of the batch
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool has_s = student != nullptr, has_t = teacher != nullptr;

    if (g.wide) {
        const int x0 = t * 16;
        if (x0 >= g.W) return;
        const int64_t px = row * g.W + x0;                               // first of the lane's 16 pixels
        int sl[16];
        uint32_t tw[4] = {0u, 0u, 0u, 0u};
        if (has_s) {
            if (g.s32) {
                const uint4* p = reinterpret_cast<const uint4*>(static_cast<const int32_t*>(student) + px);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint4 v = p[q];
                    sl[4 * q] = (int)v.x; sl[4 * q + 1] = (int)v.y; sl[4 * q + 2] = (int)v.z; sl[4 * q + 3] = (int)v.w;
                }
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(student) + px);
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int i = 0; i < 16; ++i) sl[i] = (int)((w[i >> 2] >> (8 * (i & 3))) & 255u);
            }
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i) sl[i] = -1;
        }
        if (has_t) {
            const uint4 v = *reinterpret_cast<const uint4*>(teacher + px);
            tw[0] = v.x; tw[1] = v.y; tw[2] = v.z; tw[3] = v.w;
        }
        uint32_t f[12];
        if (frames != nullptr && (out.overlay_student || out.overlay_teacher)) {
            const uint4* p = reinterpret_cast<const uint4*>(frames + px * 3);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = p[q];
                f[4 * q] = v.x; f[4 * q + 1] = v.y; f[4 * q + 2] = v.z; f[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) f[i] = 0u;
        }
        uint32_t cs[12], ct[12], ig[12], cr[12];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t a[4], b[4], c[4], d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = 4 * q + j;
                const RenderPixel p = render_pixel(s, g.K, sl[i], has_s, tw[i >> 2] >> (8 * (i & 3)), has_t);
                a[j] = p.student; b[j] = p.teacher; c[j] = p.ignore; d[j] = p.cross;
            }
            pack4(a, cs + 3 * q); pack4(b, ct + 3 * q); pack4(c, ig + 3 * q); pack4(d, cr + 3 * q);
        }
        const int64_t o = px * 3;
        if (out.colour_student) store48(out.colour_student + o, cs);
        if (out.colour_teacher) store48(out.colour_teacher + o, ct);
        if (out.ignore_mask) store48(out.ignore_mask + o, ig);
        if (out.cross_mask) store48(out.cross_mask + o, cr);
        if (out.overlay_student) {
#pragma unroll
            for (int i = 0; i < 12; ++i) cs[i] = blend4(f[i], cs[i]);
            store48(out.overlay_student + o, cs);
        }
        if (out.overlay_teacher) {
#pragma unroll
            for (int i = 0; i < 12; ++i) ct[i] = blend4(f[i], ct[i]);
            store48(out.overlay_teacher + o, ct);
        }
        return;
    }

    if (t >= g.W) return;
    const int64_t px = row * g.W + t;
    int sl = -1;
    if (has_s) sl = g.s32 ? static_cast<const int32_t*>(student)[px] : (int)static_cast<const uint8_t*>(student)[px];
    const RenderPixel p = render_pixel(s, g.K, sl, has_s, has_t ? teacher[px] : 0u, has_t);
    const int64_t o = px * 3;
    if (out.colour_student) store_rgb(out.colour_student + o, p.student);
    if (out.colour_teacher) store_rgb(out.colour_teacher + o, p.teacher);
    if (out.ignore_mask) store_rgb(out.ignore_mask + o, p.ignore);
    if (out.cross_mask) store_rgb(out.cross_mask + o, p.cross);
    if (out.overlay_student || out.overlay_teacher) {
        const int f0 = frames[o], f1 = frames[o + 1], f2 = frames[o + 2];
        if (out.overlay_student) {
            uint8_t* d = out.overlay_student + o;
            d[0] = blend1(f0, p.student & 255); d[1] = blend1(f1, (p.student >> 8) & 255); d[2] = blend1(f2, (p.student >> 16) & 255);
        }
        if (out.overlay_teacher) {
            uint8_t* d = out.overlay_teacher + o;
            d[0] = blend1(f0, p.teacher & 255); d[1] = blend1(f1, (p.teacher >> 8) & 255); d[2] = blend1(f2, (p.teacher >> 16) & 255);
        }
    }
}

static inline bool render_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// Everything is checked before the launch: a refused call sets the error, returns AMS_E_INVALID and touches no output.
int launch_render_views(const uint8_t* frames, const void* student, int student_dtype, const uint8_t* teacher, int B, int H, int W, int K,
                        const uint8_t* tables, const ams_render_out* out, hipStream_t st) {
    AMS_REQUIRE(B > 0 && H > 0 && W > 0, "render_views: bad geometry %d x %dx%d", B, H, W);
    AMS_REQUIRE(B <= 65535 && H <= 65535, "render_views: %d x %d rows exceed the grid (65535 each)", B, H);
    AMS_REQUIRE(K >= 1 && K <= 32, "render_views: K=%d outside 1..32", K);
    AMS_REQUIRE(student_dtype == AMS_DT_U8 || student_dtype == AMS_DT_I32, "render_views: student labels of dtype %d (uint8 or int32)", student_dtype);
    AMS_REQUIRE(tables, "render_views: null table block");
    AMS_REQUIRE(out && (out->colour_student || out->overlay_student || out->colour_teacher || out->overlay_teacher || out->ignore_mask || out->cross_mask),
                "render_views: no view requested");
    AMS_REQUIRE(!(out->colour_student || out->overlay_student || out->cross_mask) || student, "render_views: a requested view reads the student labels, which are null");
    AMS_REQUIRE(!(out->colour_teacher || out->overlay_teacher || out->ignore_mask || out->cross_mask) || teacher,
                "render_views: a requested view reads the teacher labels, which are null");
    AMS_REQUIRE(!(out->overlay_student || out->overlay_teacher) || frames, "render_views: an overlay is requested and the frames are null");
    RenderGeom g;
    g.B = B; g.H = H; g.W = W; g.K = K;
    g.s32 = student_dtype == AMS_DT_I32;
    g.tab_words = render_aligned(tables, 4);
    // every row starts at a multiple of W (x 3, x 4) bytes from its base: W % 16 == 0 and 16-byte bases make every access of the wide path aligned
    g.wide = W % 16 == 0 && render_aligned(frames, 16) && render_aligned(student, 16) && render_aligned(teacher, 16) &&
             render_aligned(out->colour_student, 16) && render_aligned(out->overlay_student, 16) && render_aligned(out->colour_teacher, 16) &&
             render_aligned(out->overlay_teacher, 16) && render_aligned(out->ignore_mask, 16) && render_aligned(out->cross_mask, 16);
    note_kernel("render_views_kernel");
    hipLaunchKernelGGL(render_views_kernel, dim3(cdiv(W, g.wide ? 16 * 256 : 256), H, B), dim3(256), 0, st, frames, student, teacher, tables, g, *out);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
