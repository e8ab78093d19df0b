// The predicted uplink frame AUP1 (include/ams_hip.h states the format; tests/uplink_inter_ref.py is its NumPy restatement, byte for byte): a
// frame as one vector per 16 x 16 macroblock into a reference frame plus the residual through AUC1's transform and block code
// (uplink_common.hpp).  Integer arithmetic throughout; slices = the motion slices (32 macroblocks each), then AUC1's.
//
// Encoder scratch (bytes): [int16 residual coefficients, zig-zag order, 64 per block, planes Y Cb Cr][int32 slice lengths -> offsets, slices + 1]
//                          [int32 byte counts, 100 qualities x slices][int8 vectors (dy, dx) per macroblock]
//   uplink_inter_search_kernel    one block per macroblock: the clipped 46 x 46 luma window of the reference and the macroblock's own luma as
//                                 bytes in LDS; lanes split the 961 candidates, skip the ones whose window leaves the frame (no pixel outside
//                                 it is read), 16 rows of four v_sad_u8 on words aligned at the candidate's byte offset; one min over
//                                 cost << 10 | rank (shuffles in a wave, an LDS atomic across the four)
//   uplink_inter_transform_kernel one wave per macroblock: the prediction (luma per lane, the 9 x 9 chroma samples the averages need in LDS),
//                                 current - prediction, the forward passes, coefficients out in zig-zag order
//   uplink_inter_sizes_kernel     one block per slice, one thread per quality; a motion slice's count is the same at every quality; an
//                                 all-zero slice counts 0 (every block, every macroblock of it takes exactly two bits)
//   uplink_inter_totals_kernel    one block per quality
//   uplink_inter_lengths_kernel, uplink_inter_encode_scan_kernel, uplink_inter_write_kernel: as AUC1's, over motion and residual slices
// Decoder scratch (bytes): [int16 levels][int32 slice offsets, slices + 1][int8 vectors]
//   uplink_inter_decode_scan_kernel  header "AUP1", table sum, scan -> status
//   uplink_inter_parse_kernel     nothing unless OK: a thread per slice; a motion slice's vectors are validated (range, window in the frame) as
//                                 they are read; a slice of length 0 is zeros; a long slice of zeros is AMS_UPLINK_BAD_ZERO_SLICE
//   uplink_inter_rebuild_kernel   nothing unless OK (so every vector it reads through is legal): dequantise, inverse passes, + prediction,
//                                 clamp, colour -> RGB
#include "uplink_common.hpp"

namespace ams {

namespace {

constexpr int UP_RANGE = 15;                   // vector components in -15 .. 15
constexpr int UP_CAND = 31 * 31;
constexpr int UP_ZERO_BIAS = 128;              // the search's bias against a vector != 0 (DESIGN 4.11 has the grid that chose it)
constexpr int UP_WIN = 46, UP_WIN_WORDS = 12;  // the search window: 46 rows of 46 bytes in 12 words

// a candidate's place in the tie order: |dy| + |dx|, then dy, then dx; candidate (dy, dx) sits at (dy + 15) * 31 + dx + 15
struct RankTable { uint16_t r[UP_CAND]; };
constexpr RankTable up_make_rank() {
    RankTable t{};
    int n = 0;
    for (int l = 0; l <= 2 * UP_RANGE; ++l)
        for (int dy = -UP_RANGE; dy <= UP_RANGE; ++dy) {
            const int a = l - (dy < 0 ? -dy : dy);
            if (a < 0 || a > UP_RANGE) continue;
            t.r[(dy + UP_RANGE) * 31 - a + UP_RANGE] = (uint16_t)n++;
            if (a) t.r[(dy + UP_RANGE) * 31 + a + UP_RANGE] = (uint16_t)n++;
        }
    return t;
}
__constant__ RankTable UP_RANK = up_make_rank();

struct InterGeom { int nmb, nms, total; };     // macroblocks, motion slices, all slices
__host__ __device__ inline InterGeom inter_geom(const UplinkGeom& g) {
    InterGeom m;
    m.nmb = g.nb[1];
    m.nms = (m.nmb + UP_SLICE - 1) / UP_SLICE;
    m.total = m.nms + g.nslices;
    return m;
}

__device__ inline int up_luma_at(const uint8_t* p) { return up_luma(p[0], p[1], p[2]); }

// the bits of macroblock i's two codes; j = its place in its motion slice
__device__ inline uint32_t up_vec_value(int d) { return d ? up_se_value(d) : 1u; }
__device__ inline int up_mb_bits(const int8_t* vec, int i, int j) {
    const int pdy = j ? vec[2 * i - 2] : 0, pdx = j ? vec[2 * i - 1] : 0;
    return up_code_bits(up_vec_value(vec[2 * i] - pdy)) + up_code_bits(up_vec_value(vec[2 * i + 1] - pdx));
}
__device__ inline int up_motion_n(const InterGeom& m, int s) { return m.nmb - s * UP_SLICE < UP_SLICE ? m.nmb - s * UP_SLICE : UP_SLICE; }

// The prediction of macroblock (mby, mbx) for the LEGAL vector (dy, dx), by the macroblock's wave: lane (qy, qx) gets its 2 x 2 luma pixels
// and its chroma sample.  cw = the 9 x 9 chroma samples of the reference at (8 mby + (dy >> 1), 8 mbx + (dx >> 1)), of which only the rows
// and columns the vector's parity needs are formed: those lie in the plane (include/ams_hip.h).  One barrier inside.
struct Prediction { int y[2][2], cb, cr; };
__device__ inline void up_predict(const uint8_t* ref, const UplinkGeom& g, int mby, int mbx, int dy, int dx, int t, int (*cw)[81], Prediction& p) {
    const int oy = dy & 1, ox = dx & 1, cy0 = 8 * mby + (dy >> 1), cx0 = 8 * mbx + (dx >> 1);
    for (int i = t; i < 81; i += 64) {
        const int r = i / 9, c = i - 9 * r;
        if (r >= 8 + oy || c >= 8 + ox) continue;
        int cb = 2, cr = 2;
        for (int k = 0; k < 4; ++k) {
            const uint8_t* s = ref + ((int64_t)(2 * (cy0 + r) + (k >> 1)) * g.W + 2 * (cx0 + c) + (k & 1)) * 3;
            cb += up_cb(s[0], s[1], s[2]);
            cr += up_cr(s[0], s[1], s[2]);
        }
        cw[0][i] = cb >> 2;
        cw[1][i] = cr >> 2;
    }
    const int qy = t >> 3, qx = t & 7;
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) p.y[a][b] = up_luma_at(ref + ((int64_t)(16 * mby + 2 * qy + a + dy) * g.W + 16 * mbx + 2 * qx + b + dx) * 3);
    __syncthreads();
    int v[2];
    for (int k = 0; k < 2; ++k) {
        const int* w = cw[k] + qy * 9 + qx;
        v[k] = oy && ox ? (w[0] + w[1] + w[9] + w[10] + 2) >> 2 : oy ? (w[0] + w[9] + 1) >> 1 : ox ? (w[0] + w[1] + 1) >> 1 : w[0];
    }
    p.cb = v[0];
    p.cr = v[1];
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------- encoder
__global__ void __launch_bounds__(256) uplink_inter_search_kernel(const uint8_t* frame, const uint8_t* ref, UplinkGeom g, int8_t* vec) {
    __shared__ uint32_t win[UP_WIN * UP_WIN_WORDS];
    __shared__ uint32_t cur[64];
    __shared__ uint32_t best;
    const int mbw = g.W >> 4, mby = blockIdx.x / mbw, mbx = blockIdx.x - mby * mbw, t = threadIdx.x;
    const int y0 = 16 * mby, x0 = 16 * mbx;
    // the window, clipped to the frame: rows wy .. wy + wh - 1, columns wx .. wx + ww - 1
    const int wy = y0 > UP_RANGE ? y0 - UP_RANGE : 0, wx = x0 > UP_RANGE ? x0 - UP_RANGE : 0;
    const int wh = (y0 + 16 + UP_RANGE < g.H ? y0 + 16 + UP_RANGE : g.H) - wy, ww = (x0 + 16 + UP_RANGE < g.W ? x0 + 16 + UP_RANGE : g.W) - wx;
    uint8_t* winb = reinterpret_cast<uint8_t*>(win);
    for (int i = t; i < wh * ww; i += 256) {
        const int r = i / ww, c = i - r * ww;
        winb[r * 4 * UP_WIN_WORDS + c] = (uint8_t)up_luma_at(ref + ((int64_t)(wy + r) * g.W + wx + c) * 3);
    }
    reinterpret_cast<uint8_t*>(cur)[t] = (uint8_t)up_luma_at(frame + ((int64_t)(y0 + (t >> 4)) * g.W + x0 + (t & 15)) * 3);
    if (t == 0) best = 0xffffffffu;
    __syncthreads();
    // the legal components: the candidate's 16 x 16 window inside the frame (border macroblocks have fewer candidates)
    const int dy_lo = y0 < UP_RANGE ? -y0 : -UP_RANGE, dy_hi = g.H - 16 - y0 < UP_RANGE ? g.H - 16 - y0 : UP_RANGE;
    const int dx_lo = x0 < UP_RANGE ? -x0 : -UP_RANGE, dx_hi = g.W - 16 - x0 < UP_RANGE ? g.W - 16 - x0 : UP_RANGE;
    uint32_t mine = 0xffffffffu;
    for (int c = t; c < UP_CAND; c += 256) {
        const int dy = c / 31 - UP_RANGE, dx = c - (c / 31) * 31 - UP_RANGE;
        if (dy < dy_lo || dy > dy_hi || dx < dx_lo || dx > dx_hi) continue;
        const int oy = y0 + dy - wy, ox = x0 + dx - wx;                          // 0 <= oy <= wh - 16, 0 <= ox <= ww - 16 <= 30
        const uint32_t* row = win + oy * UP_WIN_WORDS + (ox >> 2);                // words row[0 .. 4]: ox >> 2 <= 7
        const uint32_t sh = (uint32_t)ox & 3u;
        uint32_t sad = 0;
        for (int r = 0; r < 16; ++r, row += UP_WIN_WORDS) {
            const uint32_t w0 = row[0], w1 = row[1], w2 = row[2], w3 = row[3], w4 = row[4];
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, sh), cur[4 * r], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w2, w1, sh), cur[4 * r + 1], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w3, w2, sh), cur[4 * r + 2], sad);
            sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w4, w3, sh), cur[4 * r + 3], sad);
        }
        const uint32_t key = (sad + (dy || dx ? (uint32_t)UP_ZERO_BIAS : 0u)) << 10 | UP_RANK.r[c];      // cost <= 65280 + bias: 22 bits
        mine = key < mine ? key : mine;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)mine, o);
        mine = other < mine ? other : mine;
    }
    if ((t & 63) == 0) atomicMin(&best, mine);
    __syncthreads();
    const uint32_t rank = best & 1023u;                                          // (0, 0) is always legal: best was set
    for (int c = t; c < UP_CAND; c += 256)
        if (UP_RANK.r[c] == rank) {
            vec[2 * blockIdx.x] = (int8_t)(c / 31 - UP_RANGE);
            vec[2 * blockIdx.x + 1] = (int8_t)(c - (c / 31) * 31 - UP_RANGE);
        }
}

__global__ void __launch_bounds__(64) uplink_inter_transform_kernel(const uint8_t* frame, const uint8_t* ref, UplinkGeom g, const int8_t* vec,
                                                                    int16_t* coefs) {
    __shared__ int px[6][8 * UP_ROW];
    __shared__ int16_t ob[6][64];
    __shared__ int cw[2][81];
    const int mbw = g.W >> 4, mby = blockIdx.x / mbw, mbx = blockIdx.x - mby * mbw;
    const int t = threadIdx.x, qy = t >> 3, qx = t & 7;
    Prediction pr;
    up_predict(ref, g, mby, mbx, vec[2 * blockIdx.x], vec[2 * blockIdx.x + 1], t, cw, pr);      // the search's vector: legal
    int cb = 2, cr = 2;
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * qy + dy;
        const uint8_t* p = frame + ((int64_t)(16 * mby + y) * g.W + 16 * mbx + 2 * qx) * 3;
        for (int dx = 0; dx < 2; ++dx) {
            const int x = 2 * qx + dx, r = p[3 * dx], gr = p[3 * dx + 1], b = p[3 * dx + 2];
            cb += up_cb(r, gr, b);
            cr += up_cr(r, gr, b);
            px[(y >> 3) * 2 + (x >> 3)][(y & 7) * UP_ROW + (x & 7)] = up_luma(r, gr, b) - pr.y[dy][dx];
        }
    }
    px[4][qy * UP_ROW + qx] = (cb >> 2) - pr.cb;
    px[5][qy * UP_ROW + qx] = (cr >> 2) - pr.cr;
    __syncthreads();
    up_forward_passes(px, ob, t);
    up_store_coefs(ob, g, mby, mbx, coefs, t);
}

__global__ void __launch_bounds__(128) uplink_inter_sizes_kernel(const int16_t* coefs, const int8_t* vec, UplinkGeom g, int32_t* table) {
    __shared__ uint32_t qtab[64][100];
    __shared__ uint32_t cf[UP_SLICE * 32];
    const InterGeom m = inter_geom(g);
    const int s = blockIdx.x;
    if (s >= m.nms) {
        up_slice_sizes<true>(coefs, slice_ref(g, s - m.nms), qtab, cf, table + s, m.total);
        return;
    }
    if (threadIdx.x >= 100) return;
    const int n = up_motion_n(m, s);
    int bits = 0;
    for (int j = 0; j < n; ++j) bits += up_mb_bits(vec, s * UP_SLICE + j, j);
    table[(int64_t)threadIdx.x * m.total + s] = bits == 2 * n ? 0 : (bits + 7) >> 3;
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_inter_totals_kernel(const int32_t* table, UplinkGeom g, int64_t* sizes) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    up_totals(table, inter_geom(g).total, sizes, sh);
}

__global__ void __launch_bounds__(64) uplink_inter_lengths_kernel(const int16_t* coefs, const int8_t* vec, UplinkGeom g, int q, int32_t* lens) {
    __shared__ uint32_t qt[2][64];
    up_fill_tables(qt, q);
    const InterGeom m = inter_geom(g);
    const int sidx = 2 * blockIdx.x + (threadIdx.x >> 5), j = threadIdx.x & 31;
    int bits = 0, n = 0;
    if (sidx < m.nms) {
        n = up_motion_n(m, sidx);
        if (j < n) bits = up_mb_bits(vec, sidx * UP_SLICE + j, j);
    } else if (sidx < m.total) {
        const SliceRef s = slice_ref(g, sidx - m.nms);
        n = s.n;
        if (j < n) {
            const int16_t* c = coefs + (int64_t)(s.first + j) * 64;
            CountSink sink;
            walk_block(c, qt[s.plane > 0], up_pred(c, qt[s.plane > 0], j), sink);
            bits = sink.bits;
        }
    }
    for (int o = 16; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 32);
    if (j == 0 && sidx < m.total) lens[sidx] = bits == 2 * n ? 0 : (bits + 7) >> 3;          // two bits each: nothing but zeros
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_inter_encode_scan_kernel(int32_t* lens, UplinkGeom g, int q, uint8_t* payload, int64_t cap,
                                                                                      int64_t* bytes_out, int32_t* status) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    up_encode_scan(lens, inter_geom(g).total, g.H, g.W, q, 'P', payload, cap, bytes_out, status, sh);
}

__global__ void __launch_bounds__(64) uplink_inter_write_kernel(const int16_t* coefs, const int8_t* vec, UplinkGeom g, int q, const int32_t* offs,
                                                                const int32_t* status, uint8_t* payload, int64_t cap) {
    __shared__ uint32_t qt[2][64];
    __shared__ uint32_t img[2][UP_SLICE_WORDS];
    if (*status != AMS_UPLINK_OK) return;                        // all or nothing (the same word for every thread)
    up_fill_tables(qt, q);
    const InterGeom m = inter_geom(g);
    const int half = threadIdx.x >> 5, sidx = 2 * blockIdx.x + half, j = threadIdx.x & 31;
    int len = 0;
    int64_t at = 0;
    if (sidx < m.total) {
        at = offs[sidx];
        len = offs[sidx + 1] - offs[sidx];
        len = len < 0 ? 0 : len > 4 * UP_SLICE_WORDS ? 4 * UP_SLICE_WORDS : len;
    }
    for (int w = j; w < (len + 3) >> 2; w += 32) img[half][w] = 0;
    __syncthreads();
    int bits = 0, pred = 0, mb = -1;
    const int16_t* c = nullptr;
    const uint32_t* table = nullptr;
    if (len > 0) {                                               // a slice of length 0 has no bits to write
        if (sidx < m.nms) {
            if (j < up_motion_n(m, sidx)) {
                mb = sidx * UP_SLICE + j;
                bits = up_mb_bits(vec, mb, j);
            }
        } else {
            const SliceRef s = slice_ref(g, sidx - m.nms);
            if (j < s.n) {
                c = coefs + (int64_t)(s.first + j) * 64;
                table = qt[s.plane > 0];
                pred = up_pred(c, table, j);
                CountSink count;
                walk_block(c, table, pred, count);
                bits = count.bits;
            }
        }
    }
    int start = bits;                                            // inclusive scan over the half wave, then exclusive
    for (int o = 1; o < 32; o <<= 1) {
        const int up = __shfl_up(start, o, 32);
        if (j >= o) start += up;
    }
    start -= bits;
    if (c) {
        EmitSink sink(img[half], start);
        walk_block(c, table, pred, sink);
        sink.flush();
    } else if (mb >= 0) {
        EmitSink sink(img[half], start);
        for (int k = 0; k < 2; ++k) {
            const uint32_t value = up_vec_value(vec[2 * mb + k] - (j ? vec[2 * mb - 2 + k] : 0));
            sink.put(value, up_code_bits(value));
        }
        sink.flush();
    }
    __syncthreads();
    const int64_t base = 16 + 2 * (int64_t)m.total + at;
    for (int i = j; i < len; i += 32)
        if (base + i < cap) payload[base + i] = (uint8_t)(img[half][i >> 2] >> (24 - 8 * (i & 3)));      // (implied by the status)
}

// ------------------------------------------------------------------------------------------------------------------- decoder
__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_inter_decode_scan_kernel(const uint8_t* payload, int64_t bytes, UplinkGeom g, int32_t* offs,
                                                                                      int32_t* status) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    __shared__ int header_ok;
    up_decode_scan(payload, bytes, g.H, g.W, inter_geom(g).total, 'P', offs, status, sh, &header_ok);
}

namespace {

// A motion slice of len > 0 bytes: the first violation in reading order, or AMS_UPLINK_OK; v = the slice's n vectors, written as validated
__device__ inline int parse_motion(const uint8_t* data, int len, const UplinkGeom& g, int first, int n, int8_t* v) {
    BitReader r(data, len);
    const int mbw = g.W >> 4;
    int p[2] = {0, 0}, any = 0;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 2; ++k) {
            const int u = r.ue();
            if (u < 0) return -u;
            p[k] += (u & 1) ? (u + 1) >> 1 : -(u >> 1);
            if (p[k] > UP_RANGE || p[k] < -UP_RANGE) return AMS_UPLINK_BAD_VECTOR;
        }
        const int mby = (first + i) / mbw, mbx = first + i - mby * mbw, y = 16 * mby + p[0], x = 16 * mbx + p[1];
        if (y < 0 || y > g.H - 16 || x < 0 || x > g.W - 16) return AMS_UPLINK_BAD_VECTOR;
        v[2 * i] = (int8_t)p[0];
        v[2 * i + 1] = (int8_t)p[1];
        any |= p[0] | p[1];
    }
    r.fill();
    if ((r.pos + 7) >> 3 != len || (r.left() > 0 && (r.buf >> (64 - r.left())) != 0)) return AMS_UPLINK_BAD_SLICE_END;
    return any ? AMS_UPLINK_OK : AMS_UPLINK_BAD_ZERO_SLICE;
}

}  // namespace

__global__ void __launch_bounds__(64) uplink_inter_parse_kernel(const uint8_t* payload, UplinkGeom g, const int32_t* offs, int16_t* levels, int8_t* vec,
                                                                int32_t* status) {
    if (*status != AMS_UPLINK_OK) return;                        // header or table refused: the offsets were never written
    const InterGeom m = inter_geom(g);
    const int sidx = blockIdx.x * 64 + threadIdx.x;
    if (sidx >= m.total) return;
    const uint8_t* data = payload + 16 + 2 * (int64_t)m.total + offs[sidx];
    const int len = offs[sidx + 1] - offs[sidx];
    int st = AMS_UPLINK_OK;
    if (sidx < m.nms) {
        const int n = up_motion_n(m, sidx);
        int8_t* v = vec + 2 * sidx * UP_SLICE;
        if (len == 0)
            for (int i = 0; i < 2 * n; ++i) v[i] = 0;
        else
            st = parse_motion(data, len, g, sidx * UP_SLICE, n, v);
    } else {
        const SliceRef s = slice_ref(g, sidx - m.nms);
        uint4* lv = reinterpret_cast<uint4*>(levels + (int64_t)s.first * 64);
        if (len == 0) {
            for (int i = 0; i < 8 * s.n; ++i) lv[i] = make_uint4(0, 0, 0, 0);
        } else {
            st = parse_slice(data, len, s.n, levels + (int64_t)s.first * 64);
            if (st == AMS_UPLINK_OK) {                           // the slice's own levels, as this thread has just written them
                uint32_t any = 0;
                for (int i = 0; i < 8 * s.n; ++i) any |= lv[i].x | lv[i].y | lv[i].z | lv[i].w;
                if (!any) st = AMS_UPLINK_BAD_ZERO_SLICE;
            }
        }
    }
    if (st != AMS_UPLINK_OK) atomicMax(status, st);
}

__global__ void __launch_bounds__(64) uplink_inter_rebuild_kernel(const uint8_t* payload, const uint8_t* ref, UplinkGeom g, const int16_t* levels,
                                                                  const int8_t* vec, const int32_t* status, uint8_t* frame) {
    __shared__ int px[6][8 * UP_ROW];
    __shared__ int cw[2][81];
    if (*status != AMS_UPLINK_OK) return;                        // all or nothing; under OK every vector has been validated
    const int q = payload[8];
    const int mbw = g.W >> 4, mby = blockIdx.x / mbw, mbx = blockIdx.x - mby * mbw;
    const int t = threadIdx.x, qy = t >> 3, qx = t & 7;
    up_dequantise(px, levels, g, q, mby, mbx, t);
    up_inverse_passes<false>(px, t);
    Prediction pr;
    up_predict(ref, g, mby, mbx, vec[2 * blockIdx.x], vec[2 * blockIdx.x + 1], t, cw, pr);
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int y = 2 * qy + dy, x = 2 * qx + dx;
            int* v = &px[(y >> 3) * 2 + (x >> 3)][(y & 7) * UP_ROW + (x & 7)];
            *v = clamp255(*v + pr.y[dy][dx]);
        }
    px[4][qy * UP_ROW + qx] = clamp255(px[4][qy * UP_ROW + qx] + pr.cb);
    px[5][qy * UP_ROW + qx] = clamp255(px[5][qy * UP_ROW + qx] + pr.cr);
    up_write_rgb(px, g, mby, mbx, frame, t);                     // each lane reads back what it has just written
}

// ---------------------------------------------------------------------------------------------------------------------- host
static size_t round16(size_t n) { return (n + 15) / 16 * 16; }
static size_t upi_offsets_at(const UplinkGeom& g) { return (size_t)g.nblocks * 128; }
static size_t upi_after_offsets(const UplinkGeom& g) { return upi_offsets_at(g) + round16(4 * ((size_t)inter_geom(g).total + 1)); }
static size_t upi_vectors_bytes(const UplinkGeom& g) { return round16(2 * (size_t)inter_geom(g).nmb); }
static size_t upi_enc_vectors_at(const UplinkGeom& g) { return upi_after_offsets(g) + 400 * (size_t)inter_geom(g).total; }

int64_t uplink_inter_max_bytes(int H, int W) {
    const UplinkGeom g = uplink_geom(H, W);
    const InterGeom m = inter_geom(g);
    return 16 + 2 * (int64_t)m.total + 208 * (int64_t)g.nblocks + 3 * (int64_t)m.nmb;
}
size_t uplink_inter_encode_scratch_bytes(int H, int W) {
    const UplinkGeom g = uplink_geom(H, W);
    return upi_enc_vectors_at(g) + upi_vectors_bytes(g);
}
size_t uplink_inter_decode_scratch_bytes(int H, int W) {
    const UplinkGeom g = uplink_geom(H, W);
    return upi_after_offsets(g) + upi_vectors_bytes(g);
}

int launch_uplink_inter_transform(const uint8_t* frame, const uint8_t* ref, int H, int W, void* scratch, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    int8_t* vec = reinterpret_cast<int8_t*>((char*)scratch + upi_enc_vectors_at(g));
    hipLaunchKernelGGL(uplink_inter_search_kernel, dim3(inter_geom(g).nmb), dim3(256), 0, st, frame, ref, g, vec);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_transform_kernel, dim3(inter_geom(g).nmb), dim3(64), 0, st, frame, ref, g, (const int8_t*)vec, (int16_t*)scratch);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_inter_size_table(void* scratch, int H, int W, int64_t* sizes, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    int32_t* table = reinterpret_cast<int32_t*>((char*)scratch + upi_after_offsets(g));
    const int8_t* vec = reinterpret_cast<const int8_t*>((char*)scratch + upi_enc_vectors_at(g));
    hipLaunchKernelGGL(uplink_inter_sizes_kernel, dim3(inter_geom(g).total), dim3(128), 0, st, (const int16_t*)scratch, vec, g, table);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_totals_kernel, dim3(100), dim3(BLOCK_SCAN_THREADS), 0, st, (const int32_t*)table, g, sizes);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_inter_encode(void* scratch, int H, int W, int q, uint8_t* payload, int64_t cap, int64_t* bytes_out, int32_t* status, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    const int total = inter_geom(g).total;
    const int16_t* coefs = (const int16_t*)scratch;
    int32_t* lens = reinterpret_cast<int32_t*>((char*)scratch + upi_offsets_at(g));
    const int8_t* vec = reinterpret_cast<const int8_t*>((char*)scratch + upi_enc_vectors_at(g));
    hipLaunchKernelGGL(uplink_inter_lengths_kernel, dim3((total + 1) / 2), dim3(64), 0, st, coefs, vec, g, q, lens);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_encode_scan_kernel, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, st, lens, g, q, payload, cap, bytes_out, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_write_kernel, dim3((total + 1) / 2), dim3(64), 0, st, coefs, vec, g, q, (const int32_t*)lens,
                       (const int32_t*)status, payload, cap);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_inter_decode(const uint8_t* payload, int64_t bytes, const uint8_t* ref, int H, int W, uint8_t* frame, int32_t* status, void* scratch,
                               hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    const int total = inter_geom(g).total;
    int16_t* levels = (int16_t*)scratch;
    int32_t* offs = reinterpret_cast<int32_t*>((char*)scratch + upi_offsets_at(g));
    int8_t* vec = reinterpret_cast<int8_t*>((char*)scratch + upi_after_offsets(g));
    hipLaunchKernelGGL(uplink_inter_decode_scan_kernel, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, st, payload, bytes, g, offs, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_parse_kernel, dim3((total + 63) / 64), dim3(64), 0, st, payload, g, (const int32_t*)offs, levels, vec, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_inter_rebuild_kernel, dim3(inter_geom(g).nmb), dim3(64), 0, st, payload, ref, g, (const int16_t*)levels,
                       (const int8_t*)vec, (const int32_t*)status, frame);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
