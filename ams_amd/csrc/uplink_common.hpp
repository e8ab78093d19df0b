// What the uplink codec's two payload kinds share (k_uplink.hip: AUC1, k_uplink_inter.hip: AUP1): tables, the level rule, the block code and
// its sinks, the slice cut, the two transform passes over the six blocks of a macroblock, the scans and the slice parser.  Device code only;
// every kernel that uses a piece is in one of those two files.
#pragma once
#include "common.hpp"
#include "kernels.hpp"
#include "block_scan.hpp"

namespace ams {

namespace {

constexpr int UP_SLICE = 32;                   // blocks per slice
constexpr int UP_SLICE_WORDS = 1664;           // 32 blocks x 1664 bits, in 32-bit words
constexpr int UP_ROW = 9;                      // words per row of an 8 x 8 block in LDS

__constant__ int UP_M[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},     {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                               {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784}, {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                               {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896}, {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                               {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567}, {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
__constant__ uint8_t UP_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
// zig-zag position -> natural index
__constant__ uint8_t UP_ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                  35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// natural index -> zig-zag position
__constant__ uint8_t UP_ZZ_INV[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
                                      10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

__device__ inline int clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// the colour equations of one RGB pixel
__device__ inline int up_luma(int r, int gr, int b) { return clamp255((19595 * r + 38470 * gr + 7471 * b + 32768) >> 16); }
__device__ inline int up_cb(int r, int gr, int b) { return clamp255(((-11059 * r - 21709 * gr + 32768 * b + 32768) >> 16) + 128); }
__device__ inline int up_cr(int r, int gr, int b) { return clamp255(((32768 * r - 27439 * gr - 5329 * b + 32768) >> 16) + 128); }

// the table entry of quality q (1 .. 100) for the coefficient at natural index `nat`
__device__ inline int up_qt(int q, int chroma, int nat) {
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    const int v = ((int)UP_BASE[chroma][nat] * s + 50) / 100;
    return v < 1 ? 1 : v > 255 ? 255 : v;
}
// entry | ceil(2^20 / entry) << 8: (n * m) >> 20 == n / entry for every n < 4096
__device__ inline uint32_t up_qt_packed(int qt) { return (uint32_t)qt | (((1u << 20) + (uint32_t)qt - 1) / (uint32_t)qt) << 8; }
// |level| of a coefficient; |c| is held to 2047 (the transform stays below 1100), so the numerator stays below 4096
__device__ inline int up_level_abs(int c, uint32_t packed) {
    const uint32_t a = (uint32_t)(c < 0 ? -c : c), qt = packed & 255u;
    return (int)((((a > 2047u ? 2047u : a) + (qt >> 1)) * (packed >> 8)) >> 20);
}
__device__ inline int up_level(int c, uint32_t packed) {
    const int l = up_level_abs(c, packed);
    return c < 0 ? -l : l;
}
// ue(v) is v + 1 written in 2 floor(log2(v + 1)) + 1 bits
__device__ inline int up_code_bits(uint32_t value) { return 63 - 2 * __clz((int)value); }          // value >= 1
__device__ inline uint32_t up_se_value(int v) { return v > 0 ? 2u * (uint32_t)v : 2u * (uint32_t)(-v) + 1u; }

struct SliceRef { int plane, first, n; };      // first: the slice's first block, counted over the three planes; n: its blocks
__device__ inline SliceRef slice_ref(const UplinkGeom& g, int s) {
    SliceRef r;
    r.plane = s < g.ns[0] ? 0 : s < g.ns[0] + g.ns[1] ? 1 : 2;
    const int sb = r.plane == 0 ? 0 : r.plane == 1 ? g.ns[0] : g.ns[0] + g.ns[1];
    const int pb = r.plane == 0 ? 0 : r.plane == 1 ? g.nb[0] : g.nb[0] + g.nb[1];
    const int b0 = (s - sb) * UP_SLICE, left = g.nb[r.plane] - b0;
    r.first = pb + b0;
    r.n = left < UP_SLICE ? left : UP_SLICE;
    return r;
}

struct CountSink {
    int bits = 0;
    __device__ void put(uint32_t, int n) { bits += n; }
};
// ORs codes into a slice image of 32-bit words, the stream's first bit in bit 31 of word 0
struct EmitSink {
    uint32_t* img;
    int w, pending;                            // the word the pending bits belong to; 0 .. 31 of them, the low bits of acc
    uint64_t acc = 0;
    __device__ EmitSink(uint32_t* image, int bit) : img(image), w(bit >> 5), pending(bit & 31) {}
    __device__ void put(uint32_t value, int n) {                 // n <= 25
        acc = (acc << n) | value;
        pending += n;
        if (pending >= 32) {
            pending -= 32;
            if (w < UP_SLICE_WORDS) atomicOr(&img[w], (uint32_t)(acc >> pending));
            ++w;
            acc &= (1ull << pending) - 1;
        }
    }
    __device__ void flush() {
        if (pending && w < UP_SLICE_WORDS) atomicOr(&img[w], (uint32_t)(acc << (32 - pending)));
    }
};

// One block's codes: c = its 64 coefficients (16-byte aligned), qt = the packed table in zig-zag order, pred = the DC level before it
template <class Sink>
__device__ inline void walk_block(const int16_t* c, const uint32_t* qt, int pred, Sink& sink) {
    int run = 0;
    for (int i = 0; i < 8; ++i) {
        const uint4 v = *reinterpret_cast<const uint4*>(c + 8 * i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * i + j;
            const int coef = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1)));
            if (k == 0) {
                const int d = up_level(coef, qt[0]) - pred;
                const uint32_t value = d ? up_se_value(d) : 1u;
                sink.put(value, up_code_bits(value));
                continue;
            }
            const int l = coef ? up_level(coef, qt[k]) : 0;
            if (!l) { ++run; continue; }
            sink.put((uint32_t)run + 2u, up_code_bits((uint32_t)run + 2u));
            const uint32_t value = up_se_value(l);
            sink.put(value, up_code_bits(value));
            run = 0;
        }
    }
    sink.put(1u, 1);
}

__device__ inline uint32_t load_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
__device__ inline uint32_t load_u32(const uint8_t* p) { return load_u16(p) | (load_u16(p + 2) << 16); }


// the packed tables of one quality in zig-zag order, luminance then chrominance, by the block's 64 threads
__device__ inline void up_fill_tables(uint32_t (*qt)[64], int q) {
    qt[0][threadIdx.x] = up_qt_packed(up_qt(q, 0, UP_ZZ[threadIdx.x]));
    qt[1][threadIdx.x] = up_qt_packed(up_qt(q, 1, UP_ZZ[threadIdx.x]));
    __syncthreads();
}
// the DC level in front of block j of a slice
__device__ inline int up_pred(const int16_t* c, const uint32_t* qt, int j) { return j ? up_level((int)c[-64], qt[0]) : 0; }

// The forward transform of the six 8 x 8 blocks in px (rows of UP_ROW words), by the macroblock's wave: rows in place, then columns into ob in
// zig-zag order.  Ends behind a barrier.
__device__ inline void up_forward_passes(int (*px)[8 * UP_ROW], int16_t (*ob)[64], int t) {
    const int blk = t >> 3, lane8 = t & 7;
    if (t < 48) {                                                 // along the rows: lane8 = the row, in place
        int* row = &px[blk][lane8 * UP_ROW];
        int x[8], o[8];
        for (int j = 0; j < 8; ++j) x[j] = row[j];
        for (int u = 0; u < 8; ++u) {
            int a = 512;
            for (int j = 0; j < 8; ++j) a += UP_M[u][j] * x[j];
            o[u] = a >> 10;
        }
        for (int u = 0; u < 8; ++u) row[u] = o[u];
    }
    __syncthreads();
    if (t < 48) {                                                 // along the columns: lane8 = u
        int x[8];
        for (int i = 0; i < 8; ++i) x[i] = px[blk][i * UP_ROW + lane8];
        for (int v = 0; v < 8; ++v) {
            int a = 32768;
            for (int i = 0; i < 8; ++i) a += UP_M[v][i] * x[i];
            ob[blk][UP_ZZ_INV[v * 8 + lane8]] = (int16_t)(a >> 16);
        }
    }
    __syncthreads();
}

// ob -> the macroblock's six blocks in the coefficient planes, 32 words per block
__device__ inline void up_store_coefs(const int16_t (*ob)[64], const UplinkGeom& g, int mby, int mbx, int16_t* coefs, int t) {
    const int mbw = g.W >> 4;
    const int cidx = mby * mbw + mbx;
    for (int i = t; i < 6 * 32; i += 64) {                        // 32 words per block
        const int b = i >> 5, wd = i & 31;
        const int64_t dst = b < 4 ? (int64_t)(2 * mby + (b >> 1)) * (g.W >> 3) + 2 * mbx + (b & 1) : (int64_t)g.nb[0] + (b - 4) * (int64_t)g.nb[1] + cidx;
        reinterpret_cast<uint32_t*>(coefs + dst * 64)[wd] = reinterpret_cast<const uint32_t*>(ob[b])[wd];
    }
}

// the byte counts of one slice at the 100 qualities: thread q - 1 of 128 writes out[(q - 1) * stride]; ZERO: a slice of zero levels counts 0
template <bool ZERO>
__device__ inline void up_slice_sizes(const int16_t* coefs, const SliceRef& s, uint32_t (*qtab)[100], uint32_t* cf, int32_t* out, int64_t stride) {
    const int chroma = s.plane > 0;
    for (int e = threadIdx.x; e < 6400; e += 128) {
        const int k = e / 100, q = e - 100 * k + 1;
        qtab[k][q - 1] = up_qt_packed(up_qt(q, chroma, UP_ZZ[k]));
    }
    const uint32_t* src = reinterpret_cast<const uint32_t*>(coefs + (int64_t)s.first * 64);
    for (int i = threadIdx.x; i < s.n * 32; i += 128) cf[i] = src[i];
    __syncthreads();
    const int q = threadIdx.x;
    if (q >= 100) return;
    int bits = 0, pred = 0;
    for (int b = 0; b < s.n; ++b) {
        const uint32_t* c = cf + b * 32;
        const int dc = up_level((int)(int16_t)c[0], qtab[0][q]), d = dc - pred;
        pred = dc;
        bits += 1 + (d ? up_code_bits(up_se_value(d)) : 1);
        int run = 0;
        for (int k = 1; k < 64; ++k) {
            const int coef = (int)(int16_t)(c[k >> 1] >> (16 * (k & 1)));        // the same word in every lane
            const int l = coef ? up_level_abs(coef, qtab[k][q]) : 0;
            if (!l) { ++run; continue; }
            bits += up_code_bits((uint32_t)run + 2u) + up_code_bits(2u * (uint32_t)l);
            run = 0;
        }
    }
    out[(int64_t)q * stride] = ZERO && bits == 2 * s.n ? 0 : (bits + 7) >> 3;
}

// sizes[blockIdx.x] = header + table + the bytes of the ns slices of quality blockIdx.x + 1
__device__ inline void up_totals(const int32_t* table, int ns, int64_t* sizes, int64_t* sh) {
    int64_t mine = 0;
    for (int s = threadIdx.x; s < ns; s += BLOCK_SCAN_THREADS) mine += table[(int64_t)blockIdx.x * ns + s];
    const int64_t total = block_sum(mine, sh);
    if (threadIdx.x == 0) sizes[blockIdx.x] = 16 + 2 * (int64_t)ns + total;
}

// one block: exclusive scan of the ns lengths; the size; AMS_UPLINK_NO_ROOM or header ("AU", kind, '1') and table
__device__ inline void up_encode_scan(int32_t* lens, int ns, int H, int W, int q, char kind, uint8_t* payload, int64_t cap, int64_t* bytes_out,
                                      int32_t* status, int64_t* sh) {
    const int chunk = (ns + BLOCK_SCAN_THREADS - 1) / BLOCK_SCAN_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < ns ? s0 + chunk : ns;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += lens[s];
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh), need = 16 + 2 * (int64_t)ns + total;
    const bool ok = need <= cap;                                 // all or nothing: the same for every thread
    for (int s = s0; s < s1; ++s) {
        const int32_t len = lens[s];
        lens[s] = (int32_t)run;
        run += len;
        if (ok) { payload[16 + 2 * s] = (uint8_t)len; payload[17 + 2 * s] = (uint8_t)(len >> 8); }
    }
    if (threadIdx.x == 0) {
        lens[ns] = (int32_t)total;
        *bytes_out = need;
        *status = ok ? AMS_UPLINK_OK : AMS_UPLINK_NO_ROOM;
        if (ok) {
            const uint8_t h[16] = {'A', 'U', (uint8_t)kind, '1', (uint8_t)H, (uint8_t)(H >> 8), (uint8_t)W, (uint8_t)(W >> 8), (uint8_t)q, 0, 0, 0,
                                   (uint8_t)need, (uint8_t)(need >> 8), (uint8_t)(need >> 16), (uint8_t)(need >> 24)};
            for (int i = 0; i < 16; ++i) payload[i] = h[i];
        }
    }
}

// one block: header of `kind`, table sum, scan of the ns lengths into offs -> status
__device__ inline void up_decode_scan(const uint8_t* payload, int64_t bytes, int H, int W, int ns, char kind, int32_t* offs, int32_t* status,
                                      int64_t* sh, int* header_ok) {
    const int64_t first = 16 + 2 * (int64_t)ns;                  // the first slice's byte
    if (threadIdx.x == 0) {
        bool ok = bytes >= first;                                // header and table lie inside what was handed in
        if (ok) {
            ok = payload[0] == 'A' && payload[1] == 'U' && payload[2] == (uint8_t)kind && payload[3] == '1' && (int)load_u16(payload + 4) == H &&
                 (int)load_u16(payload + 6) == W && payload[8] >= 1 && payload[8] <= 100 && !payload[9] && !payload[10] && !payload[11] &&
                 (int64_t)load_u32(payload + 12) == bytes;
        }
        *header_ok = ok;
        if (!ok) *status = AMS_UPLINK_BAD_HEADER;
    }
    __syncthreads();
    if (!*header_ok) return;
    const int chunk = (ns + BLOCK_SCAN_THREADS - 1) / BLOCK_SCAN_THREADS;
    const int s0 = (int)threadIdx.x * chunk, s1 = s0 + chunk < ns ? s0 + chunk : ns;
    int64_t mine = 0;
    for (int s = s0; s < s1; ++s) mine += load_u16(payload + 16 + 2 * s);
    int64_t run = block_exclusive_scan(mine, sh);
    const int64_t total = block_sum(mine, sh);
    const bool ok = first + total == bytes;
    if (ok)
        for (int s = s0; s < s1; ++s) { offs[s] = (int32_t)run; run += load_u16(payload + 16 + 2 * s); }
    if (threadIdx.x == 0) {
        if (ok) offs[ns] = (int32_t)total;
        *status = ok ? AMS_UPLINK_OK : AMS_UPLINK_BAD_TABLE;
    }
}

// The macroblock's dequantised coefficients into px, natural order, clamped to +-2047 (thread t = zig-zag position t of each block)
__device__ inline void up_dequantise(int (*px)[8 * UP_ROW], const int16_t* levels, const UplinkGeom& g, int q, int mby, int mbx, int t) {
    const int mbw = g.W >> 4, cidx = mby * mbw + mbx;
    const int nat = UP_ZZ[t], qt0 = up_qt(q, 0, nat), qt1 = up_qt(q, 1, nat);
    for (int b = 0; b < 6; ++b) {
        const int64_t src = b < 4 ? (int64_t)(2 * mby + (b >> 1)) * (g.W >> 3) + 2 * mbx + (b & 1) : (int64_t)g.nb[0] + (b - 4) * (int64_t)g.nb[1] + cidx;
        const int c = (int)levels[src * 64 + t] * (b < 4 ? qt0 : qt1);
        px[b][(nat >> 3) * UP_ROW + (nat & 7)] = c < -2047 ? -2047 : c > 2047 ? 2047 : c;
    }
}

// The inverse transform of the six blocks in px, in place, between barriers.  PIXELS: + 128 and the clamp to 0 .. 255 (AUC1); else the bare
// residual (AUP1)
template <bool PIXELS>
__device__ inline void up_inverse_passes(int (*px)[8 * UP_ROW], int t) {
    __syncthreads();
    const int blk = t >> 3, lane8 = t & 7;
    if (t < 48) {                                                 // along the columns with M transposed: lane8 = u, in place
        int x[8], o[8];
        for (int v = 0; v < 8; ++v) x[v] = px[blk][v * UP_ROW + lane8];
        for (int i = 0; i < 8; ++i) {
            int a = 512;
            for (int v = 0; v < 8; ++v) a += UP_M[v][i] * x[v];
            o[i] = a >> 10;
        }
        for (int i = 0; i < 8; ++i) px[blk][i * UP_ROW + lane8] = o[i];
    }
    __syncthreads();
    if (t < 48) {                                                 // along the rows: lane8 = the row, in place
        int* row = &px[blk][lane8 * UP_ROW];
        int x[8], o[8];
        for (int u = 0; u < 8; ++u) x[u] = row[u];
        for (int j = 0; j < 8; ++j) {
            int a = 32768;
            for (int u = 0; u < 8; ++u) a += UP_M[u][j] * x[u];
            o[j] = PIXELS ? clamp255((a >> 16) + 128) : a >> 16;
        }
        for (int j = 0; j < 8; ++j) row[j] = o[j];
    }
    __syncthreads();
}

// The macroblock's pixels in px (Y in blocks 0 .. 3, Cb and Cr in 4 and 5, each lane its own 2 x 2 and chroma sample) -> RGB
__device__ inline void up_write_rgb(const int (*px)[8 * UP_ROW], const UplinkGeom& g, int mby, int mbx, uint8_t* frame, int t) {
    const int qy = t >> 3, qx = t & 7;
    const int cb = px[4][qy * UP_ROW + qx] - 128, cr = px[5][qy * UP_ROW + qx] - 128;
    const int dr = (91881 * cr + 32768) >> 16, dg = (22554 * cb + 46802 * cr + 32768) >> 16, db = (116130 * cb + 32768) >> 16;
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * qy + dy;
        uint8_t* p = frame + ((int64_t)(16 * mby + y) * g.W + 16 * mbx + 2 * qx) * 3;
        for (int dx = 0; dx < 2; ++dx) {
            const int x = 2 * qx + dx, yy = px[(y >> 3) * 2 + (x >> 3)][(y & 7) * UP_ROW + (x & 7)];
            p[3 * dx] = (uint8_t)clamp255(yy + dr);
            p[3 * dx + 1] = (uint8_t)clamp255(yy - dg);
            p[3 * dx + 2] = (uint8_t)clamp255(yy + db);
        }
    }
}

// a slice's bits in order; bytes beyond the slice read as zeros and are never loaded
struct BitReader {
    const uint8_t* p;
    int len, next = 0, have = 0;               // next: the next byte to load; have: valid bits at the top of buf
    int64_t pos = 0;                           // bits consumed
    uint64_t buf = 0;
    __device__ BitReader(const uint8_t* data, int n) : p(data), len(n) {}
    __device__ void fill() {
        while (have <= 56 && next < len) { buf |= (uint64_t)p[next++] << (56 - have); have += 8; }
    }
    __device__ int64_t left() const { return 8 * (int64_t)len - pos; }
    __device__ void skip(int n) { buf <<= n; have -= n; pos += n; }
    // ue(v) -> v, or a negative status: no 1 among the next 17 bits = a level beyond every bound, unless the slice ends first
    __device__ int ue() {
        fill();
        const int64_t rest = left();
        const int zeros = buf ? __clzll((long long)buf) : 64;
        if (zeros > 16 || zeros >= rest) return rest > 16 && zeros > 16 ? -AMS_UPLINK_BAD_LEVEL : -AMS_UPLINK_BAD_OVERRUN;
        if (2 * zeros + 1 > rest) return -AMS_UPLINK_BAD_OVERRUN;
        const int v = (int)(buf >> (63 - 2 * zeros)) - 1;
        skip(2 * zeros + 1);
        return v;
    }
};

// the first violation in reading order, or AMS_UPLINK_OK; lv = the slice's levels, 64 per block, zeroed here
__device__ inline int parse_slice(const uint8_t* data, int len, int nblocks, int16_t* lv) {
    BitReader r(data, len);
    int pred = 0;
    for (int b = 0; b < nblocks; ++b, lv += 64) {
        for (int i = 0; i < 8; ++i) reinterpret_cast<uint4*>(lv)[i] = make_uint4(0, 0, 0, 0);
        int v = r.ue();
        if (v < 0) return -v;
        const int dc = pred + ((v & 1) ? (v + 1) >> 1 : -(v >> 1));
        if (dc > 2047 || dc < -2047) return AMS_UPLINK_BAD_LEVEL;
        lv[0] = (int16_t)dc;
        pred = dc;
        for (int k = 0;;) {
            v = r.ue();
            if (v < 0) return -v;
            if (v == 0) break;
            k += v;
            if (k > 63) return AMS_UPLINK_BAD_POSITION;
            v = r.ue();
            if (v < 0) return -v;
            if (v == 0) return AMS_UPLINK_BAD_ZERO_LEVEL;
            const int l = (v & 1) ? (v + 1) >> 1 : -(v >> 1);
            if (l > 2047 || l < -2047) return AMS_UPLINK_BAD_LEVEL;
            lv[k] = (int16_t)l;
        }
    }
    // the last block ends inside the last byte, and what is left of that byte is zero
    r.fill();
    if ((r.pos + 7) >> 3 != len || (r.left() > 0 && (r.buf >> (64 - r.left())) != 0)) return AMS_UPLINK_BAD_SLICE_END;
    return AMS_UPLINK_OK;
}

}  // namespace

}  // namespace ams
