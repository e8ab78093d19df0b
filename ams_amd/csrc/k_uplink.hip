// The uplink frame codec AUC1 (include/ams_hip.h states the format; tests/uplink_ref.py is its NumPy restatement, byte for byte): the edge
// encodes a sampled frame on the device at a byte budget, the server decodes it on the device.  Integer arithmetic throughout.  What the
// predicted frame AUP1 (k_uplink_inter.hip) shares with it is device code in uplink_common.hpp; the kernels here are AUC1's alone.
//
// Encoder scratch (bytes): [int16 coefficients, zig-zag order, 64 per block, planes Y Cb Cr][int32 slice lengths -> offsets, slices + 1]
//                          [int32 byte counts, 100 qualities x slices]
//   uplink_transform_kernel   one wave per 16 x 16 macroblock: colour and 2 x 2 chroma mean per lane, the six 8 x 8 blocks in LDS (rows of 9
//                             words: the row pass and the column pass both read without bank conflicts), coefficients out in zig-zag order
//   uplink_sizes_kernel       one block per slice, one thread per quality: the slice's coefficients (every lane reads the same word) and the
//                             100 tables as [coefficient][quality] (lanes read consecutive words) in LDS; the division by the table entry is a
//                             multiplication by ceil(2^20 / qt), exact for numerators below 4096 (tests/test_uplink_ref_cpu.py)
//   uplink_totals_kernel      one block per quality: header + table + the slices' bytes -> sizes[q - 1]
//   uplink_lengths_kernel     one quality: a thread per 8 x 8 block, half a wave per slice -> the slice's bytes
//   uplink_encode_scan_kernel one block: exclusive scan of the lengths; the size; AMS_UPLINK_NO_ROOM or header and table
//   uplink_write_kernel       nothing unless the status is OK: half a wave per slice; each lane counts its block's bits, the lanes scan them,
//                             each ORs its codes into the slice's LDS image at its bit offset, and the image leaves as bytes (the slice
//                             starts at any address)
// Decoder scratch (bytes): [int16 levels, zig-zag order, 64 per block][int32 slice offsets, slices + 1]
//   uplink_decode_scan_kernel one block: header, table sum, scan -> status
//   uplink_parse_kernel       nothing unless OK: a thread per slice reads its bits in order and raises the status at the first violation
//   uplink_rebuild_kernel     nothing unless OK: one wave per macroblock: dequantise, clamp, inverse transform, colour -> RGB
#include "uplink_common.hpp"

namespace ams {

// ------------------------------------------------------------------------------------------------------------------- encoder
__global__ void __launch_bounds__(64) uplink_transform_kernel(const uint8_t* frame, UplinkGeom g, int16_t* coefs) {
    __shared__ int px[6][8 * UP_ROW];
    __shared__ int16_t ob[6][64];
    const int mbw = g.W >> 4, mby = blockIdx.x / mbw, mbx = blockIdx.x - mby * mbw;
    const int t = threadIdx.x, qy = t >> 3, qx = t & 7;
    int cb = 2, cr = 2;
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * qy + dy;
        const uint8_t* p = frame + ((int64_t)(16 * mby + y) * g.W + 16 * mbx + 2 * qx) * 3;
        for (int dx = 0; dx < 2; ++dx) {
            const int x = 2 * qx + dx, r = p[3 * dx], gr = p[3 * dx + 1], b = p[3 * dx + 2];
            const int yy = up_luma(r, gr, b);
            cb += up_cb(r, gr, b);
            cr += up_cr(r, gr, b);
            px[(y >> 3) * 2 + (x >> 3)][(y & 7) * UP_ROW + (x & 7)] = yy - 128;
        }
    }
    px[4][qy * UP_ROW + qx] = (cb >> 2) - 128;
    px[5][qy * UP_ROW + qx] = (cr >> 2) - 128;
    __syncthreads();
    up_forward_passes(px, ob, t);
    up_store_coefs(ob, g, mby, mbx, coefs, t);
}

__global__ void __launch_bounds__(128) uplink_sizes_kernel(const int16_t* coefs, UplinkGeom g, int32_t* table) {
    __shared__ uint32_t qtab[64][100];
    __shared__ uint32_t cf[UP_SLICE * 32];
    up_slice_sizes<false>(coefs, slice_ref(g, blockIdx.x), qtab, cf, table + blockIdx.x, g.nslices);
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_totals_kernel(const int32_t* table, UplinkGeom g, int64_t* sizes) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    up_totals(table, g.nslices, sizes, sh);
}

__global__ void __launch_bounds__(64) uplink_lengths_kernel(const int16_t* coefs, UplinkGeom g, int q, int32_t* lens) {
    __shared__ uint32_t qt[2][64];
    up_fill_tables(qt, q);
    const int sidx = 2 * blockIdx.x + (threadIdx.x >> 5), j = threadIdx.x & 31;
    int bits = 0;
    if (sidx < g.nslices) {
        const SliceRef s = slice_ref(g, sidx);
        if (j < s.n) {
            const int16_t* c = coefs + (int64_t)(s.first + j) * 64;
            CountSink sink;
            walk_block(c, qt[s.plane > 0], up_pred(c, qt[s.plane > 0], j), sink);
            bits = sink.bits;
        }
    }
    for (int o = 16; o > 0; o >>= 1) bits += __shfl_xor(bits, o, 32);
    if (j == 0 && sidx < g.nslices) lens[sidx] = (bits + 7) >> 3;
}

__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_encode_scan_kernel(int32_t* lens, UplinkGeom g, int q, uint8_t* payload, int64_t cap,
                                                                                int64_t* bytes_out, int32_t* status) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    up_encode_scan(lens, g.nslices, g.H, g.W, q, 'C', payload, cap, bytes_out, status, sh);
}

__global__ void __launch_bounds__(64) uplink_write_kernel(const int16_t* coefs, UplinkGeom g, int q, const int32_t* offs, const int32_t* status,
                                                          uint8_t* payload, int64_t cap) {
    __shared__ uint32_t qt[2][64];
    __shared__ uint32_t img[2][UP_SLICE_WORDS];
    if (*status != AMS_UPLINK_OK) return;                        // all or nothing (the same word for every thread)
    up_fill_tables(qt, q);
    const int half = threadIdx.x >> 5, sidx = 2 * blockIdx.x + half, j = threadIdx.x & 31;
    const bool live = sidx < g.nslices;
    int len = 0;
    int64_t at = 0;
    if (live) {
        at = offs[sidx];
        len = offs[sidx + 1] - offs[sidx];
        len = len < 0 ? 0 : len > 4 * UP_SLICE_WORDS ? 4 * UP_SLICE_WORDS : len;
    }
    for (int w = j; w < (len + 3) >> 2; w += 32) img[half][w] = 0;
    __syncthreads();
    int bits = 0, pred = 0;
    const int16_t* c = nullptr;
    const uint32_t* table = nullptr;
    if (live) {
        const SliceRef s = slice_ref(g, sidx);
        if (j < s.n) {
            c = coefs + (int64_t)(s.first + j) * 64;
            table = qt[s.plane > 0];
            pred = up_pred(c, table, j);
            CountSink count;
            walk_block(c, table, pred, count);
            bits = count.bits;
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
    }
    __syncthreads();
    const int64_t base = 16 + 2 * (int64_t)g.nslices + at;
    for (int i = j; i < len; i += 32)
        if (base + i < cap) payload[base + i] = (uint8_t)(img[half][i >> 2] >> (24 - 8 * (i & 3)));      // (implied by the status)
}

// ------------------------------------------------------------------------------------------------------------------- decoder
__global__ void __launch_bounds__(BLOCK_SCAN_THREADS) uplink_decode_scan_kernel(const uint8_t* payload, int64_t bytes, UplinkGeom g, int32_t* offs,
                                                                                int32_t* status) {
    __shared__ int64_t sh[BLOCK_SCAN_THREADS];
    __shared__ int header_ok;
    up_decode_scan(payload, bytes, g.H, g.W, g.nslices, 'C', offs, status, sh, &header_ok);
}

__global__ void __launch_bounds__(64) uplink_parse_kernel(const uint8_t* payload, UplinkGeom g, const int32_t* offs, int16_t* levels, int32_t* status) {
    if (*status != AMS_UPLINK_OK) return;                        // header or table refused: the offsets were never written
    const int sidx = blockIdx.x * 64 + threadIdx.x;
    if (sidx >= g.nslices) return;
    const SliceRef s = slice_ref(g, sidx);
    const int st = parse_slice(payload + 16 + 2 * (int64_t)g.nslices + offs[sidx], offs[sidx + 1] - offs[sidx], s.n, levels + (int64_t)s.first * 64);
    if (st != AMS_UPLINK_OK) atomicMax(status, st);
}

__global__ void __launch_bounds__(64) uplink_rebuild_kernel(const uint8_t* payload, UplinkGeom g, const int16_t* levels, const int32_t* status,
                                                            uint8_t* frame) {
    __shared__ int px[6][8 * UP_ROW];
    if (*status != AMS_UPLINK_OK) return;                        // all or nothing
    const int q = payload[8];
    const int mbw = g.W >> 4, mby = blockIdx.x / mbw, mbx = blockIdx.x - mby * mbw;
    const int t = threadIdx.x;
    up_dequantise(px, levels, g, q, mby, mbx, t);
    up_inverse_passes<true>(px, t);
    up_write_rgb(px, g, mby, mbx, frame, t);
}

// ---------------------------------------------------------------------------------------------------------------------- host
bool uplink_shape_ok(int H, int W) { return H % 16 == 0 && W % 16 == 0 && H >= 16 && H <= 4096 && W >= 16 && W <= 4096; }

UplinkGeom uplink_geom(int H, int W) {
    UplinkGeom g;
    g.H = H;
    g.W = W;
    g.nb[0] = (H / 8) * (W / 8);
    g.nb[1] = g.nb[2] = (H / 16) * (W / 16);
    g.nblocks = g.nslices = 0;
    for (int p = 0; p < 3; ++p) {
        g.ns[p] = (g.nb[p] + UP_SLICE - 1) / UP_SLICE;
        g.nblocks += g.nb[p];
        g.nslices += g.ns[p];
    }
    return g;
}

static size_t round16(size_t n) { return (n + 15) / 16 * 16; }
static size_t up_offsets_at(const UplinkGeom& g) { return (size_t)g.nblocks * 128; }
static size_t up_table_at(const UplinkGeom& g) { return up_offsets_at(g) + round16(4 * ((size_t)g.nslices + 1)); }

int64_t uplink_max_bytes(int H, int W) {
    const UplinkGeom g = uplink_geom(H, W);
    return 16 + 2 * (int64_t)g.nslices + 208 * (int64_t)g.nblocks;
}
size_t uplink_encode_scratch_bytes(int H, int W) {
    const UplinkGeom g = uplink_geom(H, W);
    return up_table_at(g) + 400 * (size_t)g.nslices;
}
size_t uplink_decode_scratch_bytes(int H, int W) { return up_table_at(uplink_geom(H, W)); }

int launch_uplink_transform(const uint8_t* frame, int H, int W, void* scratch, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    hipLaunchKernelGGL(uplink_transform_kernel, dim3((H / 16) * (W / 16)), dim3(64), 0, st, frame, g, (int16_t*)scratch);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_size_table(void* scratch, int H, int W, int64_t* sizes, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    int32_t* table = reinterpret_cast<int32_t*>((char*)scratch + up_table_at(g));
    hipLaunchKernelGGL(uplink_sizes_kernel, dim3(g.nslices), dim3(128), 0, st, (const int16_t*)scratch, g, table);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_totals_kernel, dim3(100), dim3(BLOCK_SCAN_THREADS), 0, st, (const int32_t*)table, g, sizes);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_encode(void* scratch, int H, int W, int q, uint8_t* payload, int64_t cap, int64_t* bytes_out, int32_t* status, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    const int16_t* coefs = (const int16_t*)scratch;
    int32_t* lens = reinterpret_cast<int32_t*>((char*)scratch + up_offsets_at(g));
    hipLaunchKernelGGL(uplink_lengths_kernel, dim3((g.nslices + 1) / 2), dim3(64), 0, st, coefs, g, q, lens);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_encode_scan_kernel, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, st, lens, g, q, payload, cap, bytes_out, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_write_kernel, dim3((g.nslices + 1) / 2), dim3(64), 0, st, coefs, g, q, (const int32_t*)lens, (const int32_t*)status,
                       payload, cap);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

int launch_uplink_decode(const uint8_t* payload, int64_t bytes, int H, int W, uint8_t* frame, int32_t* status, void* scratch, hipStream_t st) {
    const UplinkGeom g = uplink_geom(H, W);
    int16_t* levels = (int16_t*)scratch;
    int32_t* offs = reinterpret_cast<int32_t*>((char*)scratch + up_offsets_at(g));
    hipLaunchKernelGGL(uplink_decode_scan_kernel, dim3(1), dim3(BLOCK_SCAN_THREADS), 0, st, payload, bytes, g, offs, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_parse_kernel, dim3((g.nslices + 63) / 64), dim3(64), 0, st, payload, g, (const int32_t*)offs, levels, status);
    AMS_CHECK_LAUNCH();
    hipLaunchKernelGGL(uplink_rebuild_kernel, dim3((H / 16) * (W / 16)), dim3(64), 0, st, payload, g, (const int16_t*)levels, (const int32_t*)status,
                       frame);
    AMS_CHECK_LAUNCH();
    return AMS_OK;
}

}  // namespace ams
