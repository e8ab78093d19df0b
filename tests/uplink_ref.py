"""NumPy oracle of the uplink frame codec AUC1 (ams_amd/csrc/k_uplink.hip, include/ams_hip.h): encoder, size table, rate rule and decoder
with every refusal.  All arithmetic is integer, so the device must agree byte for byte; this file is the format's executable definition.

Format (>> is an arithmetic shift; every colour and pixel result is clamped to 0 .. 255):
  frame    RGB uint8 [H, W, 3], H and W multiples of 16 in 16 .. 4096
  colour   Y = (19595 R + 38470 G + 7471 B + 32768) >> 16;  Cb = ((-11059 R - 21709 G + 32768 B + 32768) >> 16) + 128;
           Cr = ((32768 R - 27439 G - 5329 B + 32768) >> 16) + 128;  4:2:0: (a + b + c + d + 2) >> 2 over each 2 x 2
           back: R = Y + ((91881 (Cr-128) + 32768) >> 16);  G = Y - ((22554 (Cb-128) + 46802 (Cr-128) + 32768) >> 16);
           B = Y + ((116130 (Cb-128) + 32768) >> 16), chroma replicated 2 x 2
  blocks   8 x 8 of pixel - 128; M = rint(2^13 C), C the orthonormal DCT-II matrix; forward t = (M x + 512) >> 10 along the rows, then
           c = (M t + 32768) >> 16 along the columns; inverse with M transposed, columns first, + 128, clamp; the decoder clamps each
           dequantised coefficient to [-2047, 2047]
  quality  Annex K tables, s = q < 50 ? 5000 // q : 200 - 2 q, qt = clamp((base s + 50) // 100, 1, 255), level = sign(c) ((|c| + qt // 2) // qt)
  bits     ue(v) = v + 1 written in 2 floor(log2(v + 1)) + 1 bits, MSB first; se(v) = ue(2 v - 1 if v > 0 else -2 v); a block in zig-zag
           order: se(dc - pred), per non-zero AC ue(run + 1) se(level), then ue(0)
  slices   planes Y, Cb, Cr; 32 consecutive raster blocks of a plane (the last may be shorter); pred = the previous block's quantised DC in
           the slice, else 0; zero bits to a whole byte
  payload  "AUC1", u16 H, u16 W, u8 q, 0, 0, 0, u32 total bytes; u16 length per slice; the slices

Rate rule: the largest q in 1 .. 100 whose payload has at most `budget` bytes; none: q = 1 and fits = False.

How far the integer steps lie from the mathematics they restate (tests/test_uplink_ref_cpu.py asserts each), with dM = M - 2^13 C,
R1 = the largest row sum of |dM|, C1 = its largest column sum, A = the largest row (= column of the transpose) sum of |C|:
  forward transform against the f64 orthonormal DCT of x in [-128, 127]:
      the row pass is floor(8 Cx + dM x / 1024 + 1/2): e_t <= 1/2 + 128 R1 / 1024;
      the column pass is floor(C t / 8 + dM t / 65536 + 1/2) with t = 8 (Cx) + e, |t| <= 8 A 128 + e_t:
      FWD_BOUND = 1/2 + A e_t / 8 + R1 (1024 A + e_t) / 65536                                     (about 0.9; the extremes measure 0.65)
  colour against the f64 JFIF equations, both sides clamped (a contraction): 1/2 for the rounding shift + 255 x the summed distances of the
      16-bit constants from the real ones (COLOUR_BOUNDS; about 0.503 each); the 2 x 2 mean: 1/2
  the decoder against the same steps in f64 (real products, no rounding, the same clamps) for coefficients |c| <= cmax:
      columns e_1 = 1/2 + C1 cmax / 1024;  rows e_x = 1/2 + A e_1 / 8 + R1 (8 A cmax + e_1) / 65536  (idct_bound(cmax));
      R: 2.402 e_x + c_R;  G: 2.058272 e_x + c_G;  B: 2.772 e_x + c_B with c_* = 1/2 + 128 x the constants' distances (decode_bounds(cmax)).
"""
import numpy as np

MAGIC = b"AUC1"
SLICE_BLOCKS = 32
BLOCK_MAX_BITS = 25 + 63 * (3 + 23) + 1
OK, BAD_HEADER, BAD_TABLE, BAD_SLICE_END, BAD_POSITION, BAD_ZERO_LEVEL, BAD_LEVEL, BAD_OVERRUN, NO_ROOM = range(9)
MAX_PREFIX_ZEROS = 16              # a longer Exp-Golomb prefix is a value above 2^17 - 2: BAD_LEVEL

C8 = np.array([[np.sqrt((1.0 if u == 0 else 2.0) / 8.0) * np.cos((2 * j + 1) * u * np.pi / 16.0) for j in range(8)] for u in range(8)])
M = np.rint(C8 * 8192.0).astype(np.int64)
DM = M - C8 * 8192.0
R1, C1, A1 = np.abs(DM).sum(1).max(), np.abs(DM).sum(0).max(), np.abs(C8).sum(1).max()
_ET = 0.5 + 128.0 * R1 / 1024.0
FWD_BOUND = 0.5 + A1 * _ET / 8.0 + R1 * (1024.0 * A1 + _ET) / 65536.0

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101,
                      72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                       + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

# (16-bit constants, the real ones) of each colour equation
_FWD = {"Y": ((19595, 38470, 7471), (0.299, 0.587, 0.114)), "Cb": ((-11059, -21709, 32768), (-0.168736, -0.331264, 0.5)),
        "Cr": ((32768, -27439, -5329), (0.5, -0.418688, -0.081312))}
_INV = {"R": ((91881,), (1.402,)), "G": ((22554, 46802), (0.344136, 0.714136)), "B": ((116130,), (1.772,))}
COLOUR_BOUNDS = {k: 0.5 + 255.0 * sum(abs(i / 65536.0 - r) for i, r in zip(*v)) for k, v in _FWD.items()}
_INV_C = {k: 0.5 + 128.0 * sum(abs(i / 65536.0 - r) for i, r in zip(*v)) for k, v in _INV.items()}


def idct_bound(cmax):
    e1 = 0.5 + C1 * cmax / 1024.0
    return 0.5 + A1 * e1 / 8.0 + R1 * (8.0 * A1 * cmax + e1) / 65536.0


def decode_bounds(cmax):
    ex = idct_bound(cmax)
    return {"R": 2.402 * ex + _INV_C["R"], "G": (1 + 0.344136 + 0.714136) * ex + _INV_C["G"], "B": 2.772 * ex + _INV_C["B"]}


def shape_ok(H, W):
    return H % 16 == 0 and W % 16 == 0 and 16 <= H <= 4096 and 16 <= W <= 4096


def plane_blocks(H, W):
    """blocks of the planes Y, Cb, Cr"""
    return [(H // 8) * (W // 8), (H // 16) * (W // 16), (H // 16) * (W // 16)]


def slice_counts(H, W):
    return [(n + SLICE_BLOCKS - 1) // SLICE_BLOCKS for n in plane_blocks(H, W)]


def max_bytes(H, W):
    return 16 + 2 * sum(slice_counts(H, W)) + (BLOCK_MAX_BITS // 8) * sum(plane_blocks(H, W))


def quant_table(q, chroma):
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip(((BASE_CHROMA if chroma else BASE_LUMA) * s + 50) // 100, 1, 255)          # natural (row-major) order


# ---------------------------------------------------------------------------------------------------------------- colour
def rgb_to_ycc(frame):
    """uint8 [H, W, 3] -> int64 Y, Cb, Cr at full resolution"""
    r, g, b = (frame[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = ((-11059 * r - 21709 * g + 32768 * b + 32768) >> 16) + 128
    cr = ((32768 * r - 27439 * g - 5329 * b + 32768) >> 16) + 128
    return [np.clip(p, 0, 255) for p in (y, cb, cr)]


def subsample(p):
    return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2


def ycc_to_rgb(y, cb, cr):
    """int64 Y [H, W], Cb, Cr [H/2, W/2] -> uint8 [H, W, 3]"""
    cb = np.repeat(np.repeat(cb, 2, 0), 2, 1) - 128
    cr = np.repeat(np.repeat(cr, 2, 0), 2, 1) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y - ((22554 * cb + 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------- transform
def to_blocks(p):
    """[h, w] -> [blocks in raster order, 8, 8]"""
    h, w = p.shape
    return p.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)


def from_blocks(b, h, w):
    return b.reshape(h // 8, w // 8, 8, 8).transpose(0, 2, 1, 3).reshape(h, w)


def fdct(x):
    """int64 [n, 8, 8] of pixel - 128 -> coefficients [n, 8 (v), 8 (u)]"""
    t = (np.einsum("uj,nij->niu", M, x) + 512) >> 10
    return (np.einsum("vi,niu->nvu", M, t) + 32768) >> 16


def idct(c):
    """coefficients [n, 8, 8] -> pixels 0 .. 255"""
    t = (np.einsum("vi,nvu->niu", M, c) + 512) >> 10
    return np.clip(((np.einsum("uj,niu->nij", M, t) + 32768) >> 16) + 128, 0, 255)


def transform(frame):
    """-> the three planes' coefficients, int64 [blocks, 64] in zig-zag order: what the encoder's scratch holds"""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and shape_ok(*frame.shape[:2]), frame.shape
    y, cb, cr = rgb_to_ycc(frame)
    return [fdct(to_blocks(p) - 128).reshape(-1, 64)[:, ZIGZAG] for p in (y, subsample(cb), subsample(cr))]


def quantise(coefs, q, chroma):
    qt = quant_table(q, chroma)[ZIGZAG]
    return np.sign(coefs) * ((np.abs(coefs) + qt // 2) // qt)


# ---------------------------------------------------------------------------------------------------------- entropy code
_BITLEN = np.array([int(v).bit_length() for v in range(1 << 14)])


def _ue_bits(v):
    return 2 * _BITLEN[v + 1] - 1


def _se_map(v):
    return np.where(v > 0, 2 * v - 1, -2 * v)


def _dc_diff(levels):
    """levels [blocks, 64] of one plane -> dc - pred per block"""
    dc = levels[:, 0]
    pred = np.concatenate([[0], dc[:-1]])
    pred[::SLICE_BLOCKS] = 0
    return dc - pred


def block_bits(levels):
    """bits of every block of one plane"""
    n = len(levels)
    bits = _ue_bits(_se_map(_dc_diff(levels))) + 1
    k = np.arange(64)
    nz = levels != 0
    nz[:, 0] = True                                              # the DC position is where the first run starts
    last = np.maximum.accumulate(np.where(nz, k, 0), axis=1)
    prev = np.concatenate([np.zeros((n, 1), np.int64), last[:, :-1]], 1)
    ac = (levels != 0) & (k > 0)
    per = _ue_bits(np.where(ac, k - prev, 1)) + _ue_bits(_se_map(np.where(ac, levels, 1)))
    return bits + np.where(ac, per, 0).sum(1)


def slice_bytes(levels):
    """byte length of every slice of one plane"""
    bits = block_bits(levels)
    starts = np.arange(0, len(bits), SLICE_BLOCKS)
    return (np.add.reduceat(bits, starts) + 7) // 8


def payload_size(planes, q):
    lens = np.concatenate([slice_bytes(quantise(c, q, i > 0)) for i, c in enumerate(planes)])
    return 16 + 2 * len(lens) + int(lens.sum())


def size_table(frame):
    """int64 [100]: the exact payload bytes at q = 1 .. 100"""
    planes = transform(frame)
    return np.array([payload_size(planes, q) for q in range(1, 101)], np.int64)


def choose_quality(sizes, budget):
    """the rate rule over the 100 sizes -> (q, fits)"""
    fit = np.nonzero(np.asarray(sizes) <= budget)[0]
    return (int(fit[-1]) + 1, True) if len(fit) else (1, False)


def _symbols(levels):
    """one slice's (value, bits) pairs: value written in `bits` bits"""
    vals = []
    pred = 0
    for blk in levels:
        vals.append(_se_map(blk[0] - pred) + 1)
        pred = blk[0]
        pos = np.nonzero(blk[1:])[0] + 1
        if len(pos):
            runs = np.diff(np.concatenate([[0], pos]))           # run + 1
            ac = np.empty(2 * len(pos), np.int64)
            ac[0::2] = runs + 1
            ac[1::2] = _se_map(blk[pos]) + 1
            vals.append(ac)
        vals.append(1)                                           # ue(0)
    v = np.concatenate([np.atleast_1d(x) for x in vals]).astype(np.int64)
    return v, 2 * _BITLEN[v] - 1


def _pack(values, nbits):
    total = int(nbits.sum())
    ends = np.cumsum(nbits)
    out = np.zeros((total + 7) // 8 * 8, np.uint8)
    sym = np.repeat(np.arange(len(values)), nbits)
    shift = ends[sym] - 1 - np.arange(total)                     # the bit of the symbol's value at each position
    out[:total] = (values[sym] >> shift) & 1
    return np.packbits(out).tobytes()


def encode(frame, q, planes=None):
    """-> the payload at quality q"""
    assert 1 <= q <= 100
    H, W = np.asarray(frame).shape[:2]
    planes = transform(frame) if planes is None else planes
    slices = []
    for i, c in enumerate(planes):
        lv = quantise(c, q, i > 0)
        slices += [_pack(*_symbols(lv[s:s + SLICE_BLOCKS])) for s in range(0, len(lv), SLICE_BLOCKS)]
    table = np.array([len(s) for s in slices], "<u2").tobytes()
    total = 16 + len(table) + sum(len(s) for s in slices)
    header = MAGIC + np.array([H, W], "<u2").tobytes() + bytes([q, 0, 0, 0]) + np.array([total], "<u4").tobytes()
    return header + table + b"".join(slices)


def encode_to_budget(frame, budget):
    """-> (payload, q, fits, the 100 sizes)"""
    planes = transform(frame)
    sizes = np.array([payload_size(planes, q) for q in range(1, 101)], np.int64)
    q, fits = choose_quality(sizes, budget)
    return encode(frame, q, planes), q, fits, sizes


# --------------------------------------------------------------------------------------------------------------- decoder
class Refused(ValueError):
    def __init__(self, status):
        ValueError.__init__(self, "uplink payload refused: status %d" % status)
        self.status = status


def _parse_slice(data, nblocks):
    """-> (levels [nblocks, 64] in zig-zag order, status): the first violation in reading order ends the slice"""
    bits = "".join("{:08b}".format(b) for b in data)
    end = len(bits)
    pos = 0
    levels = np.zeros((nblocks, 64), np.int64)

    def ue():
        nonlocal pos
        one = bits.find("1", pos, pos + MAX_PREFIX_ZEROS + 1)
        if one < 0:                                              # no 1 among the next 17 bits, or among those that are left
            return None, BAD_LEVEL if end - pos > MAX_PREFIX_ZEROS else BAD_OVERRUN
        zeros = one - pos
        if one + zeros + 1 > end:
            return None, BAD_OVERRUN
        v = int(bits[one:one + zeros + 1], 2) - 1
        pos = one + zeros + 1
        return v, OK

    def se():
        v, st = ue()
        if st:
            return None, st
        return ((v + 1) // 2 if v & 1 else -(v // 2)), OK

    pred = 0
    for b in range(nblocks):
        d, st = se()
        if st:
            return levels, st
        dc = pred + d
        if abs(dc) > 2047:
            return levels, BAD_LEVEL
        levels[b, 0] = pred = dc
        k = 0
        while True:
            v, st = ue()
            if st:
                return levels, st
            if v == 0:
                break
            k += v
            if k > 63:
                return levels, BAD_POSITION
            lv, st = se()
            if st:
                return levels, st
            if lv == 0:
                return levels, BAD_ZERO_LEVEL
            if abs(lv) > 2047:
                return levels, BAD_LEVEL
            levels[b, k] = lv
    if (pos + 7) // 8 != len(data) or "1" in bits[pos:]:
        return levels, BAD_SLICE_END
    return levels, OK


def parse(payload, H, W):
    """-> (q, the three planes' levels [blocks, 64] zig-zag, status).  Header and table first, in the order of the status codes; then
    every slice on its own, the largest code of the malformed ones."""
    p = bytes(payload)
    ns = slice_counts(H, W)
    if len(p) < 16 or p[:4] != MAGIC:
        return 0, None, BAD_HEADER
    h, w = np.frombuffer(p[4:8], "<u2")
    q = p[8]
    total = int(np.frombuffer(p[12:16], "<u4")[0])
    if (h, w) != (H, W) or not 1 <= q <= 100 or p[9:12] != b"\0\0\0" or total != len(p) or total < 16 + 2 * sum(ns):
        return 0, None, BAD_HEADER
    lens = np.frombuffer(p[16:16 + 2 * sum(ns)], "<u2").astype(np.int64)
    if 16 + 2 * sum(ns) + int(lens.sum()) != total:
        return q, None, BAD_TABLE
    offs = 16 + 2 * sum(ns) + np.concatenate([[0], np.cumsum(lens)])
    planes, status, s = [], OK, 0
    for nb, n in zip(plane_blocks(H, W), ns):
        lv = np.zeros((nb, 64), np.int64)
        for j in range(n):
            b0 = j * SLICE_BLOCKS
            part, st = _parse_slice(p[offs[s]:offs[s + 1]], min(SLICE_BLOCKS, nb - b0))
            lv[b0:b0 + len(part)] = part
            status = max(status, st)
            s += 1
        planes.append(lv)
    return q, planes, status


def dequantise(levels, q, chroma):
    """zig-zag levels -> natural-order coefficients [blocks, 8, 8], clamped to +-2047"""
    c = np.zeros_like(levels)
    c[:, ZIGZAG] = levels * quant_table(q, chroma)[ZIGZAG]
    return np.clip(c, -2047, 2047).reshape(-1, 8, 8)


def reconstruct(planes, q, H, W):
    px = [from_blocks(idct(dequantise(lv, q, i > 0)), H >> (i > 0), W >> (i > 0)) for i, lv in enumerate(planes)]
    return ycc_to_rgb(*px)


def decode(payload, H, W):
    """-> uint8 [H, W, 3], or Refused with the status"""
    q, planes, status = parse(payload, H, W)
    if status != OK:
        raise Refused(status)
    return reconstruct(planes, q, H, W)


def header_size(payload):
    """(H, W) as the header states them (what a caller reads before it can size the output)"""
    h, w = np.frombuffer(bytes(payload[4:8]), "<u2")
    return int(h), int(w)


# ------------------------------------------------------------------------------------------- the same decode in real numbers
def reconstruct_f64(planes, q, H, W):
    """The decoder's steps with real products and no rounding, the clamps kept: what decode_bounds() is a distance from."""
    px = []
    for i, lv in enumerate(planes):
        c = dequantise(lv, q, i > 0).astype(np.float64)
        x = np.einsum("vi,nvu,uj->nij", C8, c, C8) + 128.0
        px.append(from_blocks(np.clip(x, 0, 255), H >> (i > 0), W >> (i > 0)))
    y = px[0]
    cb = np.repeat(np.repeat(px[1], 2, 0), 2, 1) - 128.0
    cr = np.repeat(np.repeat(px[2], 2, 0), 2, 1) - 128.0
    return np.clip(np.stack([y + 1.402 * cr, y - 0.344136 * cb - 0.714136 * cr, y + 1.772 * cb], -1), 0, 255)


# ------------------------------------------------------------------------------------------------------------- test data
def frames(H, W, seed=0):
    """the contents the tests run: name -> uint8 [H, W, 3]"""
    from ams_amd import synth
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    prim = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 0], [0, 255, 255], [255, 0, 255], [255, 255, 255], [0, 0, 0]], np.uint8)
    clip = synth.SyntheticVideo(max(H, W // 2), 1, [0, 1, 2, 10, 11, 13], seed=3).frame(0)[0]
    return {
        "constant": np.full((H, W, 3), 93, np.uint8),
        "noise": rng.randint(0, 256, (H, W, 3)).astype(np.uint8),
        "primaries": prim[((yy // 4) * 3 + xx // 4) % 8],
        "checker": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, 2),
        "clip": np.ascontiguousarray(clip[:H, :W]),
    }


def malformed(payload, H, W):
    """name -> (bytes, the status the decoder must give) over one well-formed payload"""
    p = bytearray(payload)
    ns = sum(slice_counts(H, W))
    first = 16 + 2 * ns

    def edit(i, v, base=p):
        b = bytearray(base)
        b[i] = v
        return bytes(b)

    def grown(extra):
        """one more byte behind the first slice, lengths and total kept consistent"""
        l0 = int(np.frombuffer(bytes(p[16:18]), "<u2")[0])
        b = bytearray(p[:first + l0] + bytes([extra]) + p[first + l0:])
        b[16:18] = np.array([l0 + 1], "<u2").tobytes()
        b[12:16] = np.array([len(b)], "<u4").tobytes()
        return bytes(b)

    def first_slice(bits):
        """the first slice replaced by `bits` (a '0'/'1' string, padded with zeros), the rest of the payload kept"""
        l0 = int(np.frombuffer(bytes(p[16:18]), "<u2")[0])
        s = np.packbits(np.array([int(c) for c in bits + "0" * (-len(bits) % 8)], np.uint8)).tobytes()
        b = bytearray(p[:first] + s + p[first + l0:])
        b[16:18] = np.array([len(s)], "<u2").tobytes()
        b[12:16] = np.array([len(b)], "<u4").tobytes()
        return bytes(b)

    nb0 = min(SLICE_BLOCKS, plane_blocks(H, W)[0])
    flat = "11" * nb0                                            # every block: se(0), ue(0); a whole number of bytes
    odd = "0101" + "11" * (nb0 - 1)                              # the first DC is 1: two bits into a byte, six bits of padding
    ac63 = "1" + "0000001000000" + "010"                         # DC 0, then run 62: a level of 1 at position 63
    big = "0" * 12 + "1" + "0" * 12                              # ue(4095) = se(2048)
    cases = {
        "magic": (edit(0, ord("B")), BAD_HEADER),
        "height": (edit(4, (p[4] + 16) & 255), BAD_HEADER),
        "width": (edit(6, (p[6] + 16) & 255), BAD_HEADER),
        "quality_0": (edit(8, 0), BAD_HEADER),
        "quality_101": (edit(8, 101), BAD_HEADER),
        "reserved": (edit(10, 1), BAD_HEADER),
        "total": (edit(12, (p[12] + 1) & 255), BAD_HEADER),
        "truncated": (bytes(p[:-1]), BAD_HEADER),
        "short_header": (bytes(p[:9]), BAD_HEADER),
        "no_table": (bytes(p[:16]), BAD_HEADER),
        "empty": (b"", BAD_HEADER),
        "table_sum": (edit(16, (p[16] + 1) & 255), BAD_TABLE),
        "early_end": (grown(0), BAD_SLICE_END),
        "padding_bit": (first_slice(odd + "000001"), BAD_SLICE_END),
        "position": (first_slice(ac63 + "010" + "010" + flat), BAD_POSITION),          # one more run of 0: position 64
        "zero_level": (first_slice("1" + "010" + "1" + flat), BAD_ZERO_LEVEL),
        "level": (first_slice("1" + "010" + big + flat), BAD_LEVEL),
        "dc_level": (first_slice(big + flat), BAD_LEVEL),
        "long_prefix": (first_slice("0" * 17 + "1" + "0" * 17 + flat), BAD_LEVEL),
        "overrun": (first_slice(flat[:-2] + "01"), BAD_OVERRUN),                       # the last code wants one more bit
        "cut_slice": (first_slice(flat[:-2]), BAD_OVERRUN),                            # the last block finds only padding
    }
    good = first_slice(odd)                                      # the hand-made slices are well-formed where they mean to be
    assert parse(good, H, W)[2] == OK and parse(first_slice(ac63 + "1" + flat[2:]), H, W)[2] == OK
    return cases
