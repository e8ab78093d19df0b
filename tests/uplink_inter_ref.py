"""NumPy oracle of the predicted uplink frame AUP1 (ams_amd/csrc/k_uplink_inter.hip, include/ams_hip.h): motion search, residual coder, size
table, the per-frame rate rule and the decoder with every refusal.  Everything AUP1 shares with AUC1 (colour, transform, tables, level rule,
block code, slice cut) is uplink_ref's and is imported from there; this file states only what is new.  All arithmetic is integer, so the
device must agree byte for byte.

Format:
  reference  RGB uint8 [H, W, 3] of the frame's size: what the decoder gave for the previous frame.  Both ends take it to Y and 4:2:0 Cb, Cr
             with the AUC1 colour equations.
  motion     one (dy, dx) per 16 x 16 macroblock, full luma pels, each component in -15 .. 15, the 16 x 16 luma window at
             (16 my + dy, 16 mx + dx) inside the frame.  Luma prediction: the window.  Chroma prediction: the 8 x 8 window at
             (8 my + (dy >> 1), 8 mx + (dx >> 1)); an odd component averages the sample with its successor along that axis:
             (a + b + 1) >> 1, both odd: (a + b + c + d + 2) >> 2.
  residual   current - prediction per 8 x 8 block (no - 128) through the AUC1 forward transform, tables, level rule, zig-zag and block code;
             the decoder adds the inverse transform (no + 128) to the prediction and clamps to 0 .. 255.
  slices     motion slices first: 32 consecutive raster macroblocks each, per macroblock se(dy - pdy) se(dx - pdx) against the previous
             macroblock's vector in the slice ((0, 0) for the first), zero bits to a whole byte; then the Y, Cb, Cr slices as AUC1 cuts them.
             A table length of 0: every level of the slice is zero (a motion slice: every vector is zero) and no byte follows; such a slice
             MUST be sent so.
  payload    "AUP1", u16 H, u16 W, u8 q, 0, 0, 0, u32 total bytes; u16 length per slice; the slices

Encoder choices (the decoder takes any legal vector):
  search     exhaustive over the legal vectors: the least SAD_luma + ZERO_BIAS [vector != 0]; ties to the smaller |dy| + |dx|, then the
             smaller dy, then the smaller dx (RANK is a candidate's place in that order: the search is one min over cost << 10 | rank)
  rate rule  each kind (AUC1, AUP1) takes the largest q in 1 .. 100 whose payload has at most `budget` bytes; the kind with the larger q
             wins, on equal q the smaller payload, then AUC1; neither fits: AUC1 at q = 1 and fits = False
"""
import numpy as np

import uplink_ref as U

MAGIC = b"AUP1"
MB_SLICE = 32                      # macroblocks per motion slice
RANGE = 15
ZERO_BIAS = 128                    # the grid that chose it: zero_bias_grid(); DESIGN 4.11 has its table
BAD_VECTOR, BAD_ZERO_SLICE = 9, 10
MB_MAX_BITS = 22                   # two se() of at most +-30: 11 bits each
INTRA, INTER = 0, 1

_CAND = sorted(((dy, dx) for dy in range(-RANGE, RANGE + 1) for dx in range(-RANGE, RANGE + 1)), key=lambda v: (abs(v[0]) + abs(v[1]), v[0], v[1]))
RANK = {v: i for i, v in enumerate(_CAND)}


def macroblocks(H, W):
    return (H // 16) * (W // 16)


def motion_slices(H, W):
    return (macroblocks(H, W) + MB_SLICE - 1) // MB_SLICE


def slice_count(H, W):
    """all slices of a payload: motion, Y, Cb, Cr"""
    return motion_slices(H, W) + sum(U.slice_counts(H, W))


def max_bytes(H, W):
    return 16 + 2 * slice_count(H, W) + (U.BLOCK_MAX_BITS // 8) * sum(U.plane_blocks(H, W)) + 3 * macroblocks(H, W)


def legal(H, W, my, mx, dy, dx):
    return abs(dy) <= RANGE and abs(dx) <= RANGE and 0 <= 16 * my + dy <= H - 16 and 0 <= 16 * mx + dx <= W - 16


def planes_of(rgb):
    """uint8 [H, W, 3] -> int64 Y [H, W], Cb, Cr [H/2, W/2]"""
    y, cb, cr = U.rgb_to_ycc(np.asarray(rgb))
    return [y, U.subsample(cb), U.subsample(cr)]


# ------------------------------------------------------------------------------------------------------------------ search
def search(cur_y, ref_y, bias=None):
    """-> int64 [macroblocks, 2] (dy, dx) in raster order; one pass per candidate over the macroblocks it is legal for"""
    bias = ZERO_BIAS if bias is None else bias
    H, W = cur_y.shape
    mh, mw = H // 16, W // 16
    best = np.full((mh, mw), np.iinfo(np.int64).max, np.int64)
    for (dy, dx), rank in RANK.items():
        y0, y1 = max(0, -(dy // 16)), min(mh, (H - 16 - dy) // 16 + 1)          # macroblock rows with 0 <= 16 my + dy <= H - 16
        x0, x1 = max(0, -(dx // 16)), min(mw, (W - 16 - dx) // 16 + 1)
        if y0 >= y1 or x0 >= x1:
            continue
        a = cur_y[16 * y0:16 * y1, 16 * x0:16 * x1]
        b = ref_y[16 * y0 + dy:16 * y1 + dy, 16 * x0 + dx:16 * x1 + dx]
        sad = np.abs(a - b).reshape(y1 - y0, 16, x1 - x0, 16).sum((1, 3))
        key = (sad + (bias if (dy, dx) != (0, 0) else 0)) << 10 | rank
        best[y0:y1, x0:x1] = np.minimum(best[y0:y1, x0:x1], key)
    return np.array([_CAND[k & 1023] for k in best.reshape(-1)], np.int64).reshape(-1, 2)


def search_naive(cur_y, ref_y, bias=None):
    """the same rule as a triple loop: macroblock, dy, dx"""
    bias = ZERO_BIAS if bias is None else bias
    H, W = cur_y.shape
    out = []
    for my in range(H // 16):
        for mx in range(W // 16):
            best = None
            for dy in range(-RANGE, RANGE + 1):
                for dx in range(-RANGE, RANGE + 1):
                    if not legal(H, W, my, mx, dy, dx):
                        continue
                    sad = int(np.abs(cur_y[16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
                                     - ref_y[16 * my + dy:16 * my + dy + 16, 16 * mx + dx:16 * mx + dx + 16]).sum())
                    key = (sad + (bias if (dy, dx) != (0, 0) else 0), abs(dy) + abs(dx), dy, dx)
                    best = key if best is None or key < best else best
            out.append(best[2:])
    return np.array(out, np.int64)


# -------------------------------------------------------------------------------------------------------------- prediction
def predict(ref_planes, vectors):
    """-> the predicted Y, Cb, Cr planes for one vector per macroblock"""
    y, cb, cr = ref_planes
    H, W = y.shape
    mw = W // 16
    out = [np.zeros_like(p) for p in ref_planes]
    for i, (dy, dx) in enumerate(np.asarray(vectors).tolist()):
        my, mx = divmod(i, mw)
        assert legal(H, W, my, mx, dy, dx), (my, mx, dy, dx)
        out[0][16 * my:16 * my + 16, 16 * mx:16 * mx + 16] = y[16 * my + dy:16 * my + dy + 16, 16 * mx + dx:16 * mx + dx + 16]
        cy, cx, oy, ox = 8 * my + (dy >> 1), 8 * mx + (dx >> 1), dy & 1, dx & 1
        for o, p in zip(out[1:], (cb, cr)):
            w = p[cy:cy + 8 + oy, cx:cx + 8 + ox]                # stays in the plane for every legal vector (include/ams_hip.h)
            if oy and ox:
                w = (w[:-1, :-1] + w[:-1, 1:] + w[1:, :-1] + w[1:, 1:] + 2) >> 2
            elif oy:
                w = (w[:-1] + w[1:] + 1) >> 1
            elif ox:
                w = (w[:, :-1] + w[:, 1:] + 1) >> 1
            o[8 * my:8 * my + 8, 8 * mx:8 * mx + 8] = w
    return out


def residual_transform(cur_planes, pred_planes):
    """-> the three planes' residual coefficients, int64 [blocks, 64] in zig-zag order: what the encoder's scratch holds"""
    return [U.fdct(U.to_blocks(c - p)).reshape(-1, 64)[:, U.ZIGZAG] for c, p in zip(cur_planes, pred_planes)]


def analyse(frame, reference, bias=None, vectors=None):
    """one search and one residual transform -> (vectors, coefficient planes, predicted planes)"""
    frame, reference = np.asarray(frame), np.asarray(reference)
    assert frame.dtype == np.uint8 and frame.shape == reference.shape and U.shape_ok(*frame.shape[:2]), (frame.shape, reference.shape)
    cur, ref = planes_of(frame), planes_of(reference)
    vectors = search(cur[0], ref[0], bias) if vectors is None else np.asarray(vectors, np.int64)
    pred = predict(ref, vectors)
    return vectors, residual_transform(cur, pred), pred


# ---------------------------------------------------------------------------------------------------------------- lengths
def _vector_diff(vectors):
    pred = np.concatenate([np.zeros((1, 2), np.int64), vectors[:-1]])
    pred[::MB_SLICE] = 0
    return vectors - pred


def motion_bytes(vectors):
    """byte length of every motion slice; 0 where every vector is zero"""
    bits = U._ue_bits(U._se_map(_vector_diff(vectors))).sum(1)
    starts = np.arange(0, len(vectors), MB_SLICE)
    nz = np.add.reduceat(np.abs(vectors).sum(1), starts) != 0
    return np.where(nz, (np.add.reduceat(bits, starts) + 7) // 8, 0)


def residual_bytes(levels):
    """byte length of every slice of one plane; 0 where every level is zero"""
    starts = np.arange(0, len(levels), U.SLICE_BLOCKS)
    nz = np.add.reduceat(np.abs(levels).sum(1), starts) != 0
    return np.where(nz, U.slice_bytes(levels), 0)


def slice_lengths(vectors, planes, q):
    return np.concatenate([motion_bytes(vectors)] + [residual_bytes(U.quantise(c, q, i > 0)) for i, c in enumerate(planes)])


def size_table(frame, reference, analysed=None):
    """int64 [100]: the exact AUP1 payload bytes at q = 1 .. 100"""
    vectors, planes, _ = analysed or analyse(frame, reference)
    return np.array([16 + 2 * slice_count(*np.asarray(frame).shape[:2]) + int(slice_lengths(vectors, planes, q).sum()) for q in range(1, 101)], np.int64)


# ---------------------------------------------------------------------------------------------------------------- encoder
def _motion_symbols(vectors):
    v = (U._se_map(_vector_diff(vectors)) + 1).reshape(-1)
    return v, 2 * U._BITLEN[v] - 1


def assemble(H, W, q, slices):
    table = np.array([len(s) for s in slices], "<u2").tobytes()
    total = 16 + len(table) + sum(len(s) for s in slices)
    return MAGIC + np.array([H, W], "<u2").tobytes() + bytes([q, 0, 0, 0]) + np.array([total], "<u4").tobytes() + table + b"".join(slices)


def encode(frame, reference, q, analysed=None, bias=None, vectors=None):
    """-> the AUP1 payload at quality q"""
    assert 1 <= q <= 100
    H, W = np.asarray(frame).shape[:2]
    vectors, planes, _ = analysed or analyse(frame, reference, bias, vectors)
    slices = []
    for s in range(0, len(vectors), MB_SLICE):
        v = vectors[s:s + MB_SLICE]
        slices.append(U._pack(*_motion_symbols(v)) if v.any() else b"")
    for i, c in enumerate(planes):
        lv = U.quantise(c, q, i > 0)
        slices += [U._pack(*U._symbols(lv[s:s + U.SLICE_BLOCKS])) if lv[s:s + U.SLICE_BLOCKS].any() else b"" for s in range(0, len(lv), U.SLICE_BLOCKS)]
    return assemble(H, W, q, slices)


def reconstruct(levels, vectors, q, reference):
    """what the decoder gives for these levels and vectors: the closed loop's next reference"""
    H, W = np.asarray(reference).shape[:2]
    pred = predict(planes_of(reference), vectors)
    px = []
    for i, (lv, p) in enumerate(zip(levels, pred)):
        c = U.dequantise(lv, q, i > 0)
        t = (np.einsum("vi,nvu->niu", U.M, c) + 512) >> 10
        x = (np.einsum("uj,niu->nij", U.M, t) + 32768) >> 16                     # uplink_ref.idct without its + 128 and clamp
        px.append(np.clip(p + U.from_blocks(x, H >> (i > 0), W >> (i > 0)), 0, 255))
    return U.ycc_to_rgb(*px)


def encoder_reconstruction(frame, reference, q, analysed=None):
    vectors, planes, _ = analysed or analyse(frame, reference)
    return reconstruct([U.quantise(c, q, i > 0) for i, c in enumerate(planes)], vectors, q, reference)


def choose(sizes_intra, sizes_inter, budget):
    """the per-frame rate rule -> (kind, q, fits)"""
    qi, fi = U.choose_quality(sizes_intra, budget)
    qp, fp = U.choose_quality(sizes_inter, budget)
    if not fi and not fp:
        return INTRA, 1, False
    if fp and (not fi or qp > qi or (qp == qi and sizes_inter[qp - 1] < sizes_intra[qi - 1])):
        return INTER, qp, True
    return INTRA, qi, True


def encode_to_budget(frame, budget, reference=None):
    """-> (payload, q, fits, kind)"""
    if reference is None:
        payload, q, fits, _ = U.encode_to_budget(frame, budget)
        return payload, q, fits, INTRA
    analysed = analyse(frame, reference)
    intra = U.transform(frame)
    sizes_intra = np.array([U.payload_size(intra, q) for q in range(1, 101)], np.int64)
    kind, q, fits = choose(sizes_intra, size_table(frame, reference, analysed), budget)
    return (encode(frame, reference, q, analysed) if kind == INTER else U.encode(frame, q, intra)), q, fits, kind


def kind_of(payload):
    return {U.MAGIC: INTRA, MAGIC: INTER}.get(bytes(payload[:4]))


# ---------------------------------------------------------------------------------------------------------------- decoder
def _parse_motion(data, H, W, first, n):
    """-> (vectors [n, 2], status): the first violation in reading order ends the slice"""
    bits = "".join("{:08b}".format(b) for b in data)
    end, pos = len(bits), 0
    vectors = np.zeros((n, 2), np.int64)
    mw = W // 16

    def se():
        nonlocal pos
        one = bits.find("1", pos, pos + U.MAX_PREFIX_ZEROS + 1)
        if one < 0:
            return None, U.BAD_LEVEL if end - pos > U.MAX_PREFIX_ZEROS else U.BAD_OVERRUN
        zeros = one - pos
        if one + zeros + 1 > end:
            return None, U.BAD_OVERRUN
        v = int(bits[one:one + zeros + 1], 2) - 1
        pos = one + zeros + 1
        return ((v + 1) // 2 if v & 1 else -(v // 2)), U.OK

    pred = [0, 0]
    for i in range(n):
        for c in range(2):
            d, st = se()
            if st:
                return vectors, st
            pred[c] += d
            if abs(pred[c]) > RANGE:
                return vectors, BAD_VECTOR
        my, mx = divmod(first + i, mw)
        if not legal(H, W, my, mx, *pred):
            return vectors, BAD_VECTOR
        vectors[i] = pred
    if (pos + 7) // 8 != len(data) or "1" in bits[pos:]:
        return vectors, U.BAD_SLICE_END
    return vectors, U.OK if vectors.any() else BAD_ZERO_SLICE


def parse(payload, H, W):
    """-> (q, vectors, the three planes' levels, status).  Header and table first, in the order of the status codes; then every slice on its
    own, the largest code of the malformed ones."""
    p = bytes(payload)
    nm, ns = motion_slices(H, W), U.slice_counts(H, W)
    n_all = nm + sum(ns)
    if len(p) < 16 or p[:4] != MAGIC:
        return 0, None, None, U.BAD_HEADER
    h, w = np.frombuffer(p[4:8], "<u2")
    q = p[8]
    total = int(np.frombuffer(p[12:16], "<u4")[0])
    if (h, w) != (H, W) or not 1 <= q <= 100 or p[9:12] != b"\0\0\0" or total != len(p) or total < 16 + 2 * n_all:
        return 0, None, None, U.BAD_HEADER
    lens = np.frombuffer(p[16:16 + 2 * n_all], "<u2").astype(np.int64)
    if 16 + 2 * n_all + int(lens.sum()) != total:
        return q, None, None, U.BAD_TABLE
    offs = 16 + 2 * n_all + np.concatenate([[0], np.cumsum(lens)])
    status = U.OK
    nmb = macroblocks(H, W)
    vectors = np.zeros((nmb, 2), np.int64)
    for s in range(nm):
        if lens[s]:
            first = s * MB_SLICE
            part, st = _parse_motion(p[offs[s]:offs[s + 1]], H, W, first, min(MB_SLICE, nmb - first))
            vectors[first:first + len(part)] = part
            status = max(status, st)
    planes, s = [], nm
    for nb, n in zip(U.plane_blocks(H, W), ns):
        lv = np.zeros((nb, 64), np.int64)
        for j in range(n):
            b0 = j * U.SLICE_BLOCKS
            if lens[s]:
                part, st = U._parse_slice(p[offs[s]:offs[s + 1]], min(U.SLICE_BLOCKS, nb - b0))
                lv[b0:b0 + len(part)] = part
                status = max(status, st if st or part.any() else BAD_ZERO_SLICE)
            s += 1
        planes.append(lv)
    return q, vectors, planes, status


def decode(payload, reference):
    """-> uint8 [H, W, 3], or uplink_ref.Refused with the status"""
    H, W = np.asarray(reference).shape[:2]
    q, vectors, planes, status = parse(payload, H, W)
    if status != U.OK:
        raise U.Refused(status)
    return reconstruct(planes, vectors, q, reference)


def zero_length_slices(payload, H, W):
    """(slices of length 0, all slices) of a well-formed AUP1 payload"""
    n = slice_count(H, W)
    lens = np.frombuffer(bytes(payload[16:16 + 2 * n]), "<u2")
    return int((lens == 0).sum()), n


# -------------------------------------------------------------------------------------------------------------- test data
def pairs(H, W, seed=0):
    """the (current, reference) contents the tests run: name -> (uint8 [H, W, 3], uint8 [H, W, 3])"""
    from ams_amd import synth
    rng = np.random.RandomState(seed)
    big = rng.randint(0, 256, (H + 32, W + 32, 3)).astype(np.uint8)

    def moved(dy, dx):
        """cur(y, x) = ref(y + dy, x + dx): interior macroblocks find (dy, dx) with no residual"""
        return np.ascontiguousarray(big[16 + dy:16 + dy + H, 16 + dx:16 + dx + W]), np.ascontiguousarray(big[16:16 + H, 16:16 + W])

    video = synth.SyntheticVideo(max(H, W // 2), 1, [0, 1, 2, 10, 11, 13], seed=3)
    clip = [np.ascontiguousarray(video.frame(t)[0][:H, :W]) for t in (0, 1)]
    noise = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    extremes = np.zeros((H, W, 3), np.uint8)
    extremes[:, W // 2:] = 255                                   # left half: reference 255 under 0; right half the reverse
    return {"same": (noise, noise), "shift": moved(3, -5), "odd": moved(1, 1), "clip": (clip[1], clip[0]),
            "unrelated": (noise, rng.randint(0, 256, (H, W, 3)).astype(np.uint8)), "extremes": (extremes, 255 - extremes)}


def chain(frames, q):
    """I P P P ... in the closed loop -> (payloads, what the decoder gives for each)"""
    payloads, decoded = [], []
    for k, f in enumerate(frames):
        p = U.encode(f, q) if k == 0 else encode(f, decoded[-1], q)
        payloads.append(p)
        decoded.append(U.decode(p, *f.shape[:2]) if k == 0 else decode(p, decoded[-1]))
    return payloads, decoded


def _bits_to_bytes(bits):
    return np.packbits(np.array([int(c) for c in bits + "0" * (-len(bits) % 8)], np.uint8)).tobytes()


def _se(v):
    u = 2 * v - 1 if v > 0 else -2 * v
    return "0" * ((u + 1).bit_length() - 1) + "{:b}".format(u + 1)


def with_slice(payload, H, W, s, data):
    """slice `s` replaced by `data`, table and total kept consistent"""
    n = slice_count(H, W)
    lens = np.frombuffer(bytes(payload[16:16 + 2 * n]), "<u2").astype(np.int64)
    offs = 16 + 2 * n + np.concatenate([[0], np.cumsum(lens)])
    lens[s] = len(data)
    body = bytes(payload[:16]) + lens.astype("<u2").tobytes() + bytes(payload[16 + 2 * n:offs[s]]) + data + bytes(payload[offs[s + 1]:])
    return body[:12] + np.array([len(body)], "<u4").tobytes() + body[16:]


def _vector_bits(H, W, s, vectors):
    """motion slice `s` as a bit string: `vectors` (a list of (dy, dx)) for its first macroblocks, zero vectors for the rest"""
    n = min(MB_SLICE, macroblocks(H, W) - s * MB_SLICE)
    v = np.zeros((n, 2), np.int64)
    v[:len(vectors)] = vectors
    return "".join(_se(int(d)) for d in _vector_diff(v).reshape(-1))


def with_vectors(payload, H, W, s, vectors):
    return with_slice(payload, H, W, s, _bits_to_bytes(_vector_bits(H, W, s, vectors)))


def _padding_bit(bits):
    assert len(bits) % 8, "no padding to set a bit in"
    return bits + "0" * (-len(bits) % 8 - 1) + "1"


def malformed(payload, H, W):
    """name -> (bytes, the status the decoder must give) over one well-formed AUP1 payload (H, W >= 32 for the border cases)"""
    p = bytes(payload)
    nm = motion_slices(H, W)
    mw, nmb = W // 16, macroblocks(H, W)
    n0 = min(MB_SLICE, nmb)
    nb0 = min(U.SLICE_BLOCKS, U.plane_blocks(H, W)[0])

    def edit(i, v):
        b = bytearray(p)
        b[i] = v
        return bytes(b)

    def y_slice(bits):
        return with_slice(p, H, W, nm, _bits_to_bytes(bits))

    def vec_at(i, v):
        """macroblock i gets v, the others of its motion slice (0, 0)"""
        return with_vectors(p, H, W, i // MB_SLICE, [(0, 0)] * (i % MB_SLICE) + [v])

    flat = "11" * nb0
    odd = "0101" + "11" * (nb0 - 1)
    big = "0" * 12 + "1" + "0" * 12
    last_col, bottom = mw - 1, nmb - mw                          # macroblocks on the right and the bottom border
    one = _vector_bits(H, W, 0, [(1, 0)])                        # (1, 0) for the first macroblock, then zero vectors: ends in "11"
    assert n0 >= 3 and H >= 32 and W >= 32
    cases = {
        "magic": (edit(0, ord("B")), U.BAD_HEADER),
        "intra_magic": (edit(2, ord("C")), U.BAD_HEADER),
        "height": (edit(4, (p[4] + 16) & 255), U.BAD_HEADER),
        "width": (edit(6, (p[6] + 16) & 255), U.BAD_HEADER),
        "quality_0": (edit(8, 0), U.BAD_HEADER),
        "quality_101": (edit(8, 101), U.BAD_HEADER),
        "reserved": (edit(10, 1), U.BAD_HEADER),
        "total": (edit(12, (p[12] + 1) & 255), U.BAD_HEADER),
        "truncated": (p[:-1], U.BAD_HEADER),
        "short_header": (p[:9], U.BAD_HEADER),
        "no_table": (p[:16], U.BAD_HEADER),
        "empty": (b"", U.BAD_HEADER),
        "table_sum": (edit(16 + 2 * nm, (p[16 + 2 * nm] + 1) & 255), U.BAD_TABLE),
        "early_end": (y_slice(odd + "0" * 12), U.BAD_SLICE_END),
        "padding_bit": (y_slice(_padding_bit(odd)), U.BAD_SLICE_END),
        "position": (y_slice("1" + "0000001000000" + "010" + "010" + "010" + flat), U.BAD_POSITION),
        "zero_level": (y_slice("1" + "010" + "1" + flat), U.BAD_ZERO_LEVEL),
        "level": (y_slice("1" + "010" + big + flat), U.BAD_LEVEL),
        "dc_level": (y_slice(big + flat), U.BAD_LEVEL),
        "long_prefix": (y_slice("0" * 17 + "1" + "0" * 17 + flat), U.BAD_LEVEL),
        "overrun": (y_slice(odd[:-2] + "01"), U.BAD_OVERRUN),
        "cut_slice": (y_slice(odd[:-2]), U.BAD_OVERRUN),
        "vector_dy_16": (with_slice(p, H, W, 0, _bits_to_bytes(_se(16) + _se(0) + "11" * (n0 - 1))), BAD_VECTOR),
        "vector_dx_-16": (with_slice(p, H, W, 0, _bits_to_bytes(_se(0) + _se(-16) + "11" * (n0 - 1))), BAD_VECTOR),
        "window_top": (vec_at(0, (-1, 0)), BAD_VECTOR),
        "window_left": (vec_at(0, (0, -1)), BAD_VECTOR),
        "window_right": (vec_at(last_col, (0, 1)), BAD_VECTOR),
        "window_bottom": (vec_at(bottom, (1, 0)), BAD_VECTOR),
        "motion_cut": (with_slice(p, H, W, 0, _bits_to_bytes(one[:-2])), U.BAD_OVERRUN),
        "motion_padding": (with_slice(p, H, W, 0, _bits_to_bytes(_padding_bit(one))), U.BAD_SLICE_END),
        "motion_early_end": (with_slice(p, H, W, 0, _bits_to_bytes(one) + b"\0"), U.BAD_SLICE_END),
        "zero_motion_long": (with_slice(p, H, W, 0, _bits_to_bytes("11" * n0)), BAD_ZERO_SLICE),
        "zero_levels_long": (y_slice(flat), BAD_ZERO_SLICE),
    }
    assert parse(y_slice(odd), H, W)[3] == U.OK and parse(vec_at(0, (1, 1)), H, W)[3] == U.OK
    assert parse(vec_at(last_col, (0, -1)), H, W)[3] == U.OK and parse(vec_at(bottom, (-1, 0)), H, W)[3] == U.OK
    return cases


def zero_bias_grid(H=256, W=512, biases=(0, 64, 128, 256, 512), qualities=(10, 30, 60), gaps=(1, 25)):
    """The grid ZERO_BIAS was chosen on: rows (gap, q, intra bytes, zero-vector bytes, [bytes per bias]); the reference is frame t = 0 of the
    synthetic clip, seed 3, as the decoder gives it at the same q."""
    from ams_amd import synth
    video = synth.SyntheticVideo(max(H, W // 2), 1, [0, 1, 2, 10, 11, 13], seed=3)
    frame = lambda t: np.ascontiguousarray(video.frame(t)[0][:H, :W])
    rows = []
    for gap in gaps:
        cur = frame(gap)
        for q in qualities:
            ref = U.decode(U.encode(frame(0), q), H, W)
            zero = len(encode(cur, ref, q, vectors=np.zeros((macroblocks(H, W), 2), np.int64)))
            rows.append((gap, q, len(U.encode(cur, q)), zero, [len(encode(cur, ref, q, bias=b)) for b in biases]))
    return rows
