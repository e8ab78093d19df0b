"""NumPy oracle of the q8 downlink delta (include/ams_hip.h: ams_student_encode_delta_q8 / ams_student_apply_delta_q8), the arithmetic the
device encoder and decoder are held to bit for bit.  Every operation is one f32 operation with an f32 result.

Payload over a layout of n variables: [per variable np.packbits(mask)] [n little-endian f32 scales] [one int8 per set mask bit].

  d = cur - base;  amax_v = max |d| over the masked elements (0 if none);  scale_v = amax_v / 127, 0 if below 2^-126;
  q = 0 if scale_v == 0 else clip(rint(d / scale_v), -127, 127);  decoded = base + scale_v * q.

A plain module (like first_block_ref.py): no fixtures, no GPU.
"""
import numpy as np

from ams_amd import hip

F32 = np.float32
TINY = F32(2.0 ** -126)
ERR = 2.0 ** -22          # of the bound below


class NonFinite(ValueError):
    """a masked change is NaN or infinite: the encoder refuses"""


def scales_and_codes(vals, bases, masks):
    """per variable (scale f32, codes int8 of the masked elements in order)"""
    out = []
    with np.errstate(all="ignore"):
        for v, b, m in zip(vals, bases, masks):
            v, b, m = np.asarray(v, F32).reshape(-1), np.asarray(b, F32).reshape(-1), np.asarray(m).reshape(-1).astype(bool)
            d = (v[m] - b[m]).astype(F32)
            if not np.isfinite(d).all():
                raise NonFinite("a masked change is NaN or infinite")
            amax = F32(np.abs(d).max()) if d.size else F32(0)
            scale = F32(amax / F32(127))
            if scale < TINY:
                scale = F32(0)
            if scale == 0:
                q = np.zeros(d.size, np.int8)
            else:
                q = np.clip(np.rint((d / scale).astype(F32)), -127, 127).astype(np.int8)          # np.rint: ties to even
            out.append((scale, q))
    return out


def encode_q8(vals, bases, masks):
    """vals / bases / masks: per variable of the layout, in layout order -> the payload's bytes"""
    sq = scales_and_codes(vals, bases, masks)
    out = bytearray()
    for m in masks:
        out += np.packbits(np.asarray(m).reshape(-1).astype(bool)).tobytes()
    out += np.asarray([s for s, _ in sq], dtype="<f4").tobytes()
    for _, q in sq:
        out += q.tobytes()
    return bytes(out)


def bad_scale_bits(u):
    """uint32 bits of a scale the decoder refuses: NaN, inf, nonzero below 2^-126, negative"""
    u = np.asarray(u, np.uint32)
    a = u & np.uint32(0x7FFFFFFF)
    return (a >= 0x7F800000) | ((a != 0) & (a < 0x00800000)) | (((u >> np.uint32(31)) != 0) & (a != 0))


def decode_value(base, scale, q):
    """f32(base + f32(scale * q)): two roundings"""
    with np.errstate(all="ignore"):
        step = (F32(scale) * np.asarray(q).astype(F32)).astype(F32)
        return (np.asarray(base, F32) + step).astype(F32)


def decode_q8(payload, layout, params, stats):
    """Adds the payload's changes to copies of the flat ``params`` / ``stats`` regions (which hold the base); raises ValueError on a payload
    of the wrong size, with a set padding bit, or with a bad scale: in that order, as the device does."""
    buf = np.frombuffer(payload, dtype=np.uint8)
    n_vars = len(layout.entries)
    if buf.size < layout.mask_bytes:
        raise ValueError("truncated mask section")
    masks, padded = [], None
    for e in layout.entries:
        bits = np.unpackbits(buf[e.mask_offset:e.mask_offset + (e.count + 7) // 8])
        if bits[e.count:].any() and padded is None:
            padded = e.name
        masks.append(bits[:e.count].astype(bool))
    total = sum(int(m.sum()) for m in masks)
    fixed = layout.mask_bytes + 4 * n_vars
    if fixed + total != buf.size:
        raise ValueError("payload size %d, mask says %d" % (buf.size, fixed + total))
    if padded is not None:
        raise ValueError("padding bit set in %s" % padded)
    scale_bits = np.frombuffer(buf[layout.mask_bytes:fixed].tobytes(), dtype="<u4")
    if bad_scale_bits(scale_bits).any():
        raise ValueError("bad scale in variable %d" % int(np.nonzero(bad_scale_bits(scale_bits))[0][0]))
    scales = scale_bits.view(F32)
    codes = np.frombuffer(buf[fixed:].tobytes(), dtype=np.int8)
    params, stats = np.array(params, F32), np.array(stats, F32)
    k = 0
    for e, m, s in zip(layout.entries, masks, scales):
        dst = params if e.region == hip.REGION_PARAMS else stats
        n = int(m.sum())
        seg = dst[e.offset:e.offset + e.count]
        seg[m] = decode_value(seg[m], s, codes[k:k + n])
        k += n
    return params, stats


def error_bound(cur, base, scale, amax):
    """|decoded - cur| <= 0.5 scale + 2^-22 (|cur| + |base| + amax), in f64"""
    cur, base = np.asarray(cur, np.float64), np.asarray(base, np.float64)
    return 0.5 * float(scale) + ERR * (np.abs(cur) + np.abs(base) + float(amax))


# ---- the inputs both the CPU and the GPU tests use -------------------------------------------------------------------------------------
DENSITIES = ("zero", "one", "tenth", "all")
SEG = 2048                # mask bytes per block of the device kernels


def layout_views(layout, params, stats):
    """per entry, the slice of the flat region that holds it (a view: writes go through)"""
    return [(params if e.region == hip.REGION_PARAMS else stats)[e.offset:e.offset + e.count] for e in layout.entries]


def _element_at(layout, byte, bit, step):
    """(entry index, element) of the mask bit at or next to (byte, bit) in direction step that is an element and not padding"""
    pos = byte * 8 + bit
    while True:
        b = pos // 8
        i = max(j for j, e in enumerate(layout.entries) if e.mask_offset <= b and e.count > 0)
        el = pos - layout.entries[i].mask_offset * 8
        if el < layout.entries[i].count:
            return i, el
        pos += step


def make_case(spec, layout, density, seed=11):
    """Current variables, base and masks over the model's own variables for one mask density, with the inputs that can go wrong placed in
    variables of their own (named in the returned ``special``):

      zero      masked change all zero (scale 0), a -0.0 base element among the masked ones; the unmasked elements do change
      single    exactly one masked element
      ties      base 0, scale exactly 2^-10, changes 2^-10 (k + 1/2): every code is a rounding tie
      last      +-8 = +-amax in the last element of a variable whose count is no multiple of 8 (+ at density tenth, - otherwise)
      tiny      changes up to 1e-37: amax / 127 lies below 2^-126, the scale is flushed to 0
      shared    the most 16- to 32-element variables whose masks start in one aligned 8-byte word (one thread's), every element masked
      boundary  the last element in front of mask byte 2048 and the first one from it on, both masked

    -> dict(params, stats, base_p, base_s: flat f32; masks: per entry bool; special: name -> entry indices)."""
    assert density in DENSITIES
    rng = np.random.default_rng(seed)
    ent = layout.entries
    base_p = rng.standard_normal(spec.n_trainable).astype(F32)
    base_s = rng.standard_normal(spec.n_stats).astype(F32)
    params, stats = base_p.copy(), base_s.copy()
    bases, vals = layout_views(layout, base_p, base_s), layout_views(layout, params, stats)
    for b, v in zip(bases, vals):                            # per variable a change of its own size, 1e-6 .. 5
        v += (F32(10.0 ** rng.uniform(-6, np.log10(5.0))) * rng.standard_normal(v.size)).astype(F32)
    if density == "tenth":
        masks = [rng.random(e.count) < 0.1 for e in ent]
    else:
        masks = [np.full(e.count, density == "all", bool) for e in ent]
    force = density in ("tenth", "all")

    # the variables that get a special input, each its own
    by_word = {}
    for i, e in enumerate(ent):
        if e.count:
            by_word.setdefault(e.mask_offset // 8, []).append(i)
    small = ([i for i in g if 16 <= ent[i].count <= 32] for _, g in sorted(by_word.items()))
    shared = max(small, key=len)                             # (the first of the largest groups: 2 in the trainable layout, gamma and beta)
    assert len(shared) >= 2
    lo, hi = _element_at(layout, SEG - 1, 7, -1), _element_at(layout, SEG, 0, +1)
    taken = set(shared) | {lo[0], hi[0]}
    last = next(i for i, e in enumerate(ent) if e.count % 8 and e.count >= 9 and i not in taken)
    taken.add(last)
    free = [i for i, e in enumerate(ent) if e.count >= 256 and i not in taken]
    zero, single, ties, tiny = free[1], free[len(free) // 3], free[len(free) // 2], free[-2]
    special = dict(zero=[zero], single=[single], ties=[ties], last=[last], tiny=[tiny], shared=list(shared), boundary=[lo[0], hi[0]])

    if force:
        for i in shared:
            masks[i][:] = True
        masks[lo[0]][lo[1]] = masks[hi[0]][hi[1]] = True
        if density == "tenth":
            masks[single][:] = False
            masks[single][5] = True
        masks[zero][:3] = True
        masks[ties][:128] = True
        masks[last][-1] = True
        masks[tiny][:16] = True
    elif density == "one":
        masks[len(masks) // 2][3] = True

    m = masks[zero]
    bases[zero][0] = F32(-0.0)
    vals[zero][m] = bases[zero][m]
    vals[zero][~m] = bases[zero][~m] + F32(1)
    bases[ties][:] = 0
    vals[ties][:] = 0
    k = np.arange(128)
    vals[ties][:128] = (F32(2.0 ** -10) * (k - 64 + 0.5).astype(F32)).astype(F32)          # ties at -63.5 .. 63.5
    vals[ties][0], vals[ties][1] = F32(127 * 2.0 ** -10), F32(-127 * 2.0 ** -10)           # amax: the scale is 2^-10
    vals[last][:] = bases[last] + (F32(0.01) * rng.standard_normal(ent[last].count)).astype(F32)
    bases[last][-1] = F32(0.5)
    vals[last][-1] = F32(8.5) if density == "tenth" else F32(-7.5)
    bases[tiny][:] = 0
    vals[tiny][:] = (F32(1e-37) * rng.uniform(-1, 1, ent[tiny].count)).astype(F32)
    vals[tiny][0] = F32(1e-37)
    return dict(params=params, stats=stats, base_p=base_p, base_s=base_s, masks=masks, special=special)
