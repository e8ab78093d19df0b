"""The q8 downlink delta without a GPU: the sizes of both layouts, the NumPy oracle (tests/delta_q8_ref.py) against itself — round trip, the
per-element error bound, the inputs that can go wrong — its refusals, and the scratch sizes the library asks for."""
import numpy as np
import pytest

from ams_amd import delta as D, hip, spec as S
import delta_q8_ref as Q

SPEC19 = S.build_spec(19)
STRATEGIES = ("coord_desc_rand", "full_model")
_cases = {}


def case(strategy, density):
    """the shared inputs with the oracle's payload and decode, computed once and left unchanged"""
    key = (strategy, density)
    if key not in _cases:
        L = D.delta_layout(SPEC19, strategy)
        c = Q.make_case(SPEC19, L, density)
        c["layout"] = L
        c["vals"] = Q.layout_views(L, c["params"], c["stats"])
        c["bases"] = Q.layout_views(L, c["base_p"], c["base_s"])
        c["payload"] = Q.encode_q8(c["vals"], c["bases"], c["masks"])
        c["decoded"] = Q.decode_q8(c["payload"], L, c["base_p"], c["base_s"])
        _cases[key] = c
    return _cases[key]


def check_decoded(L, masks, vals, bases, decoded):
    """unmasked elements keep the base's bits, masked ones lie within the bound of the current value (a flushed variable: at its base, within
    amax); -> the number of variables whose scale was flushed"""
    flushed = 0
    for e, m, cur, base, dec in zip(L.entries, masks, vals, bases, decoded):
        assert np.array_equal(dec[~m].view(np.uint32), base[~m].view(np.uint32)), e.name
        if not m.any():
            continue
        d = (cur[m] - base[m]).astype(np.float32)
        amax = np.abs(d).max()
        scale = np.float32(amax / np.float32(127))
        err = np.abs(dec[m].astype(np.float64) - cur[m].astype(np.float64))
        if scale < Q.TINY:
            flushed += amax > 0
            assert np.array_equal(dec[m], (base[m] + np.float32(0)).astype(np.float32)) and err.max() <= amax < 127 * 2.0 ** -126, e.name
        else:
            assert (err <= Q.error_bound(cur[m], base[m], scale, amax)).all(), (e.name, float(err.max()), float(scale))
    return flushed


@pytest.mark.parametrize("num_classes", [19, 21])
def test_sizes(num_classes):
    spec = S.build_spec(num_classes)
    for strategy in STRATEGIES:
        L = D.delta_layout(spec, strategy)
        assert L.max_payload_bytes_q8 == L.mask_bytes + 4 * len(L.entries) + L.n_elements
        assert L.payload_limit("q8") == L.max_payload_bytes_q8 and L.payload_limit("fp16") == L.max_payload_bytes
    with pytest.raises(ValueError):
        L.payload_limit("q4")
    full = D.delta_layout(SPEC19, "full_model")
    assert (full.mask_bytes, len(full.entries), full.n_elements, full.max_payload_bytes_q8) == (268267, 272, 2146131, 2415486)
    assert full.mask_bytes % 2 == 1 and D.delta_layout(SPEC19, "coord_desc_rand").mask_bytes % 2 == 1          # the scales are unaligned


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("density", Q.DENSITIES)
def test_round_trip_and_error_bound(strategy, density):
    """Size rule; unmasked elements keep their bits; every masked element lies within the derived bound
    0.5 scale + 2^-22 (|cur| + |base| + amax) of the encoder's value.  The bound was derived for scales that are not flushed: in the one
    variable whose scale falls below 2^-126 every code is 0, the element stays at its base, and the error is the change itself, at most
    amax < 127 x 2^-126."""
    c = case(strategy, density)
    L, masks = c["layout"], c["masks"]
    set_bits = sum(int(m.sum()) for m in masks)
    assert len(c["payload"]) == L.mask_bytes + 4 * len(L.entries) + set_bits
    flushed = check_decoded(L, masks, c["vals"], c["bases"], Q.layout_views(L, *c["decoded"]))
    assert flushed == (1 if density in ("tenth", "all") else 0)
    # the layout leaves stats alone where it does not cover them
    if strategy == "coord_desc_rand":
        assert np.array_equal(c["decoded"][1].view(np.uint32), c["base_s"].view(np.uint32))


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("density", ["tenth", "all"])
def test_special_inputs(strategy, density):
    c = case(strategy, density)
    L, masks, sp = c["layout"], c["masks"], c["special"]
    sq = Q.scales_and_codes(c["vals"], c["bases"], masks)
    got = Q.layout_views(L, *c["decoded"])
    (zero,), (ties,), (last,), (tiny,), (single,) = sp["zero"], sp["ties"], sp["last"], sp["tiny"], sp["single"]
    # all-zero masked change: scale 0, codes 0; -0.0 + (+0.0) = +0.0, so the masked -0.0 base element decodes to +0.0
    assert sq[zero][0] == 0 and not sq[zero][1].any() and masks[zero][0]
    assert c["bases"][zero][:1].view(np.uint32)[0] == 0x80000000 and got[zero][:1].view(np.uint32)[0] == 0
    # ties: scale exactly 2^-10 and every tie rounds to the even neighbour
    assert sq[ties][0] == np.float32(2.0 ** -10)
    k = np.arange(2, 128) - 64
    want = np.where(k % 2 == 0, k, k + 1)                    # k + 1/2 -> the even one of k, k + 1
    assert np.array_equal(sq[ties][1][2:128], want) and list(sq[ties][1][:2]) == [127, -127]
    # +-amax in the last element of a variable of 19 elements
    assert L.entries[last].count % 8 and masks[last][-1] and sq[last][1][-1] == (127 if density == "tenth" else -127)
    assert sq[last][0] == np.float32(np.float32(8) / np.float32(127))
    # a scale below 2^-126 is flushed: codes 0, and 1e-37 itself is a normal number
    assert np.float32(1e-37) > Q.TINY and sq[tiny][0] == 0 and not sq[tiny][1].any() and masks[tiny][:16].all()
    if density == "tenth":
        assert masks[single].sum() == 1 and abs(int(sq[single][1][0])) == 127
    # the small variables share one aligned mask word, and there is a set bit on either side of byte 2048
    assert len({L.entries[i].mask_offset // 8 for i in sp["shared"]}) == 1 and all(masks[i].all() for i in sp["shared"])
    packed = np.frombuffer(c["payload"], np.uint8)[:L.mask_bytes]
    assert packed[Q.SEG - 1] & 1 and packed[Q.SEG] & 0x80


def test_minus_128_decodes_as_minus_128():
    assert Q.decode_value(np.float32(1), np.float32(0.25), np.int8(-128)) == np.float32(-31)


def test_encoder_refuses_nonfinite_changes():
    c = case("coord_desc_rand", "tenth")
    for bad in (np.nan, np.inf, -np.inf):
        vals = [v.copy() for v in c["vals"]]
        i = c["special"]["ties"][0]
        vals[i][0] = bad                                      # masked
        with pytest.raises(Q.NonFinite):
            Q.encode_q8(vals, c["bases"], c["masks"])
    vals = [v.copy() for v in c["vals"]]
    i = c["special"]["single"][0]
    vals[i][0] = np.nan                                       # not masked: encodes
    assert not c["masks"][i][0] and Q.encode_q8(vals, c["bases"], c["masks"]) == c["payload"]


def malformed(c):
    """the four kinds: (name, payload)"""
    L, good = c["layout"], c["payload"]
    last = c["special"]["last"][0]                            # 19 elements: 5 padding bits in its third byte
    pad = bytearray(good)
    pad[L.entries[last].mask_offset + 2] |= 1
    # (a device decoder that counts the padding bit as a set bit sees a size mismatch; with one more byte it has to see the bit itself)
    out = [("truncated", good[:-1]), ("over-long", good + b"\0"), ("padding", bytes(pad)), ("padding, one byte more", bytes(pad) + b"\0")]
    for name, bits in (("scale nan", 0x7FC00000), ("scale inf", 0x7F800000), ("scale negative", 0xBF800000), ("scale denormal", 0x007FFFFF)):
        bad = bytearray(good)
        bad[L.mask_bytes + 4 * 7:L.mask_bytes + 4 * 8] = np.uint32(bits).tobytes()
        out.append((name, bytes(bad)))
    return out


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_decoder_raises_on_malformed_payloads(strategy):
    c = case(strategy, "tenth")
    kinds = malformed(c)
    assert len(kinds) == 8
    for name, bad in kinds + [("empty", b""), ("mask only", c["payload"][:c["layout"].mask_bytes])]:
        with pytest.raises(ValueError):
            Q.decode_q8(bad, c["layout"], c["base_p"], c["base_s"])
    assert list(Q.bad_scale_bits([0, 0x80000000, 0x00800000, 0x7F7FFFFF, 1, 0x80800000])) == [False, False, False, False, True, True]


def test_scratch_sizes():
    lib = hip.lib()
    for strategy in STRATEGIES:
        L = D.delta_layout(SPEC19, strategy)
        t, n = L.table(), len(L.entries)
        nseg = -(-L.mask_bytes // 2048)
        # [descriptors 4n][element starts n + 1][maxima: n uint32][payload size][segment counts]
        assert lib.ams_student_encode_delta_q8_scratch(t, n) == 5 * n + 1 + (n + 1) // 2 + 1 + nseg
        assert lib.ams_student_apply_delta_q8_scratch(t, n) == 4 * n + nseg == lib.ams_student_apply_delta_scratch(t, n)
        assert lib.ams_student_encode_delta_q8_scratch(t, 0) == 0 and lib.ams_student_apply_delta_q8_scratch(t, 0) == 0
        assert lib.ams_student_encode_delta_q8_scratch(t, hip.DELTA_MAX_VARS + 1) == 0
    assert (hip.DELTA_BAD_SCALE, hip.DELTA_Q8_NONFINITE) == (3, 4)
