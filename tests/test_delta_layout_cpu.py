"""The two layouts of the downlink delta (ams_amd/delta.py) and a NumPy decoder of the payload, checked against the reference's host writer
(run.py:316-336).  The decoder here is the one tests/test_gpu_delta.py and tests/test_gpu_edge_delta_run.py hold the device decoder to."""
import ctypes as C

import numpy as np
import pytest

from ams_amd import delta as D, hip, spec as S

SPEC19 = S.build_spec(19)


def encode(params, masks):
    """the reference's writer: per variable np.packbits(mask.flatten()), then per variable p[m].astype(np.float16)"""
    out = bytearray()
    for m in masks:
        out += np.packbits(np.asarray(m).flatten()).tobytes()
    for p, m in zip(params, masks):
        out += np.asarray(p)[np.asarray(m)].astype(np.float16).tobytes()
    return bytes(out)


def decode(payload, layout, params, stats):
    """NumPy decoder: writes float32(float16 value) into copies of the flat ``params`` / ``stats`` regions; raises ValueError on a payload
    that does not fit its mask (size, or a set padding bit)"""
    buf = np.frombuffer(payload, dtype=np.uint8)
    if buf.size < layout.mask_bytes:
        raise ValueError("truncated mask section")
    params, stats = params.copy(), stats.copy()
    masks = []
    for e in layout.entries:
        bits = np.unpackbits(buf[e.mask_offset:e.mask_offset + (e.count + 7) // 8])
        if bits[e.count:].any():
            raise ValueError("padding bit set in %s" % e.name)
        masks.append(bits[:e.count].astype(bool))
    total = sum(int(m.sum()) for m in masks)
    if layout.mask_bytes + 2 * total != buf.size:
        raise ValueError("payload size %d, mask says %d" % (buf.size, layout.mask_bytes + 2 * total))
    vals = buf[layout.mask_bytes:].view("<f2").astype(np.float32)
    k = 0
    for e, m in zip(layout.entries, masks):
        dst = params if e.region == hip.REGION_PARAMS else stats
        n = int(m.sum())
        seg = dst[e.offset:e.offset + e.count]
        seg[m] = vals[k:k + n]
        k += n
    return params, stats


def layout_vars(spec, layout, params, stats):
    return [(params if e.region == hip.REGION_PARAMS else stats)[e.offset:e.offset + e.count] for e in layout.entries]


@pytest.mark.parametrize("num_classes,counts", [(19, ((164, 2113043, 264131), (272, 2146131, 268267))),
                                                (21, ((164, None, 264195), (272, None, 268331)))])
def test_layout_sizes(num_classes, counts):
    spec = S.build_spec(num_classes)
    for strategy, (n_vars, n_el, mask) in zip(("coord_desc_rand", "full_model"), counts):
        L = D.delta_layout(spec, strategy)
        assert len(L.entries) == n_vars and L.mask_bytes == mask
        if n_el is not None:
            assert L.n_elements == n_el
        assert L.max_payload_bytes == L.mask_bytes + 2 * L.n_elements
    assert D.delta_layout(SPEC19, "full_model").max_payload_bytes == 4560529
    for s in ("coord_desc_auto", "coord_desc_last", "coord_desc_first", "coord_desc_both"):
        assert D.delta_layout(spec, s).kind == D.TRAINABLE
    with pytest.raises(ValueError):
        D.delta_layout(spec, "no_such_strategy")


def test_layout_orders_and_tiling():
    tr = D.delta_layout(SPEC19, "coord_desc_rand")
    assert [e.name for e in tr.entries] == [v.name for v in SPEC19.trainable]
    al = D.delta_layout(SPEC19, "full_model")
    assert [e.name for e in al.entries] == SPEC19.all_variable_names()
    for L in (tr, al):
        mask = 0
        for e in L.entries:
            v = SPEC19.by_name[e.name]
            assert (e.region, e.offset, e.count) == (hip.REGION_PARAMS if v.trainable else hip.REGION_STATS, v.offset, v.size)
            assert e.mask_offset == mask
            mask += (e.count + 7) // 8
        assert mask == L.mask_bytes
    # the all-variables layout tiles both regions exactly, the trainable one tiles params exactly
    for L, regions in ((al, (hip.REGION_PARAMS, hip.REGION_STATS)), (tr, (hip.REGION_PARAMS,))):
        for r, n in zip(regions, (SPEC19.n_trainable, SPEC19.n_stats)):
            spans = sorted((e.offset, e.count) for e in L.entries if e.region == r)
            pos = 0
            for off, cnt in spans:
                assert off == pos
                pos += cnt
            assert pos == n
    assert not any(e.region == hip.REGION_STATS for e in tr.entries)


def test_c_table_matches_entries():
    L = D.delta_layout(SPEC19, "full_model")
    t = L.table()
    assert C.sizeof(hip.DeltaVar) == 32 and len(t) == len(L.entries)
    for d, e in zip(t, L.entries):
        assert (d.region, d.reserved, d.offset, d.count, d.mask_offset) == (e.region, 0, e.offset, e.count, e.mask_offset)
    lib = hip.lib()
    nseg = -(-L.mask_bytes // 2048)
    assert lib.ams_student_apply_delta_scratch(t, len(t)) == 4 * len(t) + nseg
    assert lib.ams_student_apply_delta_scratch(t, 0) == 0


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
@pytest.mark.parametrize("density", ["zero", "one", "tenth", "all"])
def test_numpy_decoder_round_trips_reference_payloads(strategy, density):
    rng = np.random.default_rng(7)
    L = D.delta_layout(SPEC19, strategy)
    params = rng.standard_normal(SPEC19.n_trainable).astype(np.float32)
    stats = rng.standard_normal(SPEC19.n_stats).astype(np.float32)
    base_p = rng.standard_normal(SPEC19.n_trainable).astype(np.float32)
    base_s = rng.standard_normal(SPEC19.n_stats).astype(np.float32)
    vals = layout_vars(SPEC19, L, params, stats)
    if density == "zero":
        masks = [np.zeros(v.size, bool) for v in vals]
    elif density == "one":
        masks = [np.zeros(v.size, bool) for v in vals]
        masks[len(masks) // 2][3] = True
    elif density == "tenth":
        masks = [rng.random(v.size) < 0.1 for v in vals]
    else:
        masks = [np.ones(v.size, bool) for v in vals]
    payload = encode(vals, masks)
    assert len(payload) == L.mask_bytes + 2 * sum(int(m.sum()) for m in masks)
    got_p, got_s = decode(payload, L, base_p, base_s)
    want_p, want_s = base_p.copy(), base_s.copy()
    for e, m, v in zip(L.entries, masks, vals):
        dst = want_p if e.region == hip.REGION_PARAMS else want_s
        seg = dst[e.offset:e.offset + e.count]
        seg[m] = v[m].astype(np.float16).astype(np.float32)
    assert np.array_equal(got_p.view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32))
    for bad in (payload[:-1], payload + b"\0", b""):
        with pytest.raises(ValueError):
            decode(bad, L, base_p, base_s)
