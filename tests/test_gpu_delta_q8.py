"""The q8 downlink delta on the device (k_delta_q8.hip; ams_student_encode_delta_q8 / ams_student_apply_delta_q8; StudentEngine and
SemanticNetwork with fmt="q8"), held to the NumPy oracle of tests/delta_q8_ref.py bit for bit.

  a. encoder and decoder equal the oracle on both layouts at mask densities zero, one element, a tenth and all, over the inputs of
     delta_q8_ref.make_case, with the payload at an even and at an odd address; payload, base, scratch and result words are guarded buffers
     (tests/guarded.py), the scratch exact and poisoned;
  b. malformed payloads raise and leave params and stats bit-identical, also after a base was loaded for them;
  c. a NaN or infinite masked change refuses encoding, a cap one byte short writes nothing: payload and base untouched;
  d. advance_base leaves the oracle's decode in the base, and the next payload from unchanged variables stays inside the bound;
  e. what the host can refuse only with the handle: a variable outside its region;
  f. server -> frozen edge through two SemanticNetworks: the oracle's variables, a re-freeze, queued frames on the old model.
"""
import ctypes as C
import random
from collections import deque

import numpy as np
import pytest
import torch

from ams_amd import delta as D, exp_configs, hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
import delta_q8_ref as Q
import guarded
from test_delta_q8_cpu import case, check_decoded, malformed

pytestmark = pytest.mark.gpu

CI = [0, 1, 2, 10, 11, 13]
SPEC = S.build_spec()
CW = exp_configs.class_weights(25)
STRATEGIES = ("coord_desc_rand", "full_model")


@pytest.fixture(scope="module")
def eng():
    e = StudentEngine(CI, 64, 128, max_batch=1, trainable=False)
    yield e
    e.close()


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(SPEC, seed=0)


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def set_variables(eng, params, stats):
    eng.params.copy_(torch.from_numpy(np.ascontiguousarray(params)))
    eng.stats.copy_(torch.from_numpy(np.ascontiguousarray(stats)))


def flat_mask(masks):
    return guarded.inp(np.concatenate(masks).astype(np.uint8), torch.uint8)


def encode(eng, L, mask, base_p, base_s, advance, cap, odd=False, written=True):
    """ams_student_encode_delta_q8 on guarded buffers: a payload buffer of exactly `cap` bytes (behind one more byte when `odd`), exact
    poisoned scratch.  A payload byte may well be 255, the byte pattern of the poison, so what the call wrote is judged here: `written=False`
    asserts that every byte still holds the pattern, and the callers compare a written payload with the oracle's byte for byte.
    -> (payload bytes as numpy, size, status)"""
    table = L.table()
    out = guarded.scratch(cap + int(odd), torch.uint8)
    size, status = guarded.out(1, torch.int64), guarded.out(1, torch.int32)
    scratch = guarded.scratch(int(eng.lib.ams_student_encode_delta_q8_scratch(table, len(table))), torch.int64)
    hip.check(eng.lib.ams_student_encode_delta_q8(eng._h, _ptr(mask), table, len(table), _ptr(base_p), _ptr(base_s), int(advance), _ptr(out, int(odd)),
                                                  cap, _ptr(size), _ptr(status), _ptr(scratch), scratch.numel(), eng._stream()),
              "ams_student_encode_delta_q8")
    guarded.check("ams_student_encode_delta_q8")
    kept = guarded.poisoned(out)
    assert bool(kept[:int(odd)].all()) and (written or bool(kept.all()))          # the byte in front of an odd start; a refused payload
    return out.cpu().numpy()[int(odd):], int(size.item()), int(status.item())


def apply(eng, L, payload, odd=False):
    """ams_student_apply_delta_q8 on a guarded payload (at an odd address when `odd`) and exact poisoned scratch -> (applied, status)"""
    table = L.table()
    buf = guarded.inp(np.concatenate([np.zeros(int(odd), np.uint8), np.frombuffer(payload, np.uint8)]), torch.uint8)
    n = buf.numel() - int(odd)
    applied, status = guarded.out(1, torch.int64), guarded.out(1, torch.int32)
    scratch = guarded.scratch(int(eng.lib.ams_student_apply_delta_q8_scratch(table, len(table))), torch.int64)
    hip.check(eng.lib.ams_student_apply_delta_q8(eng._h, _ptr(buf, int(odd)) if n else None, n, table, len(table), _ptr(applied), _ptr(status),
                                                 _ptr(scratch), scratch.numel(), eng._stream()), "ams_student_apply_delta_q8")
    guarded.check("ams_student_apply_delta_q8")
    return int(applied.item()), int(status.item())


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("density", Q.DENSITIES)
def test_encoder_and_decoder_match_the_oracle(eng, strategy, density):
    guarded.reset()
    c = case(strategy, density)
    L, want = c["layout"], c["payload"]
    set_bits = sum(int(m.sum()) for m in c["masks"])
    set_variables(eng, c["params"], c["stats"])
    base_p, base_s = guarded.inp(c["base_p"]), guarded.inp(c["base_s"])
    mask = flat_mask(c["masks"])
    for odd in (False, True):
        got, size, status = encode(eng, L, mask, base_p, base_s, 0, len(want), odd)
        assert (size, status) == (len(want), hip.DELTA_OK) and size == L.mask_bytes + 4 * len(L.entries) + set_bits
        assert got.tobytes() == want, (strategy, density, odd, int(np.nonzero(got != np.frombuffer(want, np.uint8))[0][0]))
    if density == "all":                                       # NULL = every element; the trainable layout needs no statistics base
        got, size, status = encode(eng, L, None, base_p, base_s if strategy == "full_model" else None, 0, len(want))
        assert (size, status) == (len(want), hip.DELTA_OK) and got.tobytes() == want
    assert bits_equal(base_p.cpu().numpy(), c["base_p"]) and bits_equal(base_s.cpu().numpy(), c["base_s"])          # advance_base = 0
    assert bits_equal(eng.params.cpu().numpy(), c["params"]) and bits_equal(eng.stats.cpu().numpy(), c["stats"])
    for odd in (False, True):
        set_variables(eng, c["base_p"], c["base_s"])
        assert apply(eng, L, want, odd) == (set_bits, hip.DELTA_OK)
        assert bits_equal(eng.params.cpu().numpy(), c["decoded"][0]), (strategy, density, odd)
        assert bits_equal(eng.stats.cpu().numpy(), c["decoded"][1]), (strategy, density, odd)


def test_a_code_of_minus_128_decodes_as_minus_128(eng):
    guarded.reset()
    c = case("coord_desc_rand", "one")
    L = c["layout"]
    payload = bytearray(c["payload"])
    assert len(payload) == L.mask_bytes + 4 * len(L.entries) + 1
    payload[-1] = 0x80
    set_variables(eng, c["base_p"], c["base_s"])
    assert apply(eng, L, bytes(payload)) == (1, hip.DELTA_OK)
    want_p, want_s = Q.decode_q8(bytes(payload), L, c["base_p"], c["base_s"])
    changed = np.nonzero(want_p.view(np.uint32) != c["base_p"].view(np.uint32))[0]
    assert len(changed) == 1 and bits_equal(eng.params.cpu().numpy(), want_p) and bits_equal(eng.stats.cpu().numpy(), want_s)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_malformed_payloads_raise_and_change_nothing(eng, strategy, W0):
    guarded.reset()
    c = case(strategy, "tenth")
    L = c["layout"]
    set_variables(eng, c["base_p"], c["base_s"])
    want_status = {"truncated": hip.DELTA_BAD_SIZE, "over-long": hip.DELTA_BAD_SIZE, "padding, one byte more": hip.DELTA_BAD_PADDING}
    kinds = malformed(c) + [("empty", b""), ("cut inside the masks", c["payload"][:L.mask_bytes - 3]), ("cut inside the scales", c["payload"][:L.mask_bytes + 9])]
    for name, bad in kinds:
        applied, status = apply(eng, L, bad, odd=name == "padding")
        assert applied == 0 and status != hip.DELTA_OK, name
        assert status == want_status.get(name, hip.DELTA_BAD_SCALE if name.startswith("scale") else hip.DELTA_BAD_SIZE), (name, status)
        assert bits_equal(eng.params.cpu().numpy(), c["base_p"]) and bits_equal(eng.stats.cpu().numpy(), c["base_s"]), name
        with pytest.raises(hip.AmsHipError, match="rejected"):
            eng.apply_delta(bad, L, fmt="q8")
        assert bits_equal(eng.params.cpu().numpy(), c["base_p"]) and bits_equal(eng.stats.cpu().numpy(), c["base_s"]), name
    assert eng.apply_delta(c["payload"], L, fmt="q8") == sum(int(m.sum()) for m in c["masks"])          # the engine is still usable
    assert bits_equal(eng.params.cpu().numpy(), c["decoded"][0])
    # through the network, with a base loaded for the update: the model it had stays
    edge = SemanticNetwork("unused", class_weights_exp=CW, height=64, frozen=True, frozen_graph=FrozenGraph(W0, CI, 64, 19))
    p0, s0 = edge.engine.params.cpu().numpy().copy(), edge.engine.stats.cpu().numpy().copy()
    other = Wt.unpack(SPEC, c["base_p"], c["base_s"])
    for name, bad in malformed(c)[::2]:
        with pytest.raises(hip.AmsHipError, match="rejected"):
            edge.apply_delta(bad, strategy, base_variables=other, fmt="q8")
        assert bits_equal(edge.engine.params.cpu().numpy(), p0) and bits_equal(edge.engine.stats.cpu().numpy(), s0), name
    edge.close_model()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_nonfinite_masked_change_refuses_encoding(eng, bad):
    guarded.reset()
    c = case("full_model", "tenth")
    L = c["layout"]
    i = c["special"]["last"][0]                              # its last element is masked
    params, stats = c["params"].copy(), c["stats"].copy()
    Q.layout_views(L, params, stats)[i][-1] = bad
    set_variables(eng, params, stats)
    base_p, base_s = guarded.inp(c["base_p"]), guarded.inp(c["base_s"])
    mask = flat_mask(c["masks"])
    _, size, status = encode(eng, L, mask, base_p, base_s, 1, len(c["payload"]), written=False)
    assert (size, status) == (0, hip.DELTA_Q8_NONFINITE)
    assert bits_equal(base_p.cpu().numpy(), c["base_p"]) and bits_equal(base_s.cpu().numpy(), c["base_s"])
    eng.set_delta_base((base_p, base_s))
    with pytest.raises(hip.AmsHipError, match="NaN or infinite"):
        eng.encode_delta(L, mask, fmt="q8", advance_base=True)
    assert bits_equal(base_p.cpu().numpy(), c["base_p"]) and bits_equal(base_s.cpu().numpy(), c["base_s"])
    # the same value outside the mask is not looked at
    params, stats = c["params"].copy(), c["stats"].copy()
    j = c["special"]["single"][0]
    assert not c["masks"][j][0]
    Q.layout_views(L, params, stats)[j][0] = bad
    set_variables(eng, params, stats)
    got, size, status = encode(eng, L, mask, base_p, base_s, 0, len(c["payload"]))
    assert status == hip.DELTA_OK and got.tobytes() == c["payload"]
    eng.set_delta_base(None)


@pytest.mark.parametrize("strategy", STRATEGIES)
def test_a_cap_one_byte_short_writes_nothing(eng, strategy):
    guarded.reset()
    c = case(strategy, "tenth")
    L, n = c["layout"], len(c["payload"])
    set_variables(eng, c["params"], c["stats"])
    base_p, base_s = guarded.inp(c["base_p"]), guarded.inp(c["base_s"])
    mask = flat_mask(c["masks"])
    _, size, status = encode(eng, L, mask, base_p, base_s, 1, n - 1, written=False)
    assert (size, status) == (n, hip.DELTA_OK)              # the caller sees payload_bytes > payload_cap
    assert bits_equal(base_p.cpu().numpy(), c["base_p"]) and bits_equal(base_s.cpu().numpy(), c["base_s"])
    eng.set_delta_base((base_p, base_s))
    with pytest.raises(hip.AmsHipError, match="nothing was written"):
        eng.encode_delta(L, mask, cap=n - 1, fmt="q8", advance_base=True)
    assert bits_equal(base_p.cpu().numpy(), c["base_p"]) and bits_equal(base_s.cpu().numpy(), c["base_s"])
    assert eng.encode_delta(L, mask, cap=n, fmt="q8").cpu().numpy().tobytes() == c["payload"]
    eng.set_delta_base(None)
    with pytest.raises(hip.AmsHipError, match="no base"):
        eng.encode_delta(L, mask, fmt="q8")


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("density", ["tenth", "all"])
def test_advance_base_follows_the_decoder_and_feeds_the_error_back(eng, strategy, density):
    guarded.reset()
    c = case(strategy, density)
    L, masks = c["layout"], c["masks"]
    set_variables(eng, c["params"], c["stats"])
    base_p, base_s = guarded.inp(c["base_p"]), guarded.inp(c["base_s"])
    mask = flat_mask(masks)
    got, size, status = encode(eng, L, mask, base_p, base_s, 1, len(c["payload"]))
    assert status == hip.DELTA_OK and got.tobytes() == c["payload"]
    # the base now holds what the edge decodes: the oracle's decode on the masked elements, its own bits elsewhere
    adv_p, adv_s = base_p.cpu().numpy(), base_s.cpu().numpy()
    assert bits_equal(adv_p, c["decoded"][0]) and bits_equal(adv_s, c["decoded"][1])
    # unchanged variables, encoded against the advanced base: the oracle's bytes again, and decoded onto that base every element is inside
    # the bound of ITS scale (127 times finer at least): the first update's error is what travels, it is not added to
    want2 = Q.encode_q8(c["vals"], Q.layout_views(L, adv_p, adv_s), masks)
    got2, size2, status2 = encode(eng, L, mask, base_p, base_s, 0, len(want2))
    assert status2 == hip.DELTA_OK and got2.tobytes() == want2
    dec2 = Q.decode_q8(want2, L, adv_p, adv_s)
    set_variables(eng, adv_p, adv_s)
    assert apply(eng, L, want2)[1] == hip.DELTA_OK
    assert bits_equal(eng.params.cpu().numpy(), dec2[0]) and bits_equal(eng.stats.cpu().numpy(), dec2[1])
    check_decoded(L, masks, c["vals"], Q.layout_views(L, adv_p, adv_s), Q.layout_views(L, *dec2))
    first = Q.scales_and_codes(c["vals"], c["bases"], masks)
    second = Q.scales_and_codes(c["vals"], Q.layout_views(L, adv_p, adv_s), masks)
    # (scale2 = amax2 / 127 with amax2 inside the first bound: 0.5 scale1 + 2^-22 x at most 60, and that term / 127 is below 2^-20)
    finer = [s2 <= s1 * np.float32(0.51 / 127) + np.float32(2.0 ** -20) for (s1, _), (s2, _) in zip(first, second) if s1 > 0]
    assert len(finer) > 50 and all(finer)


def test_a_variable_outside_its_region_is_refused_behind_the_handle(eng):
    guarded.reset()
    L = D.delta_layout(SPEC, "full_model")
    src = L.table()
    t = (hip.DeltaVar * len(src))()
    for d, s in zip(t, src):
        d.region, d.reserved, d.offset, d.count, d.mask_offset = s.region, 0, s.offset, s.count, s.mask_offset
    last_stat = max((i for i, e in enumerate(L.entries) if e.region == hip.REGION_STATS), key=lambda i: L.entries[i].offset)
    t[last_stat].offset += 1
    n = len(t)
    scratch = guarded.scratch(int(eng.lib.ams_student_encode_delta_q8_scratch(t, n)), torch.int64)
    words = guarded.scratch(2, torch.int64)
    base_p, base_s = guarded.scratch(SPEC.n_trainable), guarded.scratch(SPEC.n_stats)
    out = guarded.scratch(L.max_payload_bytes_q8, torch.uint8)
    rc = eng.lib.ams_student_encode_delta_q8(eng._h, None, t, n, _ptr(base_p), _ptr(base_s), 0, _ptr(out), out.numel(), _ptr(words), _ptr(words, 8),
                                             _ptr(scratch), scratch.numel(), eng._stream())
    assert rc == -1 and b"outside its region" in eng.lib.ams_last_error()
    rc = eng.lib.ams_student_apply_delta_q8(eng._h, _ptr(out), out.numel(), t, n, _ptr(words), _ptr(words, 8), _ptr(scratch), scratch.numel(), eng._stream())
    assert rc == -1 and b"outside its region" in eng.lib.ams_last_error()
    guarded.check("refused calls")
    for b in (scratch, words, base_p, base_s, out):
        assert bool(guarded.poisoned(b).all())


def _frozen(W, H=64, **kw):
    return SemanticNetwork("unused", class_weights_exp=CW, height=H, frozen=True, frozen_graph=FrozenGraph(W, CI, H, 19), **kw)


@pytest.mark.parametrize("strategy,device_masks", [("coord_desc_rand", False), ("full_model", False), ("coord_desc_rand", True)])
def test_round_trip_through_semantic_network(strategy, device_masks, W0):
    H = 64
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=2).clip()
    kw = {"device_masks": True} if device_masks else {}
    server = SemanticNetwork("unused", class_weights_exp=CW, height=H, scale=[1], mini_batch_size=2, lr=1e-3, coord_frac=0.1,
                             masked_gradients=strategy != "full_model", initial_variables=W0, **kw)
    np.random.seed(3)
    random.seed(3)
    server.train_with_deque(deque(frames), deque(labels), 2, strategy)
    payload = server.delta_payload(fmt="q8")
    assert server.delta_payload(fmt="q8", device=True).cpu().numpy().tobytes() == payload
    L = D.delta_layout(SPEC, strategy)
    masks = [np.asarray(m).reshape(-1) for m in server.curr_mask]
    trained = server.engine.get_variables()
    p0, s0 = Wt.pack_trainable(SPEC, W0), Wt.pack_stats(SPEC, W0)
    p1, s1 = Wt.pack_trainable(SPEC, trained), Wt.pack_stats(SPEC, trained)
    assert payload == Q.encode_q8(Q.layout_views(L, p1, s1), Q.layout_views(L, p0, s0), masks)
    assert len(payload) == L.mask_bytes + 4 * len(L.entries) + sum(int(m.sum()) for m in masks) < len(server.delta_payload())
    server.close_model()

    want = Wt.unpack(SPEC, *Q.decode_q8(payload, L, p0, s0))
    check_decoded(L, masks, Q.layout_views(L, p1, s1), Q.layout_views(L, p0, s0), Q.layout_views(L, *Q.decode_q8(payload, L, p0, s0)))
    edge = _frozen(W0, pipeline_depth=2)
    old, fresh = _frozen(W0), _frozen(want)
    before = [edge.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1]) for k in range(3)]    # one pass launched, one frame queued
    assert edge.apply_delta(payload, strategy, fmt="q8") == sum(int(m.sum()) for m in masks)
    after = [edge.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1]) for k in range(3)]
    got = edge.engine.get_variables()
    for name in SPEC.all_variable_names():
        assert bits_equal(got[name], want[name]), name
    for tickets, ref in ((before, old), (after, fresh)):       # queued frames see the old model; the edge re-froze for the new one
        for k, t in enumerate(tickets):
            a = edge.collect(t)
            b = ref.predict_with_metric(frames[k:k + 1], labels[k:k + 1])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, ref is old)
    assert edge.engine.f16_fallback_layers() == fresh.engine.f16_fallback_layers()
    # a second update onto the base the server used, given explicitly: the same model again
    assert edge.apply_delta(payload, strategy, base_variables=W0, fmt="q8") > 0
    got = edge.engine.get_variables()
    assert all(bits_equal(got[name], want[name]) for name in SPEC.all_variable_names())
    for n in (old, fresh, edge):
        n.close_model()
