"""Edge-side model updates: the downlink delta decoded on the device (k_delta.hip, StudentEngine.apply_delta, SemanticNetwork.apply_delta).

  a. the device decoder equals the NumPy decoder bit for bit, at several mask densities and on fp16 edge cases, in both layouts;
  b. a malformed payload raises and leaves params and stats bit-identical;
  c. the server's delta_payload applied to a frozen edge gives the fp16-rounded server model, and the edge's results equal those of a frozen
     network built fresh from that model;
  d. an update without a masked value re-freezes to the same bits;
  e. frames submitted asynchronously before an update are answered by the old model, those after it by the new one;
  f. an update that moves a layer off the fp16 product form makes an earlier GraphedPredict refuse to replay.
"""
import random
from collections import deque

import numpy as np
import pytest
import torch

from ams_amd import delta as D, exp_configs, hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
from test_delta_layout_cpu import decode, encode, layout_vars

pytestmark = pytest.mark.gpu

CI = [0, 1, 2, 10, 11, 13]
SPEC = S.build_spec()
CW = exp_configs.class_weights(25)


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(SPEC, seed=0)


def flat(W):
    return Wt.pack_trainable(SPEC, W), Wt.pack_stats(SPEC, W)


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def masks_for(L, density, rng):
    sizes = [e.count for e in L.entries]
    if density == "zero":
        return [np.zeros(n, bool) for n in sizes]
    if density == "one":
        m = [np.zeros(n, bool) for n in sizes]
        m[-1][-1] = True
        return m
    if density == "tenth":
        return [rng.random(n) < 0.1 for n in sizes]
    return [np.ones(n, bool) for n in sizes]


def server_values(L, rng):
    """random values with fp16 edge cases: +-0, subnormals, 65504, values that overflow to +-inf, values that round to them"""
    p = rng.standard_normal(SPEC.n_trainable).astype(np.float32)
    s = rng.standard_normal(SPEC.n_stats).astype(np.float32)
    special = np.array([0.0, -0.0, 2.0 ** -24, -2.0 ** -20, 3e-8, 65504.0, -65504.0, 65520.0, 1e5, -1e6, np.float32(np.inf), 6.1e-5],
                       np.float32)
    p[:special.size] = special
    p[-special.size:] = special
    s[:special.size] = special
    return p, s


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_decoder_matches_numpy_bit_for_bit(strategy, W0):
    rng = np.random.default_rng(1)
    L = D.delta_layout(SPEC, strategy)
    eng = StudentEngine(CI, 64, 128, max_batch=1, trainable=False)
    base_p, base_s = flat(W0)
    sp, ss = server_values(L, rng)
    for density in ("zero", "one", "tenth", "all"):
        masks = masks_for(L, density, rng)
        if density != "zero":
            for m in masks[:2]:
                m[:12] = True                                   # the fp16 edge cases are always sent
        with np.errstate(over="ignore"):
            payload = encode(layout_vars(SPEC, L, sp, ss), masks)
        eng.load_variables(W0)
        for as_tensor in (False, True):
            eng.load_variables(W0)
            arg = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(eng.device) if as_tensor else payload
            n = eng.apply_delta(arg, L)
            assert n == sum(int(m.sum()) for m in masks)
            want_p, want_s = decode(payload, L, base_p, base_s)
            assert bits_equal(eng.params.cpu().numpy(), want_p), (strategy, density, as_tensor)
            assert bits_equal(eng.stats.cpu().numpy(), want_s), (strategy, density, as_tensor)
    eng.close()


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_malformed_payload_raises_and_changes_nothing(strategy, W0):
    rng = np.random.default_rng(2)
    L = D.delta_layout(SPEC, strategy)
    eng = StudentEngine(CI, 64, 128, max_batch=1, trainable=False)
    eng.load_variables(W0)
    sp, ss = server_values(L, rng)
    masks = masks_for(L, "tenth", rng)
    with np.errstate(over="ignore"):
        good = encode(layout_vars(SPEC, L, sp, ss), masks)
    padded = bytearray(good)
    e = next(e for e in L.entries if e.count % 8)
    padded[e.mask_offset + e.count // 8] |= 1                 # the last padding bit of that variable
    p0, s0 = eng.params.cpu().numpy().copy(), eng.stats.cpu().numpy().copy()
    for bad in (good[:-1], good + b"\0", bytes(padded), b"", good[:L.mask_bytes - 3]):
        with pytest.raises(hip.AmsHipError, match="rejected"):
            eng.apply_delta(bad, L)
        assert bits_equal(eng.params.cpu().numpy(), p0) and bits_equal(eng.stats.cpu().numpy(), s0)
    dev = torch.from_numpy(np.frombuffer(good[:-1], np.uint8).copy()).to(eng.device)
    with pytest.raises(hip.AmsHipError, match="rejected"):
        eng.apply_delta(dev, L)
    assert bits_equal(eng.params.cpu().numpy(), p0) and bits_equal(eng.stats.cpu().numpy(), s0)
    assert eng.apply_delta(good, L) == sum(int(m.sum()) for m in masks)          # the engine is still usable
    eng.close()


def _frozen(W, H=64, **kw):
    return SemanticNetwork("unused", class_weights_exp=CW, height=H, frozen=True, frozen_graph=FrozenGraph(W, CI, H, 19), **kw)


def _expected_variables(W0, net, strategy):
    """the initial model with the server's masked values rounded to fp16 (coord_desc_*), or every variable rounded (full_model)"""
    L = D.delta_layout(SPEC, strategy)
    out = {k: np.array(v, np.float32) for k, v in W0.items()}
    for e, p, m in zip(L.entries, net.train_params, net.curr_mask):
        a = out[e.name].reshape(-1)
        with np.errstate(over="ignore"):
            a[np.asarray(m).reshape(-1)] = np.asarray(p, np.float32).reshape(-1)[np.asarray(m).reshape(-1)].astype(np.float16).astype(np.float32)
    return out


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_round_trip_through_semantic_network(strategy, W0):
    H = 64
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=2).clip()
    server = SemanticNetwork("unused", class_weights_exp=CW, height=H, scale=[1], mini_batch_size=2, lr=1e-3, coord_frac=0.1,
                             masked_gradients=strategy != "full_model", initial_variables=W0)
    np.random.seed(3)
    random.seed(3)
    server.train_with_deque(deque(frames), deque(labels), 2, strategy)
    payload = server.delta_payload()
    want = _expected_variables(W0, server, strategy)
    server.close_model()

    edge = _frozen(W0)
    n = edge.apply_delta(payload, strategy)
    assert n == sum(int(np.sum(m)) for m in edge_masks(payload, strategy))
    got = edge.engine.get_variables()
    for name in SPEC.all_variable_names():
        assert bits_equal(got[name], want[name]), name
    if strategy != "full_model":
        for v in SPEC.stats:
            assert bits_equal(got[v.name], W0[v.name]), v.name
    fresh = _frozen(want)
    for k in range(len(frames)):
        a = edge.predict_with_metric(frames[k:k + 1], labels[k:k + 1])
        b = fresh.predict_with_metric(frames[k:k + 1], labels[k:k + 1])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert np.float32(a[4]).tobytes() == np.float32(b[4]).tobytes()
    assert edge.engine.f16_fallback_layers() == fresh.engine.f16_fallback_layers()
    edge.close_model()
    fresh.close_model()


def edge_masks(payload, strategy):
    L = D.delta_layout(SPEC, strategy)
    buf = np.frombuffer(payload, np.uint8)
    return [np.unpackbits(buf[e.mask_offset:e.mask_offset + (e.count + 7) // 8])[:e.count] for e in L.entries]


def test_empty_update_refreezes_to_the_same_bits(W0):
    H = 512
    frames, _ = synth.SyntheticVideo(H, 1, CI, seed=4).clip()
    eng = StudentEngine(CI, H, 2 * H, max_batch=1, trainable=False)
    eng.load_variables(W0)
    eng.freeze()
    g = eng.graphed_predict(1)
    lab0 = eng.predict(frames).cpu().numpy()
    logit0 = eng.logits_lowres.cpu().numpy().copy()
    glab0 = g(frames).cpu().numpy()
    L = D.delta_layout(SPEC, "coord_desc_rand")
    assert eng.apply_delta(bytes(L.mask_bytes), L) == 0
    eng.freeze()
    lab1 = eng.predict(frames).cpu().numpy()
    assert np.array_equal(lab0, lab1) and bits_equal(eng.logits_lowres.cpu().numpy(), logit0)
    assert np.array_equal(g(frames).cpu().numpy(), glab0)          # nothing applied: the graph replays as before
    eng.close()


def test_async_frames_before_an_update_see_the_old_model(W0):
    H = 64
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=5).clip()
    L = D.delta_layout(SPEC, "full_model")
    rng = np.random.default_rng(5)
    W1 = {k: (np.asarray(v) * np.float32(1.0 + 0.2 * rng.standard_normal())).astype(np.float32) for k, v in W0.items()}
    masks = [np.ones(e.count, bool) for e in L.entries]
    payload = encode([W1[e.name].reshape(-1) for e in L.entries], masks)
    want = {k: v.astype(np.float16).astype(np.float32) for k, v in W1.items()}
    old, new = _frozen(W0), _frozen(want)
    edge = _frozen(W0, pipeline_depth=2)
    before = [edge.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1]) for k in range(3)]    # one pass launched, one frame queued
    edge.apply_delta(payload, "full_model")
    after = [edge.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1]) for k in range(3)]
    for tickets, ref in ((before, old), (after, new)):
        for k, t in enumerate(tickets):
            a = edge.collect(t)
            b = ref.predict_with_metric(frames[k:k + 1], labels[k:k + 1])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (k, ref is old)
    for n in (old, new, edge):
        n.close_model()


def test_graph_captured_before_a_fallback_change_refuses_to_replay(W0):
    """aspp0 scaled by 2^-12 with its BN compensating: every weight below 2^-10, so the re-freeze moves it to the three-part bf16 form"""
    H = 64
    frames, labels = synth.SyntheticVideo(H, 2, CI, seed=6).clip()
    scope, f = "aspp0", np.float32(2.0 ** -12)
    names = [scope + "/weights:0", scope + "/BatchNorm/gamma:0", scope + "/BatchNorm/moving_mean:0"]
    W1 = dict(W0)
    W1[names[0]] = W0[names[0]] * f
    W1[names[1]] = W0[names[1]] / f
    W1[names[2]] = W0[names[2]] * f
    assert np.abs(W1[names[0]]).max() < 2.0 ** -10
    L = D.delta_layout(SPEC, "full_model")
    masks = [np.full(e.count, e.name in names) for e in L.entries]
    payload = encode([np.asarray(W1[e.name]).reshape(-1) for e in L.entries], masks)
    want = dict(W0)
    for nm in names:
        want[nm] = W1[nm].astype(np.float16).astype(np.float32)
    edge = _frozen(W0)
    g = edge.engine.graphed_predict(1)
    g(frames[:1])
    assert edge.engine.f16_fallback_layers() == 0
    edge.apply_delta(payload, "full_model")
    assert edge.engine.f16_fallback_layers() >= 1
    with pytest.raises(hip.AmsHipError, match="capture a new one"):
        g(frames[:1])
    fresh = _frozen(want)
    assert fresh.engine.f16_fallback_layers() == edge.engine.f16_fallback_layers()
    a = edge.predict_with_metric(frames[:1], labels[:1])
    b = fresh.predict_with_metric(frames[:1], labels[:1])
    assert np.isfinite(a[4]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    g2 = edge.engine.graphed_predict(1)                            # a graph captured after the update replays
    assert np.array_equal(g2(frames[:1]).cpu().numpy(), a[0])
    edge.close_model()
    fresh.close_model()
