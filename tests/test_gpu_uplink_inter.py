"""The predicted uplink frame on the device (k_uplink_inter.hip; ams_uplink_inter_*; UplinkCodec's reference= keyword), held to the NumPy oracle
of tests/uplink_inter_ref.py byte for byte: the search's vectors, the size table, the payload and the decode.  Buffers as in
tests/test_gpu_uplink.py: guarded (tests/guarded.py), the scratch exact and poisoned, the payload at an even and at an odd address; payloads
and frames may hold the poison's byte, so they are `scratch` buffers judged here.

Shapes: 16 x 16 = one macroblock, only the zero vector is legal; 16 x 144 = a Y slice that wraps a block row; 48 x 80 = short last slices and
a clipped search window on every border (the middle macroblock alone has all 961 candidates' rows, none has all columns); 128 x 256 = whole
slices, four motion slices, what --height 64 sends.
Pairs (uplink_inter_ref.pairs): the same frame twice (every slice of length 0); a noise texture moved by (3, -5) (interior macroblocks find
exactly that vector and no luma residual) and by (1, 1) (both chroma averages); two frames of the synthetic clip; two unrelated noise frames at
q = 100 (the longest codes); 0 under 255 and the reverse (the residual's range).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ams_amd import hip
from ams_amd import uplink as UL
import guarded
import uplink_ref as U
import uplink_inter_ref as P

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (16, 144), (48, 80), (128, 256)]
PAIRS = ("same", "shift", "odd", "clip", "unrelated", "extremes")
KIND = {P.INTRA: UL.INTRA, P.INTER: UL.INTER}


@functools.lru_cache(maxsize=None)
def pairs(shape):
    return P.pairs(*shape)


@functools.lru_cache(maxsize=None)
def reference(shape, name):
    """the oracle's answers for one pair, computed once: vectors, sizes, and per tested quality the payload and its decode"""
    cur, ref = pairs(shape)[name]
    analysed = P.analyse(cur, ref)
    sizes = P.size_table(cur, ref, analysed)
    qualities = sorted({100 if name == "unrelated" else 50, 1})
    payloads = {q: P.encode(cur, ref, q, analysed) for q in qualities}
    decoded = {q: P.decode(p, ref) for q, p in payloads.items()}
    return dict(cur=cur, ref=ref, vectors=analysed[0], planes=analysed[1], sizes=sizes, payloads=payloads, decoded=decoded)


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def transform_and_sizes(lib, cur, ref):
    """ams_uplink_inter_transform and _size_table on guarded buffers -> (the scratch, the 100 sizes, the vectors the scratch ends in)"""
    H, W = cur.shape[:2]
    src, prev = guarded.inp(cur, torch.uint8), guarded.inp(ref, torch.uint8)
    scratch = guarded.scratch(int(lib.ams_uplink_inter_encode_scratch(H, W)), torch.uint8)
    sizes = guarded.out(100, torch.int64)
    hip.check(lib.ams_uplink_inter_transform(_ptr(src), _ptr(prev), H, W, _ptr(scratch), scratch.numel(), _stream()), "ams_uplink_inter_transform")
    hip.check(lib.ams_uplink_inter_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes), _stream()), "ams_uplink_inter_size_table")
    guarded.check("ams_uplink_inter_transform + ams_uplink_inter_size_table")
    nmb = P.macroblocks(H, W)
    tail = scratch.cpu().numpy()[-((2 * nmb + 15) // 16 * 16):]
    return scratch, sizes.cpu().numpy(), tail[:2 * nmb].view(np.int8).astype(np.int64).reshape(-1, 2)


def encode(lib, scratch, shape, q, cap, odd=False, written=True):
    out = guarded.scratch(cap + int(odd), torch.uint8)
    size, status = guarded.out(1, torch.int64), guarded.out(1, torch.int32)
    hip.check(lib.ams_uplink_inter_encode(_ptr(scratch), scratch.numel(), shape[0], shape[1], q, _ptr(out, int(odd)), cap, _ptr(size), _ptr(status),
                                          _stream()), "ams_uplink_inter_encode")
    guarded.check("ams_uplink_inter_encode")
    kept = guarded.poisoned(out)
    assert bool(kept[:int(odd)].all()) and (written or bool(kept.all()))
    return out.cpu().numpy()[int(odd):].tobytes(), int(size.item()), int(status.item())


def decode(lib, payload, ref, odd=False, entry="inter"):
    """ams_uplink_inter_decode (or, entry="intra", ams_uplink_decode) of a guarded payload with exact poisoned scratch -> (frame buffer, status)"""
    H, W = ref.shape[:2]
    buf = guarded.inp(np.concatenate([np.zeros(int(odd), np.uint8), np.frombuffer(payload, np.uint8)]), torch.uint8)
    n = buf.numel() - int(odd)
    out = guarded.scratch(H * W * 3, torch.uint8)
    status = guarded.out(1, torch.int32)
    data = _ptr(buf, int(odd)) if n else None
    if entry == "inter":
        prev = guarded.inp(ref, torch.uint8)
        scratch = guarded.scratch(int(lib.ams_uplink_inter_decode_scratch(H, W)), torch.uint8)
        hip.check(lib.ams_uplink_inter_decode(data, n, _ptr(prev), H, W, _ptr(out), _ptr(status), _ptr(scratch), scratch.numel(), _stream()),
                  "ams_uplink_inter_decode")
    else:
        scratch = guarded.scratch(int(lib.ams_uplink_decode_scratch(H, W)), torch.uint8)
        hip.check(lib.ams_uplink_decode(data, n, H, W, _ptr(out), _ptr(status), _ptr(scratch), scratch.numel(), _stream()), "ams_uplink_decode")
    guarded.check("ams_uplink_%s_decode" % entry)
    return out, int(status.item())


def test_the_moved_texture_is_found_exactly():
    """what the `shift` pair is for, said of the oracle the device is held to: interior macroblocks, vector (3, -5), no luma level at q = 100"""
    shape = SHAPES[3]
    ref = reference(shape, "shift")
    mw = shape[1] // 16
    v = ref["vectors"].reshape(shape[0] // 16, mw, 2)
    assert np.array_equal(v[1:-1, 1:-1], np.broadcast_to([3, -5], v[1:-1, 1:-1].shape))
    luma = U.quantise(ref["planes"][0], 100, False).reshape(shape[0] // 8, shape[1] // 8, 64)
    assert not luma[2:-2, 2:-2].any() and luma.any()


@pytest.mark.parametrize("name", PAIRS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_encoder_and_decoder_match_the_oracle(shape, name):
    guarded.reset()
    lib = hip.lib()
    ref = reference(shape, name)
    scratch, sizes, vectors = transform_and_sizes(lib, ref["cur"], ref["ref"])
    assert np.array_equal(vectors, ref["vectors"]), (np.nonzero((vectors != ref["vectors"]).any(1))[0][:5], vectors[:3], ref["vectors"][:3])
    assert np.array_equal(sizes, ref["sizes"]), (np.nonzero(sizes != ref["sizes"])[0][:5], sizes[:3], ref["sizes"][:3])
    if shape == (16, 16):
        assert not vectors.any()
    if name == "same":
        assert np.array_equal(sizes, np.full(100, 16 + 2 * P.slice_count(*shape)))
    for q, want in ref["payloads"].items():
        for odd in (False, True):
            got, size, status = encode(lib, scratch, shape, q, len(want), odd)
            assert (size, status) == (len(want), hip.UPLINK_OK), (q, odd)
            assert got == want, (q, odd, int(np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0][0]))
            out, status = decode(lib, want, ref["ref"], odd)
            assert status == hip.UPLINK_OK and np.array_equal(out.cpu().numpy().reshape(shape + (3,)), ref["decoded"][q]), (q, odd)
    # a cap one byte short writes nothing, and says how much room it takes
    q, want = max(ref["payloads"].items())
    got, size, status = encode(lib, scratch, shape, q, len(want) - 1, written=False)
    assert (size, status) == (len(want), hip.UPLINK_NO_ROOM)


@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "%dx%d" % s)
def test_malformed_payloads_are_refused_and_write_nothing(shape):
    guarded.reset()
    lib = hip.lib()
    cur, ref = pairs(shape)["clip"]
    good = P.encode(cur, ref, 50)
    cases = P.malformed(good, *shape)
    for name, (bad, want) in cases.items():
        for odd in (False, True):
            out, status = decode(lib, bad, ref, odd)
            assert status == want, (name, odd, status)
            assert bool(guarded.poisoned(out).all()), (name, odd)
    two = bytearray(cases["window_top"][0])
    two[-1] |= 1                                                 # a second malformed slice with a smaller code: the larger stands
    want = P.parse(bytes(two), *shape)[3]
    out, status = decode(lib, bytes(two), ref)
    assert status == want == P.BAD_VECTOR and bool(guarded.poisoned(out).all())
    # each decoder refuses the other kind's payload
    for payload, entry in ((U.encode(cur, 50), "inter"), (good, "intra")):
        out, status = decode(lib, payload, ref, entry=entry)
        assert status == hip.UPLINK_BAD_HEADER and bool(guarded.poisoned(out).all()), entry


@pytest.fixture(scope="module")
def codec():
    return UL.UplinkCodec("cuda:0")


def test_four_frame_chain_holds_on_the_device(codec):
    """I P P P in the closed loop: every payload and every decoded frame is the oracle's, so nothing drifts"""
    from ams_amd import synth
    shape, q = SHAPES[2], 50
    video = synth.SyntheticVideo(shape[0], 1, [0, 1, 2, 10, 11, 13], seed=3)
    frames = [np.ascontiguousarray(video.frame(t)[0][:shape[0], :shape[1]]) for t in range(4)]
    payloads, decoded = P.chain(frames, q)
    prev = None
    for k, frame in enumerate(frames):
        payload = codec.encode(frame, q, reference=prev)
        assert payload.cpu().numpy().tobytes() == payloads[k], k
        assert UL.kind_of(payload) == (UL.INTER if k else UL.INTRA)
        prev = codec.decode(payload, reference=prev)             # the device's own frame feeds the next one
        assert np.array_equal(prev.cpu().numpy(), decoded[k]), k


@pytest.mark.parametrize("name", ("clip", "unrelated"))
@pytest.mark.parametrize("shape", SHAPES[2:], ids=lambda s: "%dx%d" % s)
def test_codec_class_follows_the_rate_rule(codec, shape, name):
    ref = reference(shape, name)
    cur, prev = ref["cur"], ref["ref"]
    intra = U.size_table(cur)
    assert np.array_equal(codec.size_table(cur, reference=prev), ref["sizes"])
    budgets = [int(min(intra[0], ref["sizes"][0])) - 1, int(np.median(intra)), int(np.median(ref["sizes"])), int(max(intra[99], ref["sizes"][99]))]
    kinds = set()
    for budget in budgets:
        want, q, fits, kind = P.encode_to_budget(cur, budget, prev)
        assert (kind, q, fits) == P.choose(intra, ref["sizes"], budget)
        for frame, given in ((cur, prev), (torch.from_numpy(cur).cuda(), torch.from_numpy(prev).cuda())):
            payload, got_q, got_fits = codec.encode_to_budget(frame, budget, reference=given)
            assert (got_q, got_fits) == (q, fits) and payload.is_cuda and payload.dtype == torch.uint8
            assert payload.cpu().numpy().tobytes() == want and UL.kind_of(payload) == KIND[kind], budget
        kinds.add(kind if fits else None)
        back = codec.decode(payload, reference=prev) if kind == P.INTER else codec.decode(payload)
        assert np.array_equal(back.cpu().numpy(), P.decode(want, prev) if kind == P.INTER else U.decode(want, *shape))
        # without a reference the call is the intra call
        payload, got_q, got_fits = codec.encode_to_budget(cur, budget)
        assert payload.cpu().numpy().tobytes() == U.encode_to_budget(cur, budget)[0]
    assert None in kinds and (P.INTER if name == "clip" else P.INTRA) in kinds          # unrelated frames: intra wins


def test_codec_class_raises_in_words(codec):
    shape = SHAPES[2]
    cur, prev = pairs(shape)["clip"]
    good = P.encode(cur, prev, 50)
    with pytest.raises(ValueError, match="reference"):
        codec.decode(good)
    for name in ("vector_dy_16", "window_bottom", "zero_motion_long", "zero_levels_long", "intra_magic"):
        bad, want = P.malformed(good, *shape)[name]
        with pytest.raises(UL.UplinkRefused) as e:
            codec.decode(bad, reference=prev)
        assert e.value.status == want and UL.STATUS_WORDS[want] in str(e.value), name
    with pytest.raises(UL.UplinkRefused):
        codec.decode(U.encode(cur, 50), reference=prev)
    with pytest.raises(AssertionError):
        codec.encode(cur, 50, reference=prev[:32])
