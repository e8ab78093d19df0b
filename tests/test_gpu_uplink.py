"""The uplink frame codec on the device (k_uplink.hip; ams_uplink_*; ams_amd.uplink.UplinkCodec), held to the NumPy oracle of
tests/uplink_ref.py byte for byte.  Every buffer a kernel is handed is a guarded one (tests/guarded.py), the scratch exact and poisoned, the
payload at an even and at an odd address.  A payload byte or a pixel may well be 255, the byte pattern of the poison, so payloads and frames
are `scratch` buffers judged here: compared with the oracle's whole, or asserted to hold the pattern everywhere when nothing may be written.

Shapes: 16 x 16 = one macroblock, one short slice per plane; 16 x 144 = a Y slice that wraps a block row, 32 + 4 blocks; 48 x 80 = 32 + 28
blocks, 15 chroma blocks; 128 x 256 = exact multiples of 32, the size --height 64 encodes.
Contents (uplink_ref.frames): a constant frame; uniform noise, at q = 100 for the longest codes and the largest levels; saturated primaries for
the clamps; a +-checkerboard; a synthetic clip frame.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from ams_amd import hip
from ams_amd.uplink import UplinkCodec, UplinkRefused
import guarded
import uplink_ref as U

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16), (16, 144), (48, 80), (128, 256)]
CONTENTS = ("constant", "noise", "primaries", "checker", "clip")


@functools.lru_cache(maxsize=None)
def frames(shape):
    return U.frames(*shape)


@functools.lru_cache(maxsize=None)
def reference(shape, name):
    """the oracle's answers for one frame, computed once: sizes, and per tested quality the payload and its decode"""
    frame = frames(shape)[name]
    planes = U.transform(frame)
    sizes = np.array([U.payload_size(planes, q) for q in range(1, 101)], np.int64)
    budgets = [int(sizes[0]) - 1, int(np.median(sizes)), int(sizes[99])]
    qualities = sorted({100 if name == "noise" else 50, 1} | {U.choose_quality(sizes, b)[0] for b in budgets})
    payloads = {q: U.encode(frame, q, planes) for q in qualities}
    decoded = {q: U.decode(p, *shape) for q, p in payloads.items()}
    return dict(frame=frame, sizes=sizes, budgets=budgets, payloads=payloads, decoded=decoded)


def _ptr(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def transform_and_sizes(lib, frame):
    """ams_uplink_transform and ams_uplink_size_table on guarded buffers -> (the scratch, the 100 sizes)"""
    H, W = frame.shape[:2]
    src = guarded.inp(frame, torch.uint8)
    scratch = guarded.scratch(int(lib.ams_uplink_encode_scratch(H, W)), torch.uint8)
    sizes = guarded.out(100, torch.int64)
    hip.check(lib.ams_uplink_transform(_ptr(src), H, W, _ptr(scratch), scratch.numel(), _stream()), "ams_uplink_transform")
    hip.check(lib.ams_uplink_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes), _stream()), "ams_uplink_size_table")
    guarded.check("ams_uplink_transform + ams_uplink_size_table")
    return scratch, sizes.cpu().numpy()


def encode(lib, scratch, shape, q, cap, odd=False, written=True):
    """ams_uplink_encode into a payload buffer of exactly `cap` bytes (behind one more byte when `odd`) -> (bytes, size, status)"""
    out = guarded.scratch(cap + int(odd), torch.uint8)
    size, status = guarded.out(1, torch.int64), guarded.out(1, torch.int32)
    hip.check(lib.ams_uplink_encode(_ptr(scratch), scratch.numel(), shape[0], shape[1], q, _ptr(out, int(odd)), cap, _ptr(size), _ptr(status), _stream()),
              "ams_uplink_encode")
    guarded.check("ams_uplink_encode")
    kept = guarded.poisoned(out)
    assert bool(kept[:int(odd)].all()) and (written or bool(kept.all()))          # the byte in front of an odd start; a refused payload
    return out.cpu().numpy()[int(odd):].tobytes(), int(size.item()), int(status.item())


def decode(lib, payload, shape, odd=False):
    """ams_uplink_decode of a guarded payload (at an odd address when `odd`) with exact poisoned scratch -> (the frame buffer, status)"""
    H, W = shape
    buf = guarded.inp(np.concatenate([np.zeros(int(odd), np.uint8), np.frombuffer(payload, np.uint8)]), torch.uint8)
    n = buf.numel() - int(odd)
    out = guarded.scratch(H * W * 3, torch.uint8)
    status = guarded.out(1, torch.int32)
    scratch = guarded.scratch(int(lib.ams_uplink_decode_scratch(H, W)), torch.uint8)
    hip.check(lib.ams_uplink_decode(_ptr(buf, int(odd)) if n else None, n, H, W, _ptr(out), _ptr(status), _ptr(scratch), scratch.numel(), _stream()),
              "ams_uplink_decode")
    guarded.check("ams_uplink_decode")
    return out, int(status.item())


@pytest.mark.parametrize("name", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_encoder_and_decoder_match_the_oracle(shape, name):
    guarded.reset()
    lib = hip.lib()
    ref = reference(shape, name)
    scratch, sizes = transform_and_sizes(lib, ref["frame"])
    assert np.array_equal(sizes, ref["sizes"]), (np.nonzero(sizes != ref["sizes"])[0][:5], sizes[:3], ref["sizes"][:3])
    for q, want in ref["payloads"].items():
        for odd in (False, True):
            got, size, status = encode(lib, scratch, shape, q, len(want), odd)
            assert (size, status) == (len(want), hip.UPLINK_OK), (q, odd)
            assert got == want, (q, odd, int(np.nonzero(np.frombuffer(got, np.uint8) != np.frombuffer(want, np.uint8))[0][0]))
            out, status = decode(lib, want, shape, odd)
            assert status == hip.UPLINK_OK and np.array_equal(out.cpu().numpy().reshape(shape + (3,)), ref["decoded"][q]), (q, odd)
    # a cap one byte short writes nothing, and says how much room it takes
    q, want = max(ref["payloads"].items())
    got, size, status = encode(lib, scratch, shape, q, len(want) - 1, written=False)
    assert (size, status) == (len(want), hip.UPLINK_NO_ROOM)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=lambda s: "%dx%d" % s)
def test_malformed_payloads_are_refused_and_write_nothing(shape):
    guarded.reset()
    lib = hip.lib()
    good = U.encode(frames(shape)["clip"], 50)
    for name, (bad, want) in U.malformed(good, *shape).items():
        for odd in (False, True):
            out, status = decode(lib, bad, shape, odd)
            assert status == want, (name, odd, status)
            assert bool(guarded.poisoned(out).all()), (name, odd)
    two = bytearray(U.malformed(good, *shape)["zero_level"][0])
    two[-1] |= 1                                                 # a second malformed slice: the larger code stands
    out, status = decode(lib, bytes(two), shape)
    assert status == U.parse(bytes(two), *shape)[2] and bool(guarded.poisoned(out).all())


@pytest.fixture(scope="module")
def codec():
    return UplinkCodec("cuda:0")


@pytest.mark.parametrize("name", ("clip", "noise"))
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=lambda s: "%dx%d" % s)
def test_codec_class_follows_the_rate_rule(codec, shape, name):
    ref = reference(shape, name)
    assert np.array_equal(codec.size_table(ref["frame"]), ref["sizes"])
    assert codec.max_payload_bytes(*shape) == U.max_bytes(*shape)
    for budget in ref["budgets"]:
        q, fits = U.choose_quality(ref["sizes"], budget)
        for frame in (ref["frame"], torch.from_numpy(ref["frame"]).cuda()):          # a host array, a device tensor
            payload, got_q, got_fits = codec.encode_to_budget(frame, budget)
            assert (got_q, got_fits) == (q, fits) and payload.is_cuda and payload.dtype == torch.uint8
            assert payload.cpu().numpy().tobytes() == ref["payloads"][q], (budget, q)
        assert fits == (budget >= ref["sizes"][0]) and (not fits or len(ref["payloads"][q]) <= budget)
        for given in (payload, ref["payloads"][q]):                                  # its own payload on the device, the oracle's from the host
            assert np.array_equal(codec.decode(given).cpu().numpy(), ref["decoded"][q])
    q = max(ref["payloads"])
    assert codec.encode(ref["frame"], q).cpu().numpy().tobytes() == ref["payloads"][q]


def test_codec_class_raises_on_a_refused_payload(codec):
    shape = SHAPES[2]
    good = U.encode(frames(shape)["clip"], 50)
    for name, (bad, want) in U.malformed(good, *shape).items():
        with pytest.raises(UplinkRefused) as e:
            codec.decode(bad)
        if name not in ("height", "width", "short_header", "empty"):                 # those the class meets before the device does
            assert e.value.status == want, name
    with pytest.raises(ValueError):
        codec.encode(np.zeros((24, 32, 3), np.uint8), 50)
    with pytest.raises(ValueError):
        codec.encode(frames(shape)["clip"], 0)
