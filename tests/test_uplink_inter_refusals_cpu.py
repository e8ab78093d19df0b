"""What the ams_uplink_inter_* entries refuse on the host, in which order, with AMS_E_INVALID and which word in ams_last_error(): the table of
tests/test_uplink_refusals_cpu.py over the predicted frame's entries.  The order is the same: no pixels; the shape rule (the encoder: or the
quality); the scratch; null pointers, the reference among them; the scratch's alignment; a negative byte count.

No row reaches a launch: EVERY call here carries a fault and the tests assert that it is refused; the pointers are addresses nobody reads.  The
sizes the _scratch and max_bytes entries answer are the NumPy oracle's."""
import ctypes as C

import pytest

from ams_amd import hip
import uplink_ref as U
import uplink_inter_ref as P

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, 16-byte aligned, never dereferenced
ODD = C.c_void_p(0x10001)
E_INVALID = -1
H, W = 48, 80


def _args(**over):
    a = dict(H=H, W=W, q=50, scratch=UNREAD, short=0, frame=UNREAD, ref=UNREAD, sizes=UNREAD, payload=UNREAD, cap=1 << 20, nbytes=UNREAD,
             status=UNREAD, n=100, out=UNREAD)
    a.update(over)
    return a


def _call(entry, a):
    lib = hip.lib()
    enc = lib.ams_uplink_inter_encode_scratch(H, W) - a["short"]
    dec = lib.ams_uplink_inter_decode_scratch(H, W) - a["short"]
    if entry == "transform":
        return lib.ams_uplink_inter_transform(a["frame"], a["ref"], a["H"], a["W"], a["scratch"], enc, NULL)
    if entry == "size_table":
        return lib.ams_uplink_inter_size_table(a["scratch"], enc, a["H"], a["W"], a["sizes"], NULL)
    if entry == "encode":
        return lib.ams_uplink_inter_encode(a["scratch"], enc, a["H"], a["W"], a["q"], a["payload"], a["cap"], a["nbytes"], a["status"], NULL)
    assert entry == "decode"
    return lib.ams_uplink_inter_decode(a["payload"], a["n"], a["ref"], a["H"], a["W"], a["out"], a["status"], a["scratch"], dec, NULL)


ALL, ENC, DEC, REF = ("transform", "size_table", "encode", "decode"), ("encode",), ("decode",), ("transform", "decode")
POINTER = {"transform": "frame", "size_table": "sizes", "encode": "status", "decode": "status"}

# a fault per refusable argument, in the order of refusal: name -> (entries that take it, overrides, the word in the message)
FAULTS = {
    "empty": (ALL, dict(H=0), b"empty problem"),
    "shape": (ALL, dict(W=W + 8), b"unsupported shape"),
    "scratch": (ALL, dict(short=1), b"scratch too small"),
    "pointer": (ALL, None, b"null pointer"),                     # the entry's own pointer: POINTER
    "alignment": (ALL, dict(scratch=ODD), b"not 16-byte aligned"),
    "cap": (ENC, dict(cap=-1), b"room for"),
    "bytes": (DEC, dict(n=-1, payload=UNREAD), b"payload bytes"),
}
RANK = list(FAULTS)

MORE = [("empty", ALL, dict(W=-16)), ("shape", ALL, dict(H=4112)), ("shape", ALL, dict(H=8, W=8)), ("shape", ALL, dict(H=40)),
        ("shape", ENC, dict(q=0)), ("shape", ENC, dict(q=101)), ("scratch", ALL, dict(scratch=NULL)), ("scratch", ALL, dict(short=128)),
        ("pointer", REF, dict(ref=NULL)), ("pointer", ENC, dict(payload=NULL)), ("pointer", ENC, dict(nbytes=NULL)), ("pointer", DEC, dict(out=NULL)),
        ("pointer", DEC, dict(payload=NULL, n=5))]


def _over(entry, fault, over=None):
    if over is None:
        over = FAULTS[fault][1]
    return {POINTER[entry]: NULL} if over is None else over


SINGLE = [(e, f, None) for f in RANK for e in FAULTS[f][0]] + [(e, f, o) for f, es, o in MORE for e in es]


def _id(v):
    if v is None or isinstance(v, str):
        return v or "-"
    return ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else "odd" if v[k] is ODD else "ptr" if v[k] is UNREAD else v[k]) for k in v)


def _refused(entry, a, word):
    assert _call(entry, a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("entry,fault,over", SINGLE, ids=_id)
def test_each_fault_is_refused_in_words(entry, fault, over):
    msg = _refused(entry, _args(**_over(entry, fault, over)), FAULTS[fault][2])
    assert ("uplink_inter_" + entry).encode() in msg


def _pairs():
    out = []
    for entry in ALL:
        mine = [f for f in RANK if entry in FAULTS[f][0]]
        out += [(entry, first, later) for i, first in enumerate(mine) for later in mine[i + 1:] if (first, later) != ("empty", "shape")]
    return out


@pytest.mark.parametrize("entry,first,later", _pairs())
def test_the_earlier_ranked_fault_wins(entry, first, later):
    """(no pixels and a bad shape are both said of H and W: that pair is one argument)"""
    msg = _refused(entry, _args(**dict(_over(entry, later), **_over(entry, first))), FAULTS[first][2])
    assert FAULTS[later][2] not in msg, msg


@pytest.mark.parametrize("entry", REF)
def test_the_reference_is_checked_with_the_other_pointers(entry):
    """behind the scratch's size, in front of its alignment"""
    _refused(entry, _args(ref=NULL, scratch=ODD), b"null pointer")
    _refused(entry, _args(ref=NULL, short=1), b"scratch too small")


def test_an_empty_payload_needs_no_pointer_but_everything_else():
    _refused("decode", _args(payload=NULL, n=0, scratch=ODD), b"not 16-byte aligned")
    _refused("decode", _args(payload=NULL, n=0, ref=NULL), b"null pointer")


@pytest.mark.parametrize("shape", [(16, 16), (16, 144), (48, 80), (128, 256), (1024, 2048), (4096, 4096)])
def test_sizes_are_the_oracles(shape):
    lib = hip.lib()
    h, w = shape
    blocks, slices, mbs = sum(U.plane_blocks(h, w)), P.slice_count(h, w), P.macroblocks(h, w)
    assert lib.ams_uplink_inter_max_bytes(h, w) == P.max_bytes(h, w)
    offsets, vectors = (4 * (slices + 1) + 15) // 16 * 16, (2 * mbs + 15) // 16 * 16
    assert lib.ams_uplink_inter_decode_scratch(h, w) == 128 * blocks + offsets + vectors
    assert lib.ams_uplink_inter_encode_scratch(h, w) == 128 * blocks + offsets + 400 * slices + vectors


@pytest.mark.parametrize("shape", [(0, 16), (16, 0), (-16, 16), (24, 16), (16, 8), (4112, 16), (16, 4112)])
def test_refused_sizes_answer_zero(shape):
    lib = hip.lib()
    assert lib.ams_uplink_inter_max_bytes(*shape) == 0 and lib.ams_uplink_inter_encode_scratch(*shape) == 0
    assert lib.ams_uplink_inter_decode_scratch(*shape) == 0


def test_the_status_words_extend_upward():
    assert (hip.UPLINK_NO_ROOM, hip.UPLINK_BAD_VECTOR, hip.UPLINK_BAD_ZERO_SLICE) == (U.NO_ROOM, P.BAD_VECTOR, P.BAD_ZERO_SLICE) == (8, 9, 10)
