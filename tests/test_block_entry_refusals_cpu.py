"""What the six kernel-level entry points of the frozen blocks (ams_k_block_fused, _f16, ams_k_expand_dw, ams_k_expand_dw_stream, _f16,
ams_k_dw_project) refuse, in which order, with which return code and which word in ams_last_error(): one table over the refusable arguments.
The order is the one check every block launcher goes through (block_call_check: no pixels; the launcher's shape rule; the panel scratch; the
output format; the null pointers of what the launcher reads).  tests/test_first_block_cpu.py holds the two first-block entries to the same order.

No row reaches a device call.  Every row of the table passes a NULL input tensor, which each entry refuses ("null pointer") in front of its
first launch, the weight splits included, so even a row whose expected refusal went missing would end in AMS_E_INVALID and not in a kernel on
made-up addresses.  The other pointers are either NULL or an address nobody reads: the checks only compare them against NULL."""
import ctypes as C

import pytest

from ams_amd import hip

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1


def _need(entry, a):
    """The panel scratch the header asks for, in uint16."""
    if entry == "block_fused":
        return 3 * a["Cexp"] * 32
    if entry == "block_fused_f16":
        return 2 * a["Cexp"] * 32 + 2 * a["Cout"] * ((a["Cexp"] + 31) // 32 * 32)
    if entry == "dw_project":
        return 2 * a["Cout"] * a["Cexp"]
    if entry == "expand_dw":
        return 0
    parts = 2 if entry == "expand_dw_stream_f16" else 3
    return parts * a["Cexp"] * a["Cin"] + (parts * a["B"] * a["H"] * a["W"] * a["Cin"] if a["presplit"] else 0)


# the smallest supported shape of each entry
BLOCK = dict(Cin=16, Cexp=96, Cout=24, stride=2, residual=0)
STREAM = dict(Cin=64, Cexp=384, rate=1)
BASE = {"block_fused": BLOCK, "block_fused_f16": BLOCK, "expand_dw": dict(Cin=16, Cexp=96, stride=1, rate=1), "dw_project": dict(Cexp=384, Cout=64, rate=1)}
BASE.update({"expand_dw_stream/%d/%d" % (parts, pre): dict(STREAM, parts=parts, presplit=pre) for parts in (2, 3) for pre in (0, 1, 2)})
BASE.update({"expand_dw_stream_f16/%d" % pre: dict(STREAM, presplit=pre) for pre in (0, 1, 2)})
ALL = tuple(BASE)
PANELS = tuple(e for e in ALL if e != "expand_dw")


def _args(entry, **over):
    a = dict(B=1, H=2, W=3, x=NULL, v=UNREAD, y=UNREAD, res=NULL, panels=UNREAD, panel_elems=None, y_h2i=0)
    a.update(BASE[entry])
    a.update(over)
    if a["panel_elems"] is None:
        a["panel_elems"] = max(0, _need(entry.split("/")[0], a) + a.pop("short", 0))
    return a


def _call(entry, a):
    lib = hip.lib()
    name = entry.split("/")[0]
    v, size = a["v"], (a["B"], a["H"], a["W"])
    scratch = (a["panels"], a["panel_elems"])
    if name in ("block_fused", "block_fused_f16"):
        return getattr(lib, "ams_k_" + name)(a["x"], *size, a["Cin"], v, v, v, a["Cexp"], v, a["stride"], v, v, v, a["Cout"], v, v, a["residual"],
                                             a["y"], *scratch, NULL)
    if name == "expand_dw":
        return lib.ams_k_expand_dw(a["x"], *size, a["Cin"], v, v, v, a["Cexp"], v, a["stride"], a["rate"], v, v, a["y"], NULL)
    if name == "expand_dw_stream":
        return lib.ams_k_expand_dw_stream(a["x"], *size, a["Cin"], v, v, v, a["Cexp"], v, a["rate"], v, v, a["y"], *scratch, a["parts"], a["presplit"], NULL)
    if name == "expand_dw_stream_f16":
        return lib.ams_k_expand_dw_stream_f16(a["x"], *size, a["Cin"], v, v, v, a["Cexp"], v, a["rate"], v, v, a["y"], *scratch, a["presplit"], a["y_h2i"], NULL)
    assert name == "dw_project"
    return lib.ams_k_dw_project(a["x"], *size, a["Cexp"], v, a["rate"], v, v, v, a["Cout"], v, v, a["res"], a["y"], *scratch, NULL)


# a fault per refusable argument, in the order of refusal: name -> (entries that can be given it, overrides, the word in the message)
# ("short": the panel scratch that many elements off what the call needs)
FAULTS = {
    "size": (ALL, dict(H=0), b"no pixels"),
    "shape": (ALL, dict(rate=3, stride=3), b"unsupported shape"),
    "panels": (PANELS, dict(short=-1), b"panel scratch too small (need "),
}
RANK = list(FAULTS)
STREAMS = tuple(e for e in ALL if e.startswith("expand_dw_stream"))
BLOCKS = ("block_fused", "block_fused_f16")
# further values of a single fault: (fault, entries, overrides)
MORE = [("size", ALL, dict(B=0)), ("size", ALL, dict(W=-5)), ("size", ALL, dict(B=-1, H=-1)),
        ("shape", BLOCKS, dict(Cexp=100)), ("shape", BLOCKS, dict(Cin=48)), ("shape", BLOCKS, dict(residual=1)), ("shape", BLOCKS, dict(Cout=68)),
        ("shape", ("expand_dw",), dict(Cin=96)), ("shape", ("expand_dw",), dict(Cexp=80)), ("shape", ("expand_dw",), dict(rate=2)),
        ("shape", STREAMS, dict(Cin=48)), ("shape", STREAMS, dict(Cexp=24)), ("shape", STREAMS[:6], dict(parts=1)), ("shape", STREAMS[:6], dict(parts=4)),
        ("shape", STREAMS[6:], dict(Cin=32)),                    # the fp16 parts exist from 64 channels on
        ("shape", ("dw_project",), dict(Cexp=48)), ("shape", ("dw_project",), dict(Cout=24)), ("shape", ("dw_project",), dict(Cout=7 * 16)),
        ("panels", PANELS[1:], dict(panels=NULL)), ("panels", PANELS, dict(panel_elems=0))]
# (ams_k_block_fused with panels = NULL is the exact-f32 form: no fault)

SINGLE = [(e, f, FAULTS[f][1], FAULTS[f][2]) for f in RANK for e in FAULTS[f][0]] + [(e, f, o, FAULTS[f][2]) for f, es, o in MORE for e in es]


def _id(v):
    if isinstance(v, bytes):
        return v.decode()
    return v if isinstance(v, str) else ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else "ptr" if v[k] is UNREAD else v[k]) for k in v)


def _refused(entry, a, word):
    assert _call(entry, a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("entry,fault,over,word", SINGLE, ids=_id)
def test_each_fault_is_refused_in_words(entry, fault, over, word):
    a = _args(entry, **over)
    msg = _refused(entry, a, word)
    assert msg.startswith(entry.split("/")[0].encode() + b":"), msg          # the called entry's name
    if fault == "panels":
        assert b"(need %d)" % _need(entry.split("/")[0], a) in msg, msg


@pytest.mark.parametrize("entry,first,later", [(e, f, g) for e in ALL for i, f in enumerate(RANK) for g in RANK[i + 1:]
                                               if e in FAULTS[f][0] and e in FAULTS[g][0]])
def test_the_earlier_ranked_fault_wins(entry, first, later):
    """Two faults in one call: the message is the earlier one's."""
    assert not set(FAULTS[first][1]) & set(FAULTS[later][1])
    msg = _refused(entry, _args(entry, **dict(FAULTS[first][1], **FAULTS[later][1])), FAULTS[first][2])
    assert FAULTS[later][2] not in msg, msg


@pytest.mark.parametrize("entry", ALL)
def test_a_call_without_fault_reaches_the_null_pointers(entry):
    """x is NULL in every row above, so a row whose refusal went missing would have ended here and not in a launch."""
    _refused(entry, _args(entry), b"null pointer")
    _refused(entry, _args(entry, x=UNREAD, y=NULL), b"null pointer")
    _refused(entry, _args(entry, x=UNREAD, v=NULL), b"null pointer")
    _refused(entry, _args(entry, short=1), b"null pointer")                 # more scratch than needed is no fault
    if entry == "block_fused":
        _refused(entry, _args(entry, panels=NULL, panel_elems=0), b"null pointer")         # the exact-f32 form needs no panels
    if entry == "expand_dw":
        _refused(entry, _args(entry, stride=2), b"null pointer")
    if entry.startswith("expand_dw_stream/"):                               # the exact-f32 form (Cin <= 32): no panels; rate -2 = stride 2
        for rate in (1, 2, -2):
            _refused(entry, _args(entry, Cin=16, Cexp=96, rate=rate, panels=NULL, panel_elems=0), b"null pointer")
    if entry.startswith("expand_dw_stream") or entry == "dw_project":
        _refused(entry, _args(entry, rate=2), b"null pointer")
    if entry.startswith("expand_dw_stream_f16"):
        _refused(entry, _args(entry, y_h2i=1), b"null pointer")
    if entry == "dw_project":
        _refused(entry, _args(entry, res=UNREAD), b"null pointer")
