"""What the kernel-level entries of the GEMM family (ams_k_pointwise, _split, _split3, _split_f16, _wgrad, _wgrad_split, _red, _xform,
_wgrad_xform, ams_k_pack_h2i), of the depthwise and stem family (ams_k_depthwise3x3, _dgrad, _wgrad, _fwd_bn, _dgrad_bn, _fwd_bn_tiles,
_dgrad_bn_apply, ams_k_stem_conv) and of the recompute family (ams_k_xdw_fwd_stats, _bwd_reduce, _bwd_dx, _bwd_reduce_stem, _dwe, ams_k_xx_gram,
ams_k_expand_stats) refuse, in which order, with which return code and which word in ams_last_error(): one table over the refusable arguments.
The order is entry_check's (ams_amd/csrc/entry_check.hpp): no pixels or rows; the entry's shape rule; scratch or panels NULL or too small
("need N"); scale without shift; a null pointer.  The *_scratch() functions answer 0 for what their entry refuses at the first two steps.

No row reaches a device call.  Every row of the table passes a NULL input tensor, which each entry refuses ("null pointer") in front of its
first launch, the weight splits included, so even a row whose expected refusal went missing would end in AMS_E_INVALID and not in a kernel on
made-up addresses.  The other pointers are either NULL or an address nobody reads: the checks only compare them against NULL."""
import ctypes as C

import pytest

from ams_amd import hip
from kernel_suite import dw_wgrad_scratch, wgrad_f32_scratch, wgrad_x6_scratch

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1
DT_U8, DT_F32 = hip.DT_U8, hip.DT_F32


def _same(n, stride):
    return -(-n // stride)


def _kp(K):
    return (K + 31) // 32 * 32


# entry -> (the smallest call it accepts, its scratch in elements or None)
GEMM = dict(M=17, K=32, N=4)
WG6 = dict(M=1024, K=64, N=64)
DW = dict(B=1, H=2, W=3, C=4, stride=1, rate=1)
DWBN = dict(B=1, H=2, W=3, C=4, rate=1)           # the one-kernel fine-tune forms: stride 1
XDW = dict(B=1, H=2, W=3, Cin=8, Cexp=32, stride=1)
BASE = {
    "pointwise": GEMM, "pointwise_split": GEMM, "pointwise_split3": GEMM, "pointwise_split_f16": GEMM, "pack_h2i": dict(M=3, K=8),
    "pointwise_wgrad": GEMM, "pointwise_wgrad_split": WG6,
    "pointwise_red/0": dict(GEMM, mode=1), "pointwise_red/1": dict(GEMM, mode=2), "pointwise_red/2": dict(GEMM, mode=1),
    "pointwise_xform/0": dict(GEMM, mode=1), "pointwise_xform/1": dict(GEMM, mode=2), "pointwise_xform/2": dict(GEMM, mode=1),
    "pointwise_wgrad_xform/0": dict(GEMM, mode=1), "pointwise_wgrad_xform/1": dict(WG6, mode=1),
    "depthwise3x3": DW, "depthwise3x3_dgrad": DW, "depthwise3x3_wgrad": DW,
    "depthwise3x3_fwd_bn": DWBN, "depthwise3x3_dgrad_bn": DWBN, "depthwise3x3_fwd_bn_tiles": DWBN, "depthwise3x3_dgrad_bn_apply": DWBN,
    "stem_conv": dict(B=1, H=2, W=3, cout=8, dtype=DT_U8),
    "xdw_fwd_stats": XDW, "xdw_bwd_reduce": XDW, "xdw_bwd_dx": XDW, "xdw_bwd_reduce_stem": dict(B=1, H=2, W=3, dtype=DT_U8),
    "xdw_dwe": dict(Cin=27, Cexp=32), "xx_gram": dict(M=5, Cin=4), "expand_stats": dict(Cin=4, Cexp=8, n=5.0),
}
ALL = tuple(BASE)


def _split(entry):
    return int(entry.split("/")[1]) if "/" in entry else 0


def _need(entry, a):
    """the scratch (floats, doubles) or panels (uint16) the header asks for; None: the entry has none"""
    lib, name = hip.lib(), entry.split("/")[0]
    if name in ("pointwise_split", "pointwise_split_f16"):
        return 2 * a["N"] * _kp(a["K"])
    if name == "pointwise_split3":
        return 3 * a["N"] * _kp(a["K"])
    if name in ("pointwise_red", "pointwise_xform"):
        return {0: None, 1: 3 * a["N"] * _kp(a["K"]), 2: 2 * a["N"] * _kp(a["K"])}[_split(entry)]
    if name == "pointwise_wgrad" or entry == "pointwise_wgrad_xform/0":
        return wgrad_f32_scratch(a["M"], a["K"], a["N"])
    if name in ("pointwise_wgrad_split", "pointwise_wgrad_xform"):
        return wgrad_x6_scratch(a["M"], a["K"], a["N"])
    if name == "depthwise3x3_wgrad":
        return dw_wgrad_scratch(a["B"], _same(a["H"], a["stride"]), _same(a["W"], a["stride"]), a["C"])
    size = (a.get("B"), a.get("H"), a.get("W"))
    if name == "depthwise3x3_fwd_bn":
        return lib.ams_k_depthwise3x3_fwd_bn_scratch(*size, a["C"], a["rate"])
    if name == "depthwise3x3_dgrad_bn":
        return lib.ams_k_depthwise3x3_dgrad_bn_scratch(*size, a["C"])
    if name == "depthwise3x3_fwd_bn_tiles":
        return lib.ams_k_depthwise3x3_fwd_bn_tiles_scratch(*size, a["C"], a["rate"])
    if name == "depthwise3x3_dgrad_bn_apply":
        return lib.ams_k_depthwise3x3_dgrad_bn_apply_scratch(*size, a["C"], a["rate"])
    if name in ("xdw_fwd_stats", "xdw_bwd_reduce"):
        return lib.ams_k_xdw_train_scratch(*size, a["Cin"], a["Cexp"])
    if name == "xdw_bwd_reduce_stem":
        return lib.ams_k_xdw_stem_scratch(*size)
    if name == "xx_gram":
        return lib.ams_k_xx_gram_scratch(a["M"], a["Cin"])
    return None


SCRATCH = tuple(e for e in ALL if e.split("/")[0] in (
    "pointwise_split", "pointwise_split3", "pointwise_split_f16", "pointwise_wgrad", "pointwise_wgrad_split", "pointwise_wgrad_xform",
    "depthwise3x3_wgrad", "depthwise3x3_fwd_bn", "depthwise3x3_dgrad_bn", "depthwise3x3_fwd_bn_tiles", "depthwise3x3_dgrad_bn_apply",
    "xdw_fwd_stats", "xdw_bwd_reduce", "xdw_bwd_reduce_stem", "xx_gram") or e in ("pointwise_red/1", "pointwise_red/2", "pointwise_xform/1",
                                                                                  "pointwise_xform/2"))
SCALED = ("pointwise", "pointwise_split", "pointwise_split3", "pointwise_split_f16", "depthwise3x3", "stem_conv")        # scale, shift optional


def _args(entry, **over):
    a = dict(x=NULL, p=UNREAD, y=UNREAD, scr=UNREAD, elems=None, scale=NULL, shift=NULL, y_parts=NULL)
    a.update(BASE[entry])
    a.update(over)
    short = a.pop("short", 0)
    if a["elems"] is None:
        try:
            need = _need(entry, a)
        except ZeroDivisionError:            # the formula on a size the entry refuses first (C = 0 ...)
            need = 0
        a["elems"] = max(0, (need or 0) + short)
    return a


def _call(entry, a):
    lib, name, split = hip.lib(), entry.split("/")[0], _split(entry)
    x, p, y, scr, n = a["x"], a["p"], a["y"], a["scr"], a["elems"]
    rows, stride_out = C.byref(C.c_int32(0)), C.byref(C.c_int64(0))
    if name == "pointwise":
        return lib.ams_k_pointwise(x, a["M"], a["K"], p, a["N"], 0, NULL, 1, a["scale"], a["shift"], 0, NULL, y, NULL)
    if name in ("pointwise_split", "pointwise_split3"):
        return getattr(lib, "ams_k_" + name)(x, a["M"], a["K"], p, a["N"], a["scale"], a["shift"], 0, NULL, y, scr, n, NULL)
    if name == "pointwise_split_f16":
        return lib.ams_k_pointwise_split_f16(x, a["M"], a["K"], p, a["N"], a["scale"], a["shift"], 0, NULL, y, scr, n, NULL, a["y_parts"], NULL)
    if name == "pack_h2i":
        return lib.ams_k_pack_h2i(x, a["M"], a["K"], y, NULL)
    if name in ("pointwise_wgrad", "pointwise_wgrad_split"):
        return getattr(lib, "ams_k_" + name)(x, p, a["M"], a["K"], a["N"], y, scr, n, NULL)
    if name == "pointwise_red":
        return lib.ams_k_pointwise_red(x, a["M"], a["K"], p, a["N"], 0, split, a["mode"], NULL, p, p, p, p, p, 0, NULL, y, p, 1 << 20, rows, scr, n, NULL)
    if name == "pointwise_xform":
        return lib.ams_k_pointwise_xform(x, a["M"], a["K"], p, a["N"], 0, split, a["mode"], 0, p, p, p, p, y, NULL, scr, n, NULL)
    if name == "pointwise_wgrad_xform":
        return lib.ams_k_pointwise_wgrad_xform(x, p, a["M"], a["K"], a["N"], split, a["mode"], 0, p, p, 0, NULL, NULL, NULL, NULL, y, scr, n, NULL)
    size = (a.get("B"), a.get("H"), a.get("W"))
    if name == "depthwise3x3":
        return lib.ams_k_depthwise3x3(x, *size, a["C"], p, a["stride"], a["rate"], a["scale"], a["shift"], 0, y, NULL)
    if name == "depthwise3x3_dgrad":
        return lib.ams_k_depthwise3x3_dgrad(x, *size, a["C"], p, a["stride"], a["rate"], y, NULL)
    if name == "depthwise3x3_wgrad":
        return lib.ams_k_depthwise3x3_wgrad(x, p, *size, a["C"], a["stride"], a["rate"], y, scr, n, NULL)
    if name in ("depthwise3x3_fwd_bn", "depthwise3x3_fwd_bn_tiles"):
        return getattr(lib, "ams_k_" + name)(x, *size, a["C"], p, a["rate"], p, p, 0, NULL, y, scr, n, rows, NULL)
    if name == "depthwise3x3_dgrad_bn":
        return lib.ams_k_depthwise3x3_dgrad_bn(x, *size, a["C"], p, a["rate"], p, p, p, 0, p, p, y, scr, n, rows, NULL)
    if name == "depthwise3x3_dgrad_bn_apply":
        return lib.ams_k_depthwise3x3_dgrad_bn_apply(x, p, p, p, p, *size, a["C"], p, a["rate"], p, p, p, 0, p, p, y, scr, n, rows, NULL)
    if name == "stem_conv":
        return lib.ams_k_stem_conv(x, a["dtype"], *size, p, a["cout"], a["scale"], a["shift"], 0, 1.0 / 127.5, y, NULL)
    if name == "xdw_fwd_stats":
        return lib.ams_k_xdw_fwd_stats(x, *size, a["Cin"], p, a["Cexp"], NULL, scr, n, rows, stride_out, NULL)
    if name == "xdw_bwd_reduce":
        return lib.ams_k_xdw_bwd_reduce(x, *size, a["Cin"], p, a["Cexp"], p, p, p, p, 0, p, a["stride"], p, scr, n, rows, stride_out, NULL)
    if name == "xdw_bwd_dx":
        return lib.ams_k_xdw_bwd_dx(x, *size, a["Cin"], p, a["Cexp"], p, p, 0, p, a["stride"], p, p, p, p, NULL, y, NULL)
    if name == "xdw_bwd_reduce_stem":
        return lib.ams_k_xdw_bwd_reduce_stem(x, a["dtype"], *size, 1.0 / 127.5, p, p, p, p, p, 0, p, p, scr, n, rows, stride_out, NULL)
    if name == "xdw_dwe":
        return lib.ams_k_xdw_dwe(x, p, a["Cin"], a["Cexp"], p, p, p, p, y, NULL)
    if name == "xx_gram":
        return lib.ams_k_xx_gram(x, a["M"], a["Cin"], scr, n, y, NULL, NULL)
    assert name == "expand_stats"
    return lib.ams_k_expand_stats(x, a["Cin"], p, a["Cexp"], a["n"], NULL, p, p, 1e-3, 0.1, NULL, NULL, y, y, NULL, NULL, NULL, NULL)


def _with(*keys):
    return tuple(e for e in ALL if all(k in BASE[e] for k in keys))


IMAGES, ROWS, DEPTHWISE, XDWS = _with("B"), _with("M"), _with("C"), _with("Cin", "B")
STRIDED = _with("stride", "C")                     # depthwise3x3, _dgrad, _wgrad
PARTS = tuple(e for e in ALL if e.split("/")[0] in ("pointwise_split", "pointwise_split3") or e in ("pointwise_red/1", "pointwise_xform/1"))
F16 = ("pointwise_split_f16", "pointwise_red/2", "pointwise_xform/2")
# a fault per refusable argument, in the order of refusal: name -> (entries that can be given it, overrides, the word in the message)
# ("short": the scratch that many elements off what the call needs)
FAULTS = {
    "size": (IMAGES + ROWS + ("xdw_dwe", "expand_stats"), dict(H=0, M=0, Cexp=0), b"empty problem"),
    "shape": (DEPTHWISE + ("stem_conv", "xdw_bwd_reduce_stem") + XDWS + PARTS + ("pointwise", "pointwise_wgrad_split", "pointwise_wgrad_xform/1",
                                                                                   "pack_h2i", "xdw_dwe", "xx_gram", "expand_stats") + F16,
              dict(rate=3, C=6, dtype=7, Cin=36, K=6), b"unsupported shape"),
    "scratch": (SCRATCH, dict(short=-1), b"too small (need "),
    "scale": (SCALED, dict(scale=UNREAD), b"scale without shift"),
}
FAULTS["shape"] = (tuple(e for e in FAULTS["shape"][0] if e not in ("pointwise_wgrad_split", "pointwise_wgrad_xform/1")), ) + FAULTS["shape"][1:]
RANK = list(FAULTS)
WG6S = ("pointwise_wgrad_split", "pointwise_wgrad_xform/1")
# further values of a single fault: (fault, entries, overrides)
MORE = [("size", IMAGES, dict(B=0)), ("size", IMAGES, dict(W=0)), ("size", IMAGES, dict(B=-1)), ("size", IMAGES, dict(H=-3)), ("size", IMAGES, dict(W=-5)),
        ("size", ROWS, dict(M=-1)), ("size", _with("K"), dict(K=0)), ("size", _with("K"), dict(K=-8)), ("size", _with("N"), dict(N=0)),
        ("size", _with("N"), dict(N=-4)), ("size", DEPTHWISE, dict(C=0)), ("size", DEPTHWISE, dict(C=-4)), ("size", ("stem_conv",), dict(cout=0)),
        ("size", ("stem_conv",), dict(cout=-8)), ("size", _with("Cin"), dict(Cin=0)), ("size", _with("Cin"), dict(Cin=-4)),
        ("size", _with("Cexp"), dict(Cexp=-16)), ("size", ("expand_stats",), dict(n=0.0)),
        ("shape", DEPTHWISE, dict(C=2)), ("shape", DEPTHWISE, dict(C=1028)), ("shape", STRIDED, dict(stride=3)), ("shape", DEPTHWISE, dict(rate=3)),
        ("shape", STRIDED, dict(stride=2, rate=2)), ("shape", DEPTHWISE, dict(rate=0)), ("shape", STRIDED, dict(stride=0)),
        ("shape", ("stem_conv",), dict(cout=12)), ("shape", ("stem_conv",), dict(cout=264)), ("shape", ("stem_conv", "xdw_bwd_reduce_stem"), dict(dtype=2)),
        ("shape", XDWS, dict(Cin=4)), ("shape", XDWS, dict(Cin=36)), ("shape", XDWS, dict(Cin=10)), ("shape", XDWS + ("xdw_dwe",), dict(Cexp=16)),
        ("shape", XDWS + ("xdw_dwe",), dict(Cexp=208)), ("shape", XDWS + ("xdw_dwe",), dict(Cexp=40)), ("shape", ("xdw_bwd_reduce", "xdw_bwd_dx"), dict(stride=3)),
        ("shape", ("xdw_dwe",), dict(Cin=33)), ("shape", ("xx_gram", "expand_stats"), dict(Cin=3)), ("shape", ("xx_gram", "expand_stats"), dict(Cin=33)),
        ("shape", PARTS + F16, dict(K=6)), ("shape", PARTS + F16, dict(K=12)), ("shape", F16, dict(K=24)), ("shape", ("pointwise",), dict(K=6)),
        ("shape", ("pointwise_red/0", "pointwise_xform/0"), dict(K=6)), ("shape", ("pack_h2i",), dict(K=12)),
        ("shape", ("pointwise_split_f16",), dict(N=3, y_parts=UNREAD)),                      # part planes come from a vector epilogue only
        ("shape", WG6S, dict(M=1023)), ("shape", WG6S, dict(M=32769)), ("shape", WG6S, dict(K=6)), ("shape", WG6S, dict(K=32)),
        ("shape", tuple(e for e in ALL if e.startswith("pointwise_red") or e.startswith("pointwise_xform")), dict(mode=3)),
        ("scratch", SCRATCH, dict(scr=NULL)), ("scratch", SCRATCH, dict(elems=0))]

SINGLE = [(e, f, FAULTS[f][1], FAULTS[f][2]) for f in RANK for e in FAULTS[f][0]] + [(e, f, o, FAULTS[f][2]) for f, es, o in MORE for e in es]


def _id(v):
    if isinstance(v, bytes):
        return v.decode()
    return v if isinstance(v, str) else ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else "ptr" if v[k] is UNREAD else v[k]) for k in v)


def _refused(entry, a, word):
    assert a["x"] is NULL                          # whatever else the row says, its input tensor is NULL
    assert _call(entry, a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("entry,fault,over,word", SINGLE, ids=_id)
def test_each_fault_is_refused_in_words(entry, fault, over, word):
    a = _args(entry, **over)
    msg = _refused(entry, a, word)
    assert msg.startswith(entry.split("/")[0].encode() + b":"), msg          # the called entry's name
    if fault == "scratch":
        assert b"(need %d)" % _need(entry, a) in msg, msg


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
    if entry in SCRATCH:
        _refused(entry, _args(entry, short=1), b"null pointer")             # more scratch than needed is no fault
    if entry in SCALED:
        _refused(entry, _args(entry, scale=UNREAD, shift=UNREAD), b"null pointer")
    if entry in STRIDED:
        for stride, rate in ((2, 1), (1, 2)):
            _refused(entry, _args(entry, stride=stride, rate=rate), b"null pointer")
    if entry in DEPTHWISE:
        _refused(entry, _args(entry, C=1024, rate=2 if "stride" not in BASE[entry] else 1), b"null pointer")
    if entry == "stem_conv":
        for cout in (32, 256):
            _refused(entry, _args(entry, cout=cout, dtype=DT_F32), b"null pointer")
    if entry in XDWS:
        _refused(entry, _args(entry, Cin=32, Cexp=192, stride=2 if entry != "xdw_fwd_stats" else 1), b"null pointer")


NO_RESULT = ("xdw_fwd_stats", "xdw_bwd_reduce", "xdw_bwd_reduce_stem")          # their results are the scratch rows
NO_WEIGHTS = ("pack_h2i", "xx_gram")                                             # they read x and nothing else


@pytest.mark.parametrize("entry", ALL)
def test_every_other_null_pointer_is_refused_too(entry):
    """With an input that looks real, the result NULL, or the weights and vectors NULL: still "null pointer", still in front of the launch.
    (Each call here keeps one pointer NULL that its entry reads or writes: y where it has a result, p where it has weights.)"""
    for over in ([] if entry in NO_RESULT else [dict(y=NULL)]) + ([] if entry in NO_WEIGHTS else [dict(p=NULL)]):
        a = _args(entry, **over)
        a["x"] = UNREAD
        assert _call(entry, a) == E_INVALID and b"null pointer" in hip.lib().ams_last_error(), hip.lib().ams_last_error()


def test_scratch_functions_answer_zero_for_what_their_entry_refuses():
    """Sizes <= 0 and refused shapes: 0, without dividing by a channel count of zero or wrapping; an accepted call: the formula."""
    lib = hip.lib()
    five = (lib.ams_k_depthwise3x3_fwd_bn_scratch, lib.ams_k_depthwise3x3_fwd_bn_tiles_scratch, lib.ams_k_depthwise3x3_dgrad_bn_apply_scratch)
    for B, H, W, Cn in ((0, 2, 3, 4), (1, 0, 3, 4), (1, 2, -3, 4), (1, 2, 3, 0), (1, 2, 3, -4), (1, 2, 3, 2), (1, 2, 3, 6), (1, 2, 3, 1028)):
        for f in five:
            assert f(B, H, W, Cn, 1) == 0, (f.__name__, B, H, W, Cn)
        assert lib.ams_k_depthwise3x3_dgrad_bn_scratch(B, H, W, Cn) == 0
    for f in five:
        assert f(1, 2, 3, 4, 3) == 0 and f(1, 2, 3, 4, 0) == 0 and f(1, 2, 3, 4, 1) > 0 and f(1, 2, 3, 1024, 2) > 0
    assert lib.ams_k_depthwise3x3_dgrad_bn_scratch(1, 2, 3, 4) == 11 * 4
    for M, K, N in ((0, 32, 4), (-1, 32, 4), (17, 0, 4), (17, 32, 0), (17, -32, -4)):
        assert lib.ams_k_pointwise_wgrad_scratch(M, K, N) == 0
    assert lib.ams_k_pointwise_wgrad_scratch(17, 32, 4) == max(wgrad_f32_scratch(17, 32, 4), wgrad_x6_scratch(17, 32, 4))
    for B, H, W, Cin, Cexp in ((0, 2, 3, 8, 32), (1, -2, 3, 8, 32), (1, 2, 0, 8, 32), (1, 2, 3, 4, 32), (1, 2, 3, 36, 32), (1, 2, 3, 8, 16),
                               (1, 2, 3, 8, 208), (1, 2, 3, 0, 32), (1, 2, 3, 8, 0), (1, 1 << 15, 1 << 15, 8, 32)):
        assert lib.ams_k_xdw_train_scratch(B, H, W, Cin, Cexp) == 0, (B, H, W, Cin, Cexp)
    assert lib.ams_k_xdw_train_scratch(1, 2, 3, 8, 32) > 0
    for B, H, W in ((0, 2, 3), (1, 0, 3), (1, 2, -1), (1, 1 << 15, 1 << 15)):
        assert lib.ams_k_xdw_stem_scratch(B, H, W) == 0
    assert lib.ams_k_xdw_stem_scratch(1, 2, 3) > 0
    for M, Cin in ((0, 8), (-5, 8), (5, 0), (5, 3), (5, 33), (5, -4)):
        assert lib.ams_k_xx_gram_scratch(M, Cin) == 0
    assert lib.ams_k_xx_gram_scratch(5, 4) == 2 * (16 * 16 + 16)
