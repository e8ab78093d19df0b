"""What the five kernel-level head entry points (ams_k_upsample_argmax, _confidence, _soft_metric, _soft_metric_layout, ams_k_ce_grad) refuse,
in which order, with which return code and which word in ams_last_error(): one table over the refusable arguments.  The order is the one
check every head launcher goes through (head_call_check: the class table; K; a class id; an empty size; the row stride), then the launcher's
own conditions (the teacher-logit layout; the teacher grid; metrics without buffers; ldd; the band limits), then its null pointers.

No row reaches a device call.  Every call here passes NULL student logits, which each launcher refuses ("null pointer") in front of its first
memset or launch, so even a row whose expected refusal went missing would end in AMS_E_INVALID and not in a kernel on made-up addresses.
The other pointers are either NULL or an address nobody reads: the checks only compare them against NULL.  Nothing is allocated for the
band-limit rows either, whatever their sizes say."""
import ctypes as C

import pytest

from ams_amd import hip

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1
CI = [0, 1, 2, 10, 11, 13]


def _args(**over):
    a = dict(B=2, h=5, w=9, ld=19, NC=19, cls=CI, K=6, H=64, W=128, teacher=NULL, conf=NULL, loss=NULL, tl=UNREAD, th=64, tw=128,
             layout=hip.TLOGITS_FULL)
    a.update(over)
    return a


def _call(entry, a):
    lib = hip.lib()
    ci = (C.c_int32 * len(a["cls"]))(*a["cls"]) if a["cls"] is not None else None
    head = (a["B"], a["h"], a["w"])
    labels = (ci, a["K"], a["H"], a["W"], a["teacher"])
    soft = (a["tl"], a["th"], a["tw"])
    if entry == "argmax":
        return lib.ams_k_upsample_argmax(NULL, *head, a["NC"], *labels, NULL, a["conf"], a["loss"], NULL)
    if entry == "confidence":
        return lib.ams_k_upsample_confidence(NULL, *head, a["NC"], *labels, NULL, NULL, NULL, NULL)
    if entry == "soft_metric":
        return lib.ams_k_upsample_soft_metric(NULL, *head, a["NC"], *labels, *soft, NULL, NULL, NULL, NULL)
    if entry == "soft_metric_layout":
        return lib.ams_k_upsample_soft_metric_layout(NULL, *head, a["ld"], a["NC"], *labels, *soft, a["layout"], NULL, NULL, NULL, NULL)
    assert entry == "ce_grad"
    return lib.ams_k_ce_grad(NULL, *head, a["NC"], *labels, NULL, NULL, NULL)


ALL = ("argmax", "confidence", "soft_metric", "soft_metric_layout", "ce_grad")
SOFT = ("soft_metric", "soft_metric_layout")
# one row per band with W = 1 and B = 1: 2048 bands (head_band_grid), so H above 2047 x 2048 rows is 2048 rows per band, above 8191 x 2048 is 8192
TALL_SOFT = dict(B=1, W=1, tw=1, H=2047 * 2048 + 1)
TALL_CONF = dict(B=1, W=1, H=8191 * 2048 + 1)

# a fault per refusable argument, in the order of refusal: name -> (entries that can be given it, overrides, the word in the message)
FAULTS = {
    "class_table": (ALL, dict(cls=None), b"null class table"),
    "K": (ALL, dict(K=33), b"K=33 out of range"),
    "class_id": (ALL, dict(cls=[0, 1, -1, 10, 11, 13]), b"class id -1"),
    "size": (ALL, dict(h=0), b"no pixels"),
    "stride": (("soft_metric_layout",), dict(ld=18), b"row stride"),
    "layout": (("soft_metric_layout",), dict(layout=7), b"teacher-logit layout"),
    "grid": (SOFT, dict(th=0), b"teacher logits of"),
    "metrics": (("argmax",), dict(teacher=UNREAD), b"metrics need"),
    "ldd": (("ce_grad",), dict(NC=300), b"ldd=300"),
    "band_soft": (SOFT, TALL_SOFT, b"rows per band"),
    "band_confidence": (("confidence",), TALL_CONF, b"rows per band"),
}
RANK = list(FAULTS)

# further values of a single fault: (fault, overrides, the word where it differs)
MORE = [("K", dict(K=0), b"K=0 out of range"), ("class_id", dict(cls=[0, 1, 2, 10, 11, 19]), b"class id 19"),
        ("class_id", dict(NC=300, ld=300, cls=[0, 1, 2, 10, 11, 256]), b"class id 256"),         # an id the 256-entry table cannot hold
        ("size", dict(B=0), None), ("size", dict(W=0), None), ("size", dict(w=-1), None), ("size", dict(H=0), None),
        ("stride", dict(ld=0), None), ("stride", dict(ld=-32), None), ("layout", dict(layout=-1), None), ("grid", dict(th=65), None), ("grid", dict(tw=0), None), ("grid", dict(tw=129), None),
        ("metrics", dict(teacher=UNREAD, conf=UNREAD), None), ("metrics", dict(teacher=UNREAD, loss=UNREAD), None),
        ("ldd", dict(NC=257), b"ldd=257"),
        ("band_soft", dict(TALL_SOFT, H=2 ** 30), None), ("band_confidence", dict(TALL_CONF, H=2 ** 30), None)]

SINGLE = [(e, f, FAULTS[f][1], FAULTS[f][2]) for f in RANK for e in FAULTS[f][0]] + \
         [(e, f, o, word or FAULTS[f][2]) for f, o, word in MORE for e in FAULTS[f][0]]


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
    _refused(entry, _args(**over), word)


def _pairs():
    out = []
    for entry in ALL:
        mine = [f for f in RANK if entry in FAULTS[f][0]]
        out += [(entry, first, later) for i, first in enumerate(mine) for later in mine[i + 1:]]
    # the null class table and the bad class id are values of ONE argument: no call holds both
    return [t for t in out if t[1:] != ("class_table", "class_id")]


@pytest.mark.parametrize("entry,first,later", _pairs())
def test_the_earlier_ranked_fault_wins(entry, first, later):
    """Two faults in one call: the message is the earlier one's."""
    assert not set(FAULTS[first][1]) & set(FAULTS[later][1])
    msg = _refused(entry, _args(**dict(FAULTS[first][1], **FAULTS[later][1])), FAULTS[first][2])
    assert FAULTS[later][2] not in msg, msg


@pytest.mark.parametrize("entry", ALL)
def test_a_call_without_fault_reaches_the_null_pointers(entry):
    _refused(entry, _args(), b"null pointer")
    # the tallest bands that pass
    if entry in SOFT:
        _refused(entry, _args(**dict(TALL_SOFT, H=2047 * 2048)), b"null pointer")
    if entry == "confidence":
        _refused(entry, _args(**dict(TALL_CONF, H=8191 * 2048)), b"null pointer")
