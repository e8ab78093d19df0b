"""What the five kernel-level loss entry points (ams_k_ce_loss_grad, _soft, _soft_layout, _kd, _weighted) refuse, in which order, with which
return code and which word in ams_last_error(): one table over the refusable arguments.  The order is: KD parameters; the weights, before
any pointer is looked at; null teacher logits; the class table; K; the layout; the row stride; the geometry; the scratch.

No row reaches a device call.  Every call here passes NULL student logits, labels and loss, which the launcher refuses ("null pointer") in
front of its first launch, so even a row whose expected refusal went missing would end in AMS_E_INVALID and not in a kernel on made-up
addresses.  The teacher logits and the scratch, which the entries only compare against NULL, are addresses nobody reads."""
import ctypes as C

import pytest

from ams_amd import hip

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1
CI = [0, 1, 2, 10, 11, 13]


def _floats(values):
    return (C.c_float * len(values))(*values) if values is not None else None


def _args(**over):
    a = dict(B=2, h=5, w=9, ld=19, NC=19, cls=CI, K=6, H=64, W=128, tl=UNREAD, th=64, tw=128, layout=hip.TLOGITS_FULL, scratch=UNREAD, short=0,
             T=2.0, alpha=0.5, cw=None, gamma=0.0)
    a.update(over)
    return a


def _call(entry, a):
    """The entry point on the arguments of `a`; scratch_floats is what ams_k_ce_loss_grad_scratch asks for the shape, less a["short"]."""
    lib = hip.lib()
    ci = (C.c_int32 * len(a["cls"]))(*a["cls"]) if a["cls"] is not None else None
    n = lib.ams_k_ce_loss_grad_scratch(a["B"], a["h"], a["w"], a["K"]) - a["short"]
    head = (a["B"], a["h"], a["w"])
    tail = (NULL, NULL, a["scratch"], n, NULL)                       # loss, dlogits, scratch, scratch_floats, stream
    labels = (ci, a["K"], a["H"], a["W"], NULL)
    soft = (a["tl"], a["th"], a["tw"])
    kd = (C.c_float(a["T"]), C.c_float(a["alpha"]))
    if entry == "hard":
        return lib.ams_k_ce_loss_grad(NULL, *head, a["NC"], *labels, *tail)
    if entry == "soft":
        return lib.ams_k_ce_loss_grad_soft(NULL, *head, a["NC"], *labels, *soft, *tail)
    if entry == "soft_layout":
        return lib.ams_k_ce_loss_grad_soft_layout(NULL, *head, a["ld"], a["NC"], *labels, *soft, a["layout"], *tail)
    if entry == "kd":
        return lib.ams_k_ce_loss_grad_kd(NULL, *head, a["ld"], a["NC"], *labels, *soft, a["layout"], *tail, *kd)
    assert entry == "weighted"
    return lib.ams_k_ce_loss_grad_weighted(NULL, *head, a["ld"], a["NC"], *labels, *soft, a["layout"], *tail, *kd, _floats(a["cw"]), C.c_float(a["gamma"]))


ALL = ("hard", "soft", "soft_layout", "kd", "weighted")
SOFT = ("soft", "soft_layout", "kd", "weighted")
LAYOUT = ("soft_layout", "kd", "weighted")
NAN, INF = float("nan"), float("inf")
BAD_CW = [1.0, NAN, 1.0, 1.0, 1.0, 1.0]

# a fault per refusable argument: (name, entries that take the argument, overrides, the word in the message)
FAULTS = {
    "temperature": (("kd", "weighted"), dict(T=0.0), b"temperature"),
    "alpha": (("kd", "weighted"), dict(alpha=1.5), b"alpha"),
    "gamma": (("weighted",), dict(gamma=9.0), b"conf_gamma"),
    "weight": (("weighted",), dict(cw=BAD_CW), b"class_weights[1]"),
    "teacher_logits": (SOFT, dict(tl=NULL), b"null teacher logits"),
    "class_table": (ALL, dict(cls=None), b"null class table"),
    "K": (ALL, dict(K=33), b"out of range"),
    "layout": (LAYOUT, dict(layout=7), b"teacher-logit layout"),
    "stride": (LAYOUT, dict(ld=18), b"row stride"),
    "geometry": (ALL, dict(w=2), b"one-pass"),
    "scratch": (ALL, dict(short=1), b"scratch too small"),
}
RANK = list(FAULTS)

# further values of a single fault: (fault, overrides)
MORE = [("temperature", dict(T=-1.0)), ("temperature", dict(T=NAN)), ("temperature", dict(T=INF)), ("temperature", dict(T=1e-39)),
        ("alpha", dict(alpha=-0.1)), ("alpha", dict(alpha=NAN)),
        ("gamma", dict(gamma=-0.5)), ("gamma", dict(gamma=NAN)), ("gamma", dict(gamma=INF)),
        ("weight", dict(cw=[1.0, 17.0, 1.0, 1.0, 1.0, 1.0])), ("weight", dict(cw=[1.0, 0.001, 1.0, 1.0, 1.0, 1.0])),
        ("teacher_logits", dict(tl=NULL, alpha=0.0, gamma=2.0)),         # the weighted entry: alpha = 0 alone does not excuse them
        ("K", dict(K=0)), ("layout", dict(layout=-1)), ("stride", dict(ld=257)), ("scratch", dict(scratch=NULL))]

SINGLE = [(e, f, FAULTS[f][1]) for f in RANK for e in FAULTS[f][0]] + [(e, f, o) for f, o in MORE for e in FAULTS[f][0]]


def _id(v):
    return v if isinstance(v, str) else ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else v[k]) for k in v)


def _refused(entry, a, word):
    assert _call(entry, a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("entry,fault,over", SINGLE, ids=_id)
def test_each_fault_is_refused_in_words(entry, fault, over):
    _refused(entry, _args(**over), FAULTS[fault][2])


def _pairs():
    out = []
    for entry in ALL:
        mine = [f for f in RANK if entry in FAULTS[f][0]]
        out += [(entry, first, later) for i, first in enumerate(mine) for later in mine[i + 1:]]
    return out


@pytest.mark.parametrize("entry,first,later", _pairs())
def test_the_earlier_ranked_fault_wins(entry, first, later):
    """Two faults in one call: the message is the earlier one's.  (The null-teacher-logits message quotes alpha and conf_gamma, so a later fault's
    word is looked for only where the earlier message cannot hold it.)"""
    over = dict(FAULTS[first][1], **FAULTS[later][1])
    # a weight table beside K = 33: the weights' own count check speaks (it reads no weight)
    msg = _refused(entry, _args(**over), b"class weights" if (first, later) == ("weight", "K") else FAULTS[first][2])
    if first != "teacher_logits":
        assert FAULTS[later][2] not in msg, msg


def test_the_weighted_entry_without_teacher_logits_reaches_the_launcher():
    """alpha = 0 and gamma = 0 need no teacher logits: every check of the entry passes, and the launcher refuses the NULL labels and loss."""
    msg = _refused("weighted", _args(tl=NULL, alpha=0.0, cw=[1.0, 0.0, 2.0, 1.0, 1.0, 16.0]), b"null pointer")
    assert b"teacher logits" not in msg


@pytest.mark.parametrize("entry", ALL)
def test_a_call_without_fault_reaches_the_launcher(entry):
    _refused(entry, _args(), b"null pointer")
