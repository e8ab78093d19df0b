"""What ams_student_encode_delta_q8 and ams_student_apply_delta_q8 refuse on the host, in which order, with AMS_E_INVALID and which word in
ams_last_error(): one table over the refusable arguments.  The order is: null pointers; advance_base; the table's shape; the statistics' base;
the scratch; the room for the payload; and last the handle.

No row reaches a launch.  Every call here passes a NULL handle, which both entries refuse ("null handle") behind every other check of this
table and in front of the first thing they do with it, so even a row whose expected refusal went missing would end in AMS_E_INVALID and
not in a kernel on made-up addresses.  The device pointers, which the entries only compare against NULL, are addresses nobody reads.  (What
needs the handle — a variable that does not fit its region of the arena — is refused behind it: tests/test_gpu_delta_q8.py.)"""
import ctypes as C

import pytest

from ams_amd import delta as D, hip, spec as S

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1
LAYOUTS = {"trainable": D.delta_layout(S.build_spec(19), "coord_desc_rand"), "all": D.delta_layout(S.build_spec(19), "full_model")}


def _table(layout, edit=None):
    src = layout.table()
    t = (hip.DeltaVar * len(src))()
    for d, s in zip(t, src):
        d.region, d.reserved, d.offset, d.count, d.mask_offset = s.region, 0, s.offset, s.count, s.mask_offset
    if edit:
        edit(t)
    return t


def _set(i, **fields):
    def edit(t):
        for k, v in fields.items():
            setattr(t[i], k, v)
    return edit


def _args(**over):
    a = dict(layout="all", edit=None, n_vars=None, table=True, mask=UNREAD, base_p=UNREAD, base_s=UNREAD, advance=0, payload=UNREAD, cap_short=0,
             size=UNREAD, status=UNREAD, scratch=UNREAD, short=0, n_bytes=1000, n_applied=UNREAD)
    a.update(over)
    return a


def _call(entry, a):
    """The entry on the arguments of `a` with a NULL handle; scratch_elems is what the entry's _scratch asks for the table, less a["short"];
    the encoder's cap is the mask and scale sections, less a["cap_short"]."""
    lib = hip.lib()
    L = LAYOUTS[a["layout"]]
    good = L.table()
    t = _table(L, a["edit"]) if a["table"] else None
    n = len(good) if a["n_vars"] is None else a["n_vars"]
    if entry == "encode":
        elems = lib.ams_student_encode_delta_q8_scratch(good, len(good)) - a["short"]
        cap = L.mask_bytes + 4 * len(good) - a["cap_short"]
        return lib.ams_student_encode_delta_q8(NULL, a["mask"], t, n, a["base_p"], a["base_s"], a["advance"], a["payload"], cap, a["size"],
                                               a["status"], a["scratch"], elems, NULL)
    assert entry == "apply"
    elems = lib.ams_student_apply_delta_q8_scratch(good, len(good)) - a["short"]
    return lib.ams_student_apply_delta_q8(NULL, a["payload"], a["n_bytes"], t, n, a["n_applied"], a["status"], a["scratch"], elems, NULL)


BOTH, ENC, APP = ("encode", "apply"), ("encode",), ("apply",)

# a fault per refusable argument, in the order of refusal: name -> (entries that take it, overrides, the word in the message)
FAULTS = {
    "pointer": (BOTH, dict(status=NULL), b"null pointer"),
    "payload": (APP, dict(payload=NULL), b"payload bytes at"),
    "advance_base": (ENC, dict(advance=2), b"advance_base"),
    "table": (BOTH, dict(edit=_set(3, mask_offset=1)), b"malformed table"),
    "stats_base": (ENC, dict(base_s=NULL), b"null statistics base"),
    "scratch": (BOTH, dict(short=1), b"scratch too small"),
    "cap": (ENC, dict(cap_short=1), b"mask and scale sections"),
}
RANK = list(FAULTS)

MORE = [("pointer", ENC, dict(base_p=NULL)), ("pointer", ENC, dict(payload=NULL)), ("pointer", ENC, dict(size=NULL)), ("pointer", BOTH, dict(scratch=NULL)),
        ("pointer", APP, dict(n_applied=NULL)), ("payload", APP, dict(n_bytes=-1)),
        ("advance_base", ENC, dict(advance=-1)),
        ("table", BOTH, dict(table=False)), ("table", BOTH, dict(n_vars=0)), ("table", BOTH, dict(n_vars=hip.DELTA_MAX_VARS + 1)),
        ("table", BOTH, dict(edit=_set(0, region=hip.REGION_GRADS))), ("table", BOTH, dict(edit=_set(5, count=-1))),
        ("table", BOTH, dict(edit=_set(5, offset=-8))), ("table", BOTH, dict(edit=_set(0, mask_offset=8))),
        ("scratch", BOTH, dict(short=1000))]

SINGLE = [(e, f, FAULTS[f][1]) for f in RANK for e in FAULTS[f][0]] + [(e, f, o) for f, es, o in MORE for e in es]


def _id(v):
    if isinstance(v, str):
        return v
    return ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else "edited" if callable(v[k]) else v[k]) for k in v)


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
    for entry in BOTH:
        mine = [f for f in RANK if entry in FAULTS[f][0]]
        out += [(entry, first, later) for i, first in enumerate(mine) for later in mine[i + 1:]]
    return out


@pytest.mark.parametrize("entry,first,later", _pairs())
def test_the_earlier_ranked_fault_wins(entry, first, later):
    msg = _refused(entry, _args(**dict(FAULTS[first][1], **FAULTS[later][1])), FAULTS[first][2])
    assert FAULTS[later][2] not in msg, msg


@pytest.mark.parametrize("entry", BOTH)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_a_call_without_fault_ends_at_the_handle(entry, layout):
    _refused(entry, _args(layout=layout), b"null handle")


def test_a_null_statistics_base_serves_a_layout_without_statistics():
    """the trainable layout has no entry in AMS_REGION_STATS: base_stats_dev may be NULL, and so may the mask (= every element)"""
    msg = _refused("encode", _args(layout="trainable", base_s=NULL, mask=NULL), b"null handle")
    assert b"statistics" not in msg
    _refused("apply", _args(payload=NULL, n_bytes=0), b"null handle")          # an empty payload needs no pointer
