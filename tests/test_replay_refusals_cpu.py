"""The refusals of the replay memory's gather entries (k_replay.hip), without a GPU: ``ams_replay_gather``, ``ams_replay_gather_logits`` and
``ams_replay_gather_logits_lowres`` share one check of the descriptor table, ``ams_replay_gather_f32`` uses its slot part and refuses a
cropped or flipped descriptor itself.  Every refusal comes before anything is launched, so the library answers it on a host without a
device: the slots and the outputs are NumPy arrays filled with a marker, and a refused call leaves them as they were."""
import ctypes as C

import numpy as np
import pytest

from ams_amd import hip

E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)
MARK = 0xA5
CAP, SRC, CROP, GRID, CH, BATCH = 3, (6, 10), (4, 8), (2, 3), 3, 2
GOOD = (1, 6, 10, 2, 1, 1)        # slot, th, tw, top, left, flip: a mirrored crop inside the slack (6 - 4, 10 - 8)
# the second descriptor of the table is the bad one: the whole table is checked, not its head
BAD_SAMPLE = {"slot_out_of_range": (CAP, 6, 10, 0, 0, 0), "slot_negative": (-1, 6, 10, 0, 0, 0), "th_below_H": (1, CROP[0] - 1, 10, 0, 0, 0),
              "origin_past_the_slack": (1, 6, 10, 6 - CROP[0] + 1, 0, 0)}


def _marked(nbytes):
    return np.full(nbytes, MARK, dtype=np.uint8)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(entry, samples, batch=BATCH, null=None):
    """One call of ``entry`` with every buffer on the host; returns (rc, message, the marked buffers)."""
    n_src, n_crop = SRC[0] * SRC[1], CROP[0] * CROP[1]
    if entry == "ams_replay_gather":
        p = {"frame_slots": _marked(CAP * n_src * 3), "label_slots": _marked(CAP * n_src), "frames_out": _marked(BATCH * n_crop * 3),
             "labels_out": _marked(BATCH * n_crop)}
    elif entry == "ams_replay_gather_logits":
        p = {"slots": _marked(CAP * n_src * CH * 4), "out": _marked(BATCH * n_crop * CH * 4)}
    elif entry == "ams_replay_gather_logits_lowres":
        p = {"slots": _marked(CAP * GRID[0] * GRID[1] * CH * 4), "out": _marked(BATCH * n_crop * CH * 4)}
    else:
        p = {"slots": _marked(CAP * n_src * CH * 4), "out": _marked(BATCH * n_src * CH * 4)}
    marked = dict(p)
    p["samples_host"] = np.ascontiguousarray(samples, dtype=np.int32)
    p["samples_dev"] = p["samples_host"].copy()                   # never read: the table is checked on its host copy
    if null is not None:
        assert null in p
        p[null] = None
    table = (_ptr(p["samples_dev"]), _ptr(p["samples_host"]), batch)
    lib = hip.lib()
    if entry == "ams_replay_gather":
        rc = lib.ams_replay_gather(_ptr(p["frame_slots"]), n_src * 3, _ptr(p["label_slots"]), n_src, CAP, SRC[0], SRC[1], *table, CROP[0], CROP[1],
                                   _ptr(p["frames_out"]), _ptr(p["labels_out"]), None)
    elif entry == "ams_replay_gather_logits":
        rc = lib.ams_replay_gather_logits(_ptr(p["slots"]), n_src * CH, CAP, SRC[0], SRC[1], CH, *table, CROP[0], CROP[1], _ptr(p["out"]), None)
    elif entry == "ams_replay_gather_logits_lowres":
        rc = lib.ams_replay_gather_logits_lowres(_ptr(p["slots"]), GRID[0] * GRID[1] * CH, CAP, GRID[0], GRID[1], CH, SRC[0], SRC[1], *table, CROP[0],
                                                 CROP[1], _ptr(p["out"]), None)
    else:
        rc = lib.ams_replay_gather_f32(_ptr(p["slots"]), n_src * CH, CAP, SRC[0], SRC[1], CH, *table, _ptr(p["out"]), None)
    return rc, lib.ams_last_error(), marked


def _untouched(marked):
    return all((a == MARK).all() for a in marked.values())


CROPPING = {"ams_replay_gather": ("frame_slots", "label_slots", "samples_dev", "samples_host", "frames_out", "labels_out"),
            "ams_replay_gather_logits": ("slots", "samples_dev", "samples_host", "out"),
            "ams_replay_gather_logits_lowres": ("slots", "samples_dev", "samples_host", "out")}
CASES = [(entry, bad) for entry, pointers in sorted(CROPPING.items())
         for bad in sorted(BAD_SAMPLE) + ["batch_0"] + ["null_" + name for name in pointers]]


@pytest.mark.parametrize("entry,bad", CASES, ids=["%s-%s" % c for c in CASES])
def test_every_refusal_of_the_cropping_entries_needs_no_device(entry, bad):
    if bad in BAD_SAMPLE:
        rc, msg, marked = _call(entry, [GOOD, BAD_SAMPLE[bad]])
    elif bad == "batch_0":
        rc, msg, marked = _call(entry, [GOOD, GOOD], batch=0)
    else:
        rc, msg, marked = _call(entry, [GOOD, GOOD], null=bad[len("null_"):])
    assert rc == E_INVALID
    assert msg.startswith(entry[len("ams_"):].encode() + b": ")     # (replay_gather is a prefix of the other two: the colon tells them apart)
    if bad in BAD_SAMPLE:
        assert b"sample 1" in msg
    assert _untouched(marked)


WHOLE = (1, 6, 10, 0, 0, 0)
WHOLE_SLOT_CASES = {"slot_out_of_range": ((CAP, 6, 10, 0, 0, 0), b"replay_gather_f32: "), "flipped": ((1, 6, 10, 0, 0, 1), b"cropped or flipped"),
                    "offset_top": ((1, 6, 10, 1, 0, 0), b"cropped or flipped"), "offset_left": ((1, 6, 10, 0, 1, 0), b"cropped or flipped")}


@pytest.mark.parametrize("bad", sorted(WHOLE_SLOT_CASES))
def test_every_descriptor_refusal_of_the_whole_slot_entry_needs_no_device(bad):
    sample, words = WHOLE_SLOT_CASES[bad]
    rc, msg, marked = _call("ams_replay_gather_f32", [WHOLE, sample])
    assert rc == E_INVALID
    assert msg.startswith(b"replay_gather_f32: ") and words in msg and b"sample 1" in msg
    assert _untouched(marked)
