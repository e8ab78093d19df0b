"""Hard teacher labels derived from cached teacher logits on the device (ams_teacher_labels_from_logits, k_replay.hip; include/ams_hip.h,
DESIGN 4.6): label(Y, X) = argmax_c U(Y, X, c), U the align-corners upsample of the soft loss kernel, the first maximum wins.  Every label
is an integer decided by f32 operations that the NumPy restatement (tests/teacher_labels_ref.py) performs one at a time in the same order,
so the device must give the restatement's labels exactly: no tolerance anywhere in this file.  Then ``DeviceReplayMemory.append(frame, None,
logits)``: the slot holds what ``append(frame, restated_label, logits)`` stores."""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import hip
from ams_amd.replay import DeviceReplayMemory
from teacher_labels_ref import grid_points, labels_from_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)
CI6 = [0, 1, 2, 10, 11, 13]
FILL = 0xA5                       # what the output holds before a call: a label map of up to 255 classes never needs it to be a non-label


def _logits(shape, seed, n=1):
    """Independent normal logits: neighbouring cached samples favour different classes, so the argmax changes between them."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n,) + tuple(shape)).astype(np.float32)


def _derive(t, Hs, Ws, slot_stride=None, out_stride=None, out_offset=0):
    """The raw C entry over ``t`` f32 [n, lh, lw, NC]: (rc, the whole output buffer uint8 [n, out_stride] on the host)."""
    n, lh, lw, nc = t.shape
    item = lh * lw * nc
    slot_stride = item if slot_stride is None else slot_stride
    out_stride = Hs * Ws if out_stride is None else out_stride
    src = np.full((n, max(slot_stride, item)), np.float32(np.nan), dtype=np.float32)          # the padding must never be read into a label
    src[:, :item] = t.reshape(n, item)
    src_dev = torch.from_numpy(src).to(DEV)
    out = torch.full((out_offset + n * out_stride,), FILL, dtype=torch.uint8, device=DEV)
    rc = hip.lib().ams_teacher_labels_from_logits(C.c_void_p(src_dev.data_ptr()), slot_stride, n, lh, lw, nc, Hs, Ws,
                                                  C.c_void_p(out.data_ptr() + out_offset), out_stride,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()[out_offset:].reshape(n, out_stride)


def _check(t, Hs, Ws, **kw):
    rc, buf = _derive(t, Hs, Ws, **kw)
    assert rc == 0, hip.lib().ams_last_error()
    got = buf[:, :Hs * Ws].reshape(len(t), Hs, Ws)
    want = np.stack([labels_from_logits(x, Hs, Ws) for x in t])
    bad = got != want
    assert not bad.any(), "%d of %d labels differ, first at %s" % (int(bad.sum()), bad.size, np.argwhere(bad)[:3].tolist())
    assert bool((buf[:, Hs * Ws:] == FILL).all()), "bytes past Hs * Ws of an item were written"
    return got


SHAPES = [((3, 5, 19), (32, 64)),
          ((4, 7, 21), (33, 70)),             # odd width, a partial segment, rows that do not start on 4 bytes
          ((1, 1, 19), (8, 16)),              # one cached sample: scale 0 on both axes
          ((1, 5, 6), (1, 40)),               # one output row
          ((16, 32, 19), (16, 32)),           # identity: every position is a grid point
          ((3, 5, 1), (32, 64)),              # NC = 1: every label is 0
          ((3, 5, 255), (32, 64)),            # NC = 255, the most
          ((9, 300, 19), (9, 300)),           # identity at 129 cached columns per segment: three segments, the last of 44 pixels
          ((24, 40, 255), (24, 40))]          # dense grid and many classes: 8-pixel segments, the widest whose cached columns fit in LDS


@pytest.mark.parametrize("shape,size", SHAPES, ids=lambda v: "x".join(str(d) for d in v))
def test_device_labels_are_the_restatement(shape, size):
    got = _check(_logits(shape, seed=sum(shape) + size[1]), *size)
    if shape[2] > 1 and shape[:2] != (1, 1):
        assert len(np.unique(got)) > 1                            # the case decides something
    if shape[2] == 255:
        assert got.max() > 200


def test_three_items_with_padded_strides():
    t = _logits((3, 5, 19), seed=7, n=3)
    # 3 * 5 * 19 = 285 floats in slots of 320; 20 x 36 = 720 label bytes in items of 1024, and in items of 721 from an odd base (byte stores)
    _check(t, 20, 36, slot_stride=320, out_stride=1024)
    _check(t, 20, 36, slot_stride=286, out_stride=721, out_offset=1)
    _check(t, 20, 36, slot_stride=285, out_stride=720, out_offset=2)


@pytest.fixture(scope="module")
def full_frame():
    """One 33 x 65 x 19 grid under a 512 x 1024 frame (eight segments per row): logits, the restated labels, computed once."""
    t = _logits((33, 65, 19), seed=33)
    want = labels_from_logits(t[0], 512, 1024)
    want.setflags(write=False)
    return t, want


def test_full_size_frame(full_frame):
    t, want = full_frame
    rc, buf = _derive(t, 512, 1024)
    assert rc == 0 and np.array_equal(buf.reshape(512, 1024), want)
    assert len(np.unique(want)) == 19
    on_grid, ylo, xlo = grid_points(512, 1024, 33, 65)
    assert on_grid[0, 0] and not on_grid.all()
    assert np.array_equal(want[on_grid], np.argmax(t[0], axis=-1)[ylo][:, xlo][on_grid])          # a grid point: the cached sample's own argmax


def test_ties_take_the_lowest_index():
    # all equal: label 0 everywhere, between the cached samples too (equal values interpolate to the same value in every class)
    t = np.full((1, 3, 5, 19), 1.25, dtype=np.float32)
    assert not _check(t, 32, 64).any()
    # two equal maxima: the lower index, on grid points and between them
    t = np.zeros((1, 3, 5, 19), dtype=np.float32)
    t[..., 4] = 2.0
    t[..., 11] = 2.0
    assert (_check(t, 32, 64) == 4).all()
    t[..., 2] = 2.0
    assert (_check(t, 32, 64) == 2).all()
    # -0.0 against +0.0: equal, the lower index wins whichever carries the sign (identity: the cached samples themselves are compared)
    for first, second in ((-0.0, 0.0), (0.0, -0.0)):
        t = np.full((1, 16, 32, 19), -1.0, dtype=np.float32)
        t[..., 3] = first
        t[..., 9] = second
        assert (_check(t, 16, 32) == 3).all()
    # ... and between the samples of a smaller grid
    t = np.full((1, 3, 5, 19), -1.0, dtype=np.float32)
    t[..., 5] = -0.0
    t[..., 6] = 0.0
    assert (_check(t, 32, 64) == 5).all()


@pytest.mark.parametrize("bad", ["n_0", "lh_0", "lh_above_Hs", "lw_0", "lw_above_Ws", "nc_0", "nc_256", "slot_stride", "out_stride", "null_logits",
                                 "null_out"])
def test_bad_calls_are_refused_and_write_nothing(bad):
    n, lh, lw, nc, Hs, Ws = 2, 3, 5, 19, 32, 64
    args = dict(n=n, lh=lh, lw=lw, nc=nc, slot=lh * lw * nc, out=Hs * Ws)
    args.update({"n_0": dict(n=0), "lh_0": dict(lh=0), "lh_above_Hs": dict(lh=Hs + 1), "lw_0": dict(lw=0), "lw_above_Ws": dict(lw=Ws + 1),
                 "nc_0": dict(nc=0), "nc_256": dict(nc=256), "slot_stride": dict(slot=lh * lw * nc - 1), "out_stride": dict(out=Hs * Ws - 1)}.get(bad, {}))
    src = torch.zeros(2 * (Hs + 1) * (Ws + 1) * 256, dtype=torch.float32, device=DEV)          # large enough for what any refused shape names
    out = torch.full((n * Hs * Ws,), FILL, dtype=torch.uint8, device=DEV)
    rc = hip.lib().ams_teacher_labels_from_logits(C.c_void_p(0 if bad == "null_logits" else src.data_ptr()), args["slot"], args["n"], args["lh"],
                                                  args["lw"], args["nc"], Hs, Ws, C.c_void_p(0 if bad == "null_out" else out.data_ptr()),
                                                  args["out"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == E_INVALID and b"teacher_labels_from_logits" in hip.lib().ams_last_error()
    assert bool((out == FILL).all())


# ---------------------------------------------------------------------------------------------------------
# the replay memory
# ---------------------------------------------------------------------------------------------------------
SRC, GRID = (32, 64), (3, 5)


def _material(n, seed):
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(n)]
    logits = list(_logits(GRID + (19,), seed=seed + 1, n=n))
    return frames, logits, [labels_from_logits(t, *SRC) for t in logits]


@pytest.mark.parametrize("select", [None, CI6], ids=["full", "selected"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_append_without_a_label_stores_the_restated_labels(select, where):
    frames, logits, labels = _material(3, seed=5)
    kw = dict(logits_shape=GRID + (19,), logits_upsample=True, logits_select=select)
    derived, given = DeviceReplayMemory(2, *SRC, DEV, **kw), DeviceReplayMemory(2, *SRC, DEV, **kw)          # three appends: the ring wraps
    for f, t, l in zip(frames, logits, labels):
        derived.append(f, None, torch.from_numpy(t).to(DEV) if where == "device" else t)
        given.append(f, l, t)
    assert len(derived) == len(given) == 2
    for i in range(2):
        (fa, la, ta), (fb, lb, tb) = derived[i], given[i]
        assert torch.equal(fa, fb) and torch.equal(ta, tb) and tuple(ta.shape) == derived.logits_cached_shape
        assert np.array_equal(la.cpu().numpy(), labels[i + 1])
        assert torch.equal(la, lb)
    assert np.array_equal(derived.labels_from_logits(logits[0]).cpu().numpy(), labels[0])          # ... and without storing
    assert len(derived) == 2


def test_frame_size_logits_take_the_same_kernel():
    rng = np.random.default_rng(8)
    t = _logits(SRC + (19,), seed=9)[0]
    mem = DeviceReplayMemory(1, *SRC, DEV, logits_shape=SRC + (19,))
    mem.append(rng.integers(0, 256, SRC + (3,), dtype=np.uint8), None, t)
    assert np.array_equal(mem[0][1].cpu().numpy(), np.argmax(t, axis=-1).astype(np.uint8))
    assert np.array_equal(mem[0][2].cpu().numpy(), t)


def test_refusals_of_append_without_a_label():
    frames, logits, _labels = _material(1, seed=6)
    sel = DeviceReplayMemory(2, *SRC, DEV, logits_shape=GRID + (19,), logits_select=CI6)
    with pytest.raises(ValueError, match="argmax over all classes is not defined"):
        sel.append(frames[0], None, np.take(logits[0], CI6, axis=-1))
    with pytest.raises(ValueError, match="argmax over all classes is not defined"):
        sel.labels_from_logits(np.take(logits[0], CI6, axis=-1))
    assert len(sel) == 0
    plain = DeviceReplayMemory(2, *SRC, DEV)
    with pytest.raises(AssertionError, match="logits_shape"):
        plain.append(frames[0], None)
    with pytest.raises(AssertionError, match="logits_shape"):
        plain.append(frames[0], None, logits[0])
    assert len(plain) == 0
