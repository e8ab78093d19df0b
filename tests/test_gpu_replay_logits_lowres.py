"""Teacher logits cached on a grid smaller than the frame through the replay memory's descriptors (ams_replay_gather_logits_lowres,
k_replay.hip).  The rule (include/ams_hip.h): a low-resolution slot behaves, bit for bit, as a frame-size slot that holds its own
align-corners upsample.  Stage U, the upsample by the soft loss kernel's arithmetic, is restated in NumPy in tests/teacher_labels_ref.py — f32
scale, f32 product, f32 weights, bilerp's operation order, the cached sample itself on a grid point; Stage G is the restatement of tests/test_gpu_replay_logits.py.
The expected value is ``resample_batch(U(slots), desc, H, W)`` and the kernel must give its bits.

The three rescaling cases are that file's, each with its own source size (an exact 2x down-scale to a 16 x 32 crop does not exist for 24 x 40
frames); every cached grid is no larger than any of the sources."""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import hip
from ams_amd.replay import DeviceReplayMemory
from teacher_labels_ref import src_taps, upsample
from test_gpu_replay_logits import CROP, RESCALE, SRC, _bits, _logits, resample_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)
GRIDS = [(5, 9), (3, 5), (1, 1), (24, 9), (5, 40)]
CHANNELS = [19, 21, 1, 8]
CI6 = [0, 1, 2, 10, 11, 13]


def assert_interpolates(grid, src):
    """What keeps a case from passing on grid points alone: on every axis where the grid is smaller than the source (and has more than one
    point) U has positions between cached samples; a grid other than (1, 1) has such an axis, a grid smaller on both has pixels off both."""
    if tuple(grid) == (1, 1):
        return
    ty, tx = src_taps(src[0], grid[0])[2], src_taps(src[1], grid[1])[2]
    off_y, off_x = 1 < grid[0] < src[0], 1 < grid[1] < src[1]
    assert off_y or off_x
    assert (ty != 0).any() == off_y and (tx != 0).any() == off_x
    if off_y and off_x:
        assert ((ty != 0)[:, None] & (tx != 0)[None, :]).sum() > src[0] * src[1] // 2


# ---------------------------------------------------------------------------------------------------------
def _fill(logits, src, capacity=None, upsample_opt=True, select=None):
    shape = tuple(logits[0].shape)
    mem = DeviceReplayMemory(capacity or len(logits), src[0], src[1], DEV, logits_shape=shape, logits_upsample=upsample_opt, logits_select=select)
    frame, label = np.zeros(tuple(src) + (3,), np.uint8), np.zeros(tuple(src), np.uint8)
    for t in logits:
        mem.append(frame, label, t)
    return mem


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d floats differ" % (int((_bits(got) != _bits(want)).sum()), got.size)


def _check(mem, held, src, desc, crop=CROP):
    """``held``: the cached grids the memory holds now, by logical index."""
    desc = np.asarray(desc, dtype=np.int32)
    got = mem.gather_logits(desc, crop[0], crop[1])
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(desc),) + tuple(crop) + (held[0].shape[2],)
    got = got.cpu().numpy()
    _same_bits(got, resample_batch([upsample(t, src[0], src[1]) for t in held], desc, crop[0], crop[1]))
    return got


def _descriptors(case):
    """(source, descriptors) of item 1: the crop-only copy at left 3 and 4, or a rescaling case with crops at the origin, at the maximal
    slack and in the middle, each unflipped and flipped."""
    if case == "copy":
        return SRC, [[1, SRC[0], SRC[1], 2, left, flip] for left in (3, 4) for flip in (0, 1)] + [[0, SRC[0], SRC[1], 8, 8, 1]]
    src, (th, tw) = RESCALE[case]
    sh, sw = th - CROP[0], tw - CROP[1]
    origins = [(0, 0), (sh, sw), (sh // 2, sw // 2), (0, sw), (sh, 0)]
    return src, [[k % 3, th, tw, top, left, flip] for flip in (0, 1) for k, (top, left) in enumerate(origins)]


CASES = ["copy"] + sorted(RESCALE)


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_kernel_is_the_restatement(case, grid, ch):
    src, desc = _descriptors(case)
    assert grid[0] <= src[0] and grid[1] <= src[1]
    assert_interpolates(grid, src)
    logits = _logits(grid, ch, 3, seed=len(case) + ch + grid[0])
    _check(_fill(logits, src), logits, src, desc)


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("case", CASES)
def test_device_against_a_full_size_memory_holding_u(case, grid, ch):
    """Independent of the NumPy blend: the frame-size gather over slots that hold NumPy's U gives the same bits."""
    src, desc = _descriptors(case)
    desc = np.asarray(desc, dtype=np.int32)
    logits = _logits(grid, ch, 3, seed=len(case) + ch + grid[0])
    low = _fill(logits, src)
    full = _fill([upsample(t, src[0], src[1]) for t in logits], src, upsample_opt=False)
    assert full.logits_at_source and (not low.logits_at_source or tuple(grid) == tuple(src))
    _same_bits(low.gather_logits(desc, *CROP).cpu().numpy(), full.gather_logits(desc, *CROP).cpu().numpy())


def test_grid_points_keep_the_cached_bits():
    """The grid-point branch: where U falls on a cached sample it is that sample, the sign of a zero included."""
    t = _logits((5, 9), 19, 1, seed=9)[0]
    t[0, 0, 0], t[3, 7, 3], t[2, 4, 5] = -0.0, -0.0, -0.0
    src = (9, 17)                                                 # every second point of U is a cached sample
    u = upsample(t, *src)
    _same_bits(np.ascontiguousarray(u[::2, ::2]), t)
    mem = _fill([t], src)
    got = mem.gather_logits(np.array([[0, 9, 17, 0, 0, 0], [0, 9, 17, 1, 1, 1]], dtype=np.int32), 8, 16).cpu().numpy()
    _same_bits(got[0], np.ascontiguousarray(u[:8, :16]))
    _same_bits(got[1], np.ascontiguousarray(u[1:9, 1:17][:, ::-1]))
    assert np.signbit(got[0][0, 0, 0]) and np.signbit(got[0][6, 14, 3]) and np.signbit(got[0][4, 8, 5])
    assert np.signbit(got[1][3, 8, 5])                            # U(4, 8) again: row 4 - 1, column 1 + 15 - 8 of the mirrored window


@pytest.mark.parametrize("ch", [19, 21])
def test_mixed_batch_from_a_wrapped_ring(ch):
    """One batch of five: copy, mirrored copy, up-scale, mirrored down-scale, and one slot twice, from a ring of three slots after five
    appends."""
    logits = _logits((5, 9), ch, 5, seed=ch)
    mem = _fill(logits, SRC, capacity=3)
    held = logits[2:]
    assert len(mem) == 3 and mem.ring.head != 0
    desc = [[0, 24, 40, 5, 3, 0], [2, 24, 40, 8, 8, 1], [1, 30, 50, 14, 18, 0], [0, 20, 34, 4, 2, 1], [2, 30, 50, 0, 0, 1]]
    _check(mem, held, SRC, desc)
    assert np.array_equal(mem[0][2].cpu().numpy(), logits[2])


def test_rows_wider_than_a_block_segment():
    """A block owns 128 pixels of an output row: 260 columns are two whole segments and one of four pixels."""
    src, crop = (6, 300), (4, 260)
    assert_interpolates((2, 20), src)
    logits = _logits((2, 20), 19, 2, seed=5)
    mem = _fill(logits, src)
    desc = [[0, 6, 300, 1, 40, 0], [1, 6, 300, 2, 37, 0], [0, 6, 300, 0, 33, 1], [1, 7, 350, 3, 90, 0], [0, 5, 270, 1, 10, 1]]
    _check(mem, logits, src, desc, crop)


@pytest.mark.parametrize("case", CASES)
def test_selected_layout_is_np_take_of_the_full_layout(case):
    src, desc = _descriptors(case)
    desc = np.asarray(desc, dtype=np.int32)
    logits = _logits((5, 9), 19, 3, seed=11)
    full = _fill(logits, src).gather_logits(desc, *CROP).cpu().numpy()
    sel = _fill(logits, src, select=CI6)
    assert sel.logits_cached_shape == (5, 9, 6) and sel.logits_layout == "selected"
    got = sel.gather_logits(desc, *CROP).cpu().numpy()
    _same_bits(got, np.ascontiguousarray(np.take(full, CI6, axis=-1)))


def test_peaked_logits():
    """+-1e4, the one-hot limit of tests/test_gpu_soft_teacher.py: neither stage overflows or leaves the range of the cached values."""
    rng = np.random.default_rng(2)
    logits = []
    for _ in range(2):
        t = np.full((5, 9, 19), -1e4, dtype=np.float32)
        np.put_along_axis(t, rng.integers(0, 19, (5, 9))[..., None], 1e4, axis=2)
        logits.append(t)
    mem = _fill(logits, SRC)
    got = _check(mem, logits, SRC, [[0, 30, 50, 7, 9, 0], [1, 24, 40, 8, 8, 1], [1, 20, 34, 4, 2, 1], [0, 24, 40, 0, 0, 0]])
    assert np.isfinite(got).all() and np.abs(got).max() <= 1e4
    assert got[3].max() == 1e4 and got[3].min() == -1e4           # the window at the origin holds cached samples themselves


def _raw_call(mem, table, batch, out, crop=CROP, slots=True, samples_dev=True, samples_host=True, out_ptr=True, grid=None, stride=None):
    table_dev = torch.from_numpy(table).to(DEV)
    lh, lw, ch = mem.logits_cached_shape
    if grid is not None:
        lh, lw = grid
    rc = hip.lib().ams_replay_gather_logits_lowres(C.c_void_p(mem._logits.data_ptr() if slots else 0), mem.logits_stride if stride is None else stride,
                                                   mem.capacity, lh, lw, ch, mem.src_h, mem.src_w,
                                                   C.c_void_p(table_dev.data_ptr() if samples_dev else 0),
                                                   table.ctypes.data_as(C.c_void_p) if samples_host else C.c_void_p(0), batch, crop[0], crop[1],
                                                   C.c_void_p(out.data_ptr() if out_ptr else 0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("bad", ["slot_out_of_range", "negative_slot", "th_below_H", "origin_past_the_slack", "batch_0", "null_slots",
                                 "null_samples_dev", "null_samples_host", "null_out", "lh_above_src_h", "lw_0", "stride_below_the_slot"])
def test_bad_calls_are_refused_before_the_launch(bad):
    logits = _logits((5, 9), 19, 3, seed=1)
    mem = _fill(logits, SRC)
    table = np.array([[0, 24, 40, 0, 0, 0], [1, 30, 50, 14, 18, 1]], dtype=np.int32)
    batch, kw = 2, {}
    if bad == "slot_out_of_range":
        table[1, 0] = 3
    elif bad == "negative_slot":
        table[0, 0] = -1
    elif bad == "th_below_H":
        table[1, 1:5] = (15, 50, 0, 0)
    elif bad == "origin_past_the_slack":
        table[1, 4] = 50 - 32 + 1
    elif bad == "batch_0":
        batch = 0
    elif bad == "lh_above_src_h":
        kw = {"grid": (SRC[0] + 1, 9)}
    elif bad == "lw_0":
        kw = {"grid": (5, 0)}
    elif bad == "stride_below_the_slot":
        kw = {"stride": 5 * 9 * 19 - 1}
    else:
        kw = {{"null_slots": "slots", "null_samples_dev": "samples_dev", "null_samples_host": "samples_host", "null_out": "out_ptr"}[bad]: False}
    out = torch.full((2,) + CROP + (19,), 7.0, dtype=torch.float32, device=DEV)
    rc = _raw_call(mem, table, batch, out, **kw)
    assert rc == E_INVALID and b"replay_gather_logits_lowres" in hip.lib().ams_last_error()
    assert bool((out == 7.0).all())
    # the same call, well formed, goes through
    good = np.array([[0, 24, 40, 0, 0, 0], [1, 30, 50, 14, 18, 1]], dtype=np.int32)
    assert _raw_call(mem, good, 2, out) == 0
    _same_bits(out.cpu().numpy(), resample_batch([upsample(t, *SRC) for t in logits], good, *CROP))


def test_without_the_keyword_a_low_resolution_cache_still_refuses_crops():
    mem = _fill(_logits((5, 9), 19, 2, seed=3), SRC, upsample_opt=False)
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache .5x9 logits") as e:
        mem.gather_logits(np.array([[0, 24, 40, 2, 3, 0]], dtype=np.int32), *CROP)
    assert "logits_upsample=True" in str(e.value)
    with pytest.raises(AssertionError, match="no larger than the frame"):
        DeviceReplayMemory(2, SRC[0], SRC[1], DEV, logits_shape=(25, 9, 19), logits_upsample=True)
