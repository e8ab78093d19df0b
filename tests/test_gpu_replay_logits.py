"""Teacher logits through the replay memory's descriptors (ams_replay_gather_logits, k_replay.hip): the crop of the logits rescaled to
(th, tw), mirrored when flipped, at the label size.  The rule is the project's own (include/ams_hip.h); it is restated here in
NumPy from its definition — coordinates in float64, weights and every arithmetic step in float32 — and the kernel must give its bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import hip
from ams_amd.replay import DeviceReplayMemory

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SRC, CROP = (24, 40), (16, 32)
E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)


# ---------------------------------------------------------------------------------------------------------
# the definition, restated
# ---------------------------------------------------------------------------------------------------------
def raw_positions(c, n_in, n_out):
    """f of the definition for the integer positions c of the rescaled axis, in float64"""
    return (np.asarray(c, dtype=np.float64) + np.float64(0.5)) * (np.float64(n_in) / np.float64(n_out)) - np.float64(0.5)


def taps(c, n_in, n_out):
    f = raw_positions(c, n_in, n_out)
    fl = np.floor(f)
    w = (f - fl).astype(np.float32)
    s = fl.astype(np.int64)
    lo, hi = s < 0, s >= n_in - 1
    s[lo], w[lo] = 0, 0
    s[hi], w[hi] = n_in - 1, 0
    return s, np.minimum(s + 1, n_in - 1), w


def resample_logits(t, desc, H, W):
    """One batch entry: ``t`` f32 [src_h, src_w, C], ``desc`` = (slot, th, tw, top, left, flip) -> f32 [H, W, C]."""
    t = np.asarray(t, dtype=np.float32)
    _slot, th, tw, top, left, flip = (int(v) for v in desc)
    src_h, src_w = t.shape[:2]
    x = np.arange(W)
    cy, cx = top + np.arange(H), left + (W - 1 - x if flip else x)
    if (th, tw) == (src_h, src_w):
        return t[cy][:, cx].copy()
    y0, y1, wy = taps(cy, src_h, th)
    x0, x1, wx = taps(cx, src_w, tw)
    wx, wy, one = wx[None, :, None], wy[:, None, None], np.float32(1)
    with np.errstate(all="ignore"):
        r0 = t[y0][:, x0] * (one - wx) + t[y0][:, x1] * wx
        r1 = t[y1][:, x0] * (one - wx) + t[y1][:, x1] * wx
        out = r0 * (one - wy) + r1 * wy
    assert out.dtype == np.float32
    return out


def resample_batch(slots, desc, H, W):
    """``slots``: the logits by logical index; ``desc`` [batch, 6] with logical slots."""
    return np.stack([resample_logits(slots[int(d[0])], d, H, W) for d in desc])


# ---------------------------------------------------------------------------------------------------------
def _logits(src, ch, n, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(tuple(src) + (ch,)) * 3).astype(np.float32) for _ in range(n)]


def _fill(logits, capacity=None):
    src, ch = logits[0].shape[:2], logits[0].shape[2]
    mem = DeviceReplayMemory(capacity or len(logits), src[0], src[1], DEV, logits_shape=src + (ch,))
    frame, label = np.zeros(src + (3,), np.uint8), np.zeros(src, np.uint8)
    for t in logits:
        mem.append(frame, label, t)
    return mem


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(mem, held, desc, crop=CROP):
    """``held``: what the memory holds now, by logical index."""
    desc = np.asarray(desc, dtype=np.int32)
    got = mem.gather_logits(desc, crop[0], crop[1])
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(desc),) + tuple(crop) + (held[0].shape[2],)
    got, want = got.cpu().numpy(), resample_batch(held, desc, crop[0], crop[1])
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d floats differ" % (int((_bits(got) != _bits(want)).sum()), got.size)
    return got


CHANNELS = [19, 21, 1]


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("left", [3, 4])             # 3: no 16-byte piece starts at the window; 4: left * C * 4 is a multiple of 16 for every C
@pytest.mark.parametrize("ch", CHANNELS)
def test_crop_without_rescale_is_a_copy(ch, left, flip):
    logits = _logits(SRC, ch, 2, seed=ch + left)
    top, t = 2, logits[1]
    bottom, right = top + CROP[0] - 1, left + CROP[1] - 1
    t[top - 1, left], t[top, left - 1], t[bottom + 1, left + 7], t[top + 3, right + 1] = np.inf, np.nan, -np.inf, np.inf      # just outside
    t[top, left, 0], t[bottom, right, ch - 1], t[top + 5, left, ch // 2] = np.nan, np.inf, -np.inf                     # on the window's edge
    mem = _fill(logits)
    got = _check(mem, logits, [[1, SRC[0], SRC[1], top, left, flip], [0, SRC[0], SRC[1], 8, 8, flip]])
    window = t[top:top + CROP[0], left:left + CROP[1]]
    window = window[:, ::-1] if flip else window
    assert np.array_equal(~np.isfinite(got[0]), ~np.isfinite(window)) and int((~np.isfinite(got[0])).sum()) == 3
    assert np.isfinite(got[1]).all()


# (source, (th, tw)) of the rescaling cases; the crop is 16 x 32 throughout
RESCALE = {"up": (SRC, (30, 50)), "down_non_integer": ((40, 72), (24, 43)), "down_2x": ((32, 64), (16, 32))}


@pytest.mark.parametrize("ch", CHANNELS)
@pytest.mark.parametrize("case", sorted(RESCALE))
def test_rescaled_crops_at_the_borders_and_inside(case, ch):
    src, (th, tw) = RESCALE[case]
    logits = _logits(src, ch, 3, seed=len(case) + ch)
    mem = _fill(logits)
    slack_h, slack_w = th - CROP[0], tw - CROP[1]
    # crops at the origin and at the maximal slack: the first and the last row and column of the rescaled logits (the up-scale meets both
    # clamps there: test_up_scale_meets_both_clamps)
    desc = [[0, th, tw, 0, 0, 0], [1, th, tw, slack_h, slack_w, 0], [2, th, tw, slack_h // 2, slack_w // 2, 1], [1, th, tw, 0, slack_w, 1],
            [2, th, tw, slack_h, 0, 0]]
    got = _check(mem, logits, desc)
    if case == "down_2x":                                # w = 0.5 on both axes: the 2 x 2 mean
        t = logits[0].astype(np.float64)
        mean = (t[0::2, 0::2] + t[0::2, 1::2] + t[1::2, 0::2] + t[1::2, 1::2]) / 4
        assert slack_h == 0 and slack_w == 0 and np.abs(got[0] - mean).max() < 1e-5


def test_up_scale_meets_both_clamps():
    """The premise of the border cases above, spelled out for the up-scale: the first position falls before the first sample (s < 0) and the
    last one at the last sample (s >= src - 1)."""
    for n_in, n_out in ((24, 30), (40, 50)):
        s = np.floor(raw_positions([0, n_out - 1], n_in, n_out))
        assert s[0] == -1 and s[1] == n_in - 1


@pytest.mark.parametrize("ch", [19, 21])
def test_mixed_batch_from_a_wrapped_ring(ch):
    """One batch of five: copy, mirrored copy, up-scale, mirrored down-scale, and one slot twice, from a ring of three slots after five
    appends — the case is branched per sample, and logical index 0 is the third array appended."""
    logits = _logits(SRC, ch, 5, seed=ch)
    mem = _fill(logits, capacity=3)
    held = logits[2:]
    assert len(mem) == 3 and mem.ring.head != 0
    desc = [[0, 24, 40, 5, 3, 0], [2, 24, 40, 8, 8, 1], [1, 30, 50, 14, 18, 0], [0, 20, 34, 4, 2, 1], [2, 30, 50, 0, 0, 1]]
    _check(mem, held, desc)
    assert np.array_equal(mem[0][2].cpu().numpy(), logits[2])


def test_rows_wider_than_a_block_segment():
    """A block owns 128 pixels of an output row: 260 columns are two whole segments and one of four pixels (copy in 16-byte pieces and
    unaligned, mirrored copy, rescaled)."""
    src, crop = (6, 300), (4, 260)
    logits = _logits(src, 19, 2, seed=5)
    mem = _fill(logits)
    desc = [[0, 6, 300, 1, 40, 0], [1, 6, 300, 2, 37, 0], [0, 6, 300, 0, 33, 1], [1, 7, 350, 3, 90, 0], [0, 5, 270, 1, 10, 1]]
    _check(mem, logits, desc, crop)


def test_peaked_logits():
    """+-1e4, the one-hot limit of tests/test_gpu_soft_teacher.py: the blend neither overflows nor loses the peak."""
    rng = np.random.default_rng(2)
    logits = []
    for _ in range(2):
        t = np.full(SRC + (19,), -1e4, dtype=np.float32)
        cls = rng.integers(0, 19, SRC)
        np.put_along_axis(t, cls[..., None], 1e4, axis=2)
        logits.append(t)
    mem = _fill(logits)
    got = _check(mem, logits, [[0, 30, 50, 7, 9, 0], [1, 24, 40, 8, 8, 1], [1, 20, 34, 4, 2, 1]])
    assert np.isfinite(got).all() and np.abs(got).max() <= 1e4
    assert got[1].max() == 1e4 and got[1].min() == -1e4


def _raw_call(mem, table, batch, out, crop=CROP, slots=True, samples_dev=True, samples_host=True, out_ptr=True):
    table_dev = torch.from_numpy(table).to(DEV)
    rc = hip.lib().ams_replay_gather_logits(C.c_void_p(mem._logits.data_ptr() if slots else 0), mem.logits_stride, mem.capacity, mem.src_h, mem.src_w,
                                            mem.logits_shape[2], C.c_void_p(table_dev.data_ptr() if samples_dev else 0),
                                            table.ctypes.data_as(C.c_void_p) if samples_host else C.c_void_p(0), batch, crop[0], crop[1],
                                            C.c_void_p(out.data_ptr() if out_ptr else 0), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("bad", ["slot_out_of_range", "negative_slot", "th_below_H", "origin_past_the_slack", "batch_0", "null_slots",
                                 "null_samples_dev", "null_samples_host", "null_out"])
def test_bad_calls_are_refused_before_the_launch(bad):
    logits = _logits(SRC, 19, 3, seed=1)
    mem = _fill(logits)
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
    else:
        kw = {{"null_slots": "slots", "null_samples_dev": "samples_dev", "null_samples_host": "samples_host", "null_out": "out_ptr"}[bad]: False}
    out = torch.full((2,) + CROP + (19,), 7.0, dtype=torch.float32, device=DEV)
    rc = _raw_call(mem, table, batch, out, **kw)
    assert rc == E_INVALID and b"replay_gather_logits" in hip.lib().ams_last_error()
    assert bool((out == 7.0).all())
    # the same call, well formed, goes through
    good = np.array([[0, 24, 40, 0, 0, 0], [1, 30, 50, 14, 18, 1]], dtype=np.int32)
    assert _raw_call(mem, good, 2, out) == 0
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(resample_batch(logits, good, *CROP)))


def test_whole_slot_gather_still_refuses_a_flipped_descriptor():
    """ams_replay_gather_f32 is unchanged: whole slots, and a descriptor with an origin or a flip is refused."""
    logits = _logits(SRC, 19, 2, seed=4)
    mem = _fill(logits)
    lib = hip.lib()
    out = torch.full((1,) + SRC + (19,), 7.0, dtype=torch.float32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for fields, ok in (((1, 24, 40, 0, 0, 1), False), ((1, 24, 40, 0, 3, 0), False), ((1, 24, 40, 0, 0, 0), True)):
        table = np.array([fields], dtype=np.int32)
        table_dev = torch.from_numpy(table).to(DEV)
        rc = lib.ams_replay_gather_f32(C.c_void_p(mem._logits.data_ptr()), mem.logits_stride, mem.capacity, 24, 40, 19, C.c_void_p(table_dev.data_ptr()),
                                       table.ctypes.data_as(C.c_void_p), 1, C.c_void_p(out.data_ptr()), st)
        torch.cuda.synchronize()
        if ok:
            assert rc == 0 and np.array_equal(out[0].cpu().numpy(), logits[1])
        else:
            assert rc == E_INVALID and b"cropped or flipped" in lib.ams_last_error() and bool((out == 7.0).all())


def test_a_low_resolution_cache_refuses_crops_in_words():
    """Logits cached on a smaller grid than the frame follow whole frames only, and the refusal says what to do about it."""
    mem = DeviceReplayMemory(2, SRC[0], SRC[1], DEV, logits_shape=(5, 9, 19))
    for _ in range(2):
        mem.append(np.zeros(SRC + (3,), np.uint8), np.zeros(SRC, np.uint8), np.zeros((5, 9, 19), np.float32))
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache"):
        mem.gather_logits(np.array([[0, 24, 40, 2, 3, 0]], dtype=np.int32), *CROP)
    whole = mem.gather_logits(np.array([[1, 24, 40, 0, 0, 0]], dtype=np.int32), *SRC)         # whole frames: the cached grid, as before
    assert tuple(whole.shape) == (1, 5, 9, 19)
