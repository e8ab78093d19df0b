"""Host side of low-resolution teacher logits that follow rescale, crop and flip (``DeviceReplayMemory(..., logits_upsample=True)``),
without a GPU: what ``_replay_plan`` accepts with the keyword and still refuses without it, the shape of the plan's logits buffer, which
entry of the library a phase reaches and with which arguments, and that nothing about the draws changes.  Stand-ins and recorder:
tests/test_replay_logits_cpu.py."""
import numpy as np
import pytest

from ams_amd import replay
from test_replay_cpu import H, MB, _HostMemory, _Net, _memory, _seed, _states
from test_replay_logits_cpu import CH, SRC, _SoftMemory, _soft_memory, _soft_net, lib  # noqa: F401  (lib: the recorder fixture)

GRID = (5, 9)
# (source, scale, flip) that a low-resolution cache is refused for without the keyword (test_replay_logits_cpu.py)
AUGMENTED = [((H, 2 * H), [1, 1.5], False), (SRC, [1], False), ((H, 2 * H), [1], True)]


def _lowres_memory(src, grid=GRID, n=4, select=None):
    mem = _SoftMemory(n, src[0], src[1], "cpu", logits_shape=tuple(grid) + (CH,), logits_upsample=True, logits_select=select)
    frames, labels = _memory(src, n=n, seed=1)
    for f, l in zip(frames, labels):
        mem.append(f, l, np.zeros(tuple(grid) + (CH,), np.float32))
    return mem


@pytest.mark.parametrize("src,scale,flip", AUGMENTED)
def test_replay_plan_accepts_an_opt_in_low_resolution_cache(src, scale, flip):
    mem = _lowres_memory(src)
    assert mem.logits_upsample and mem.logits_follow_frames and not mem.logits_at_source
    _seed(2)
    plan = _soft_net(scale, flip)._replay_plan(mem, 5)
    assert not plan.whole_frames
    assert tuple(plan.logits.shape) == (MB, H, 2 * H, CH)             # the label size: what the soft loss kernel reads as it is
    if flip:
        assert plan.table_host[..., 5].any()


def test_selected_layout_keeps_its_channels_in_the_plan_buffer():
    mem = _lowres_memory(SRC, select=[0, 1, 2, 10, 11, 13])
    assert mem.logits_cached_shape == GRID + (6,)
    _seed(2)
    assert tuple(_soft_net([1, 1.5], True)._replay_plan(mem, 2).logits.shape) == (MB, H, 2 * H, 6)


@pytest.mark.parametrize("src,scale,flip", AUGMENTED)
def test_augmented_phases_reach_the_lowres_entry_only(lib, src, scale, flip):
    mem = _lowres_memory(src)
    net = _soft_net(scale, flip)
    _seed(5)
    net.train_with_deque(mem, None, 6)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_logits_lowres"] * 6
    for _, args in lib.calls:
        # slot_stride, capacity, lh, lw, channels, src_h, src_w ... batch, H, W
        assert args[1:8] == (mem.logits_stride, mem.capacity, GRID[0], GRID[1], CH, src[0], src[1]) and args[10:13] == (MB, H, 2 * H)
    assert mem.logits_stride >= GRID[0] * GRID[1] * CH
    assert net.engine.logits_seen == [(MB, H, 2 * H, CH)] * 6                                  # fed with th, tw = H, W


def test_a_whole_frames_phase_keeps_the_whole_slot_entry(lib):
    mem = _lowres_memory((H, 2 * H))
    net = _soft_net([1])
    _seed(4)
    net.train_with_deque(mem, None, 3)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_f32"] * 3
    assert [args[3:6] for _, args in lib.calls] == [GRID + (CH,)] * 3                          # th, tw, channels: the cached grid
    assert net.engine.logits_seen == [(MB,) + GRID + (CH,)] * 3


def test_a_grid_at_the_frame_size_keeps_the_at_source_entry(lib):
    mem = _lowres_memory(SRC, grid=SRC)
    assert mem.logits_at_source
    net = _soft_net([1, 1.5], True)
    _seed(5)
    net.train_with_deque(mem, None, 2)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_logits"] * 2


@pytest.mark.parametrize("flip", [False, True])
def test_the_opt_in_cache_does_not_change_the_draws(flip):
    tables, states = [], []
    for soft in (False, True):
        if soft:
            mem, net = _lowres_memory(SRC), _soft_net([1, 1.5], flip)
        else:
            mem, net = _HostMemory(4, SRC[0], SRC[1], "cpu"), _Net([1, 1.5])
            net.flip = flip
            for f, l in zip(*_memory(SRC, n=4, seed=1)):
                mem.append(f, l)
        _seed(6)
        tables.append(net._replay_plan(mem, 5).table_host)
        states.append(_states())
    assert np.array_equal(tables[0], tables[1]) and states[0] == states[1]
    assert tables[0].shape == (5, MB, 6) and len({tuple(d[1:3]) for d in tables[0].reshape(-1, 6)}) == 2      # both scales were drawn


@pytest.mark.parametrize("grid", [(2 * H + 1, 9), (5, 4 * H + 1), (0, 9)])
def test_a_grid_larger_than_the_frame_is_refused_at_construction(grid):
    with pytest.raises(AssertionError, match="no larger than the frame") as e:
        _SoftMemory(2, SRC[0], SRC[1], "cpu", logits_shape=tuple(grid) + (CH,), logits_upsample=True)
    assert "%dx%d logits for %dx%d frames" % (tuple(grid) + SRC) in str(e.value)
    _SoftMemory(2, SRC[0], SRC[1], "cpu", logits_shape=tuple(grid) + (CH,))                    # without the keyword: as before
    with pytest.raises(AssertionError, match="logits_upsample goes with logits_shape"):
        _SoftMemory(2, SRC[0], SRC[1], "cpu", logits_upsample=True)


@pytest.mark.parametrize("src,scale,flip", AUGMENTED)
def test_without_the_keyword_the_refusal_stays_and_names_the_option(src, scale, flip):
    mem = _soft_memory(src, GRID)
    assert not mem.logits_upsample and not mem.logits_follow_frames
    states = (_seed(2), _states())[1]
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache .5x9 logits") as e:
        _soft_net(scale, flip)._replay_plan(mem, 3)
    assert "cache the logits at the frame size" in str(e.value) and "logits_upsample=True" in str(e.value)
    assert _states() == states                                         # refused before a random number is drawn
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache"):
        mem.plan(np.array([[[0, src[0], src[1], 0, 0, 1]] * MB], dtype=np.int32), H, 2 * H)
