"""Host side of soft-teacher training on rescaled, cropped and flipped replay batches, without a GPU: what ``_replay_plan`` accepts and
refuses, the shape of the plan's logits buffer, which entry of the library a phase reaches, and that teacher logits in the memory change
nothing about the draws.  The device touch points are the stand-ins of tests/test_replay_cpu.py; the library is a recorder."""
import numpy as np
import pytest

from ams_amd import replay
from test_replay_cpu import H, MB, _Engine, _HostMemory, _Net, _memory, _seed, _states

CH = 19
SRC = (2 * H, 4 * H)                                      # frames twice the network's size: every draw is a crop


class _Recorder:
    """libams_hip.so as far as the logits of a phase go: every entry answers AMS_OK and is counted."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class _SoftEngine(_Engine):
    def train_step(self, frames, labels, lr, mask, teacher_logits=None):
        self.logits_seen = getattr(self, "logits_seen", []) + [tuple(teacher_logits.shape)]
        return super().train_step(frames, labels, lr, mask)


class _SoftMemory(_HostMemory):
    def _stream(self):
        return None


def _soft_net(scale, flip=False):
    net = _Net(scale)
    net.soft_teacher, net.flip, net.engine = True, flip, _SoftEngine()
    return net


def _soft_memory(src, logits_hw, n=4):
    mem = _SoftMemory(n, src[0], src[1], "cpu", logits_shape=tuple(logits_hw) + (CH,))
    frames, labels = _memory(src, n=n, seed=1)
    for f, l in zip(frames, labels):
        mem.append(f, l, np.zeros(tuple(logits_hw) + (CH,), np.float32))
    return mem


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(replay.hip, "lib", lambda: rec)
    return rec


@pytest.mark.parametrize("scale,flip", [([1, 1.5], False), ([1], True), ([1, 1.5], True)])
def test_replay_plan_accepts_source_size_logits(scale, flip):
    mem = _soft_memory(SRC, SRC)
    _seed(1)
    plan = _soft_net(scale, flip)._replay_plan(mem, 5)
    assert not plan.whole_frames
    assert tuple(plan.logits.shape) == (MB, H, 2 * H, CH)             # the label size: what the soft loss kernel reads as it is
    if flip:
        assert plan.table_host[..., 5].any()


@pytest.mark.parametrize("src,scale,flip", [((H, 2 * H), [1, 1.5], False), (SRC, [1], False), ((H, 2 * H), [1], True)])
def test_replay_plan_refuses_a_low_resolution_cache_that_would_be_resampled(src, scale, flip):
    mem = _soft_memory(src, (5, 9))
    states = (_seed(2), _states())[1]
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache .5x9 logits") as e:
        _soft_net(scale, flip)._replay_plan(mem, 3)
    assert "cache the logits at the frame size" in str(e.value)       # what to do about it
    assert _states() == states                                         # refused before a random number is drawn
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache"):           # the memory's own surface refuses it too
        mem.plan(np.array([[[0, src[0], src[1], 0, 0, 1]] * MB], dtype=np.int32), H, 2 * H)


def test_logits_buffer_keeps_the_cached_grid_for_whole_frames():
    for logits_hw in ((5, 9), (H, 2 * H)):
        mem = _soft_memory((H, 2 * H), logits_hw)
        _seed(3)
        plan = _soft_net([1])._replay_plan(mem, 2)
        assert plan.whole_frames and tuple(plan.logits.shape) == (MB,) + tuple(logits_hw) + (CH,)
    mem = _soft_memory((H, 2 * H), (H, 2 * H))                          # a cache at the frame size has the label size either way
    _seed(3)
    assert tuple(_soft_net([1.5])._replay_plan(mem, 2).logits.shape) == (MB, H, 2 * H, CH)
    assert tuple(_soft_net([1])._replay_plan(mem, 2).logits.shape) == (MB, H, 2 * H, CH)


@pytest.mark.parametrize("logits_hw", [(5, 9), (H, 2 * H)])
def test_whole_frame_phases_reach_the_whole_slot_entry_only(lib, logits_hw):
    mem = _soft_memory((H, 2 * H), logits_hw)
    net = _soft_net([1])
    _seed(4)
    net.train_with_deque(mem, None, 3)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_f32"] * 3
    assert [args[3:6] for _, args in lib.calls] == [tuple(logits_hw) + (CH,)] * 3              # th, tw, channels: the cached grid
    assert net.engine.logits_seen == [(MB,) + tuple(logits_hw) + (CH,)] * 3


@pytest.mark.parametrize("src,scale,flip", [(SRC, [1], False), ((H, 2 * H), [1, 1.5], False), ((H, 2 * H), [1], True)])
def test_augmented_phases_reach_the_resampling_entry_only(lib, src, scale, flip):
    mem = _soft_memory(src, src)
    net = _soft_net(scale, flip)
    _seed(5)
    net.train_with_deque(mem, None, 6)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_logits"] * 6
    for _, args in lib.calls:
        assert args[1:6] == (mem.logits_stride, mem.capacity, src[0], src[1], CH) and args[8:11] == (MB, H, 2 * H)
    assert net.engine.logits_seen == [(MB, H, 2 * H, CH)] * 6                                  # fed with th, tw = H, W


@pytest.mark.parametrize("flip", [False, True])
def test_logits_in_the_memory_do_not_change_the_draws(flip):
    tables, states = [], []
    for soft in (False, True):
        if soft:
            mem, net = _soft_memory(SRC, SRC), _soft_net([1, 1.5], flip)
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
