"""Host side of the selected layout of cached teacher logits (a replay memory that keeps only the student's K channels), without a GPU:
the byte budget, the shapes ``append`` and the explicit-array calls accept, what reaches the library, and the refusal of a memory that
selected another network's classes.  The device touch points are the stand-ins of tests/test_replay_cpu.py and
tests/test_replay_logits_cpu.py; the library is that file's recorder."""
import numpy as np
import pytest
import torch

from ams_amd import hip, replay
from ams_amd.engine import StudentEngine
from ams_amd.replay import SLOT_ALIGN, DeviceReplayMemory
from test_replay_cpu import H, MB, _memory, _seed
from test_replay_logits_cpu import _Recorder, _SoftEngine, _SoftMemory, _soft_net

CH = 19
IDX = [0, 1, 2, 10, 11, 13]
K = len(IDX)


class _LayoutEngine(_SoftEngine):
    """The stand-in engine, also recording the layout a step names (None: not named, the engine goes by the last dimension)."""

    def train_step(self, frames, labels, lr, mask, teacher_logits=None, teacher_logits_layout=None):
        self.layouts_seen = getattr(self, "layouts_seen", []) + [teacher_logits_layout]
        return super().train_step(frames, labels, lr, mask, teacher_logits=teacher_logits)


def _net(scale, flip=False, idx=IDX):
    net = _soft_net(scale, flip)
    net.engine = _LayoutEngine()
    net.class_indices_graph = np.asarray(idx)
    net.class_count, net.TOTAL_CLASSES = len(idx), CH
    return net


def _logits(shape, seed=0):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def _stride(n_floats):
    return (4 * n_floats + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN // 4


@pytest.fixture
def lib(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(replay.hip, "lib", lambda: rec)
    return rec


def test_byte_budget_follows_k():
    full = DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, CH))
    sel = DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, CH), logits_select=IDX)
    assert (full.logits_layout, sel.logits_layout) == ("full", "selected")
    assert full.logits_shape == sel.logits_shape == (32, 64, CH)                   # what the caller feeds
    assert full.logits_cached_shape == (32, 64, CH) and sel.logits_cached_shape == (32, 64, K)
    assert full.logits_select is None and sel.logits_select == tuple(IDX)
    assert sel.logits_stride == _stride(32 * 64 * K) and full.logits_stride == _stride(32 * 64 * CH)
    assert full.nbytes - sel.nbytes == 4 * (full.logits_stride - sel.logits_stride) * 4
    assert sel.nbytes == 4 * (32 * 64 * 3 + 32 * 64 + 4 * 32 * 64 * K)
    ragged = DeviceReplayMemory(2, 5, 7, "cpu", logits_shape=(5, 7, CH), logits_select=[0, 5, 18])
    assert ragged.logits_stride == 128 and ragged.logits_stride * 4 % SLOT_ALIGN == 0      # 105 floats -> 512 bytes
    # MemoryError before anything is allocated: the budget that holds the selected memory refuses the full one
    DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, CH), logits_select=IDX, max_bytes=sel.nbytes)
    with pytest.raises(MemoryError):
        DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, CH), logits_select=IDX, max_bytes=sel.nbytes - 1)
    with pytest.raises(MemoryError):
        DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, CH), max_bytes=sel.nbytes)
    with pytest.raises(MemoryError):          # (a budget no host could allocate: raised from the arithmetic alone)
        DeviceReplayMemory(10 ** 9, 512, 1024, "cpu", logits_shape=(512, 1024, CH), logits_select=IDX, max_bytes=1 << 40)


def test_select_list_is_checked():
    with pytest.raises(AssertionError, match="goes with logits_shape"):
        DeviceReplayMemory(2, 8, 16, "cpu", logits_select=IDX)
    with pytest.raises(AssertionError, match="outside 0..18"):
        DeviceReplayMemory(2, 8, 16, "cpu", logits_shape=(8, 16, CH), logits_select=[0, 19])
    with pytest.raises(AssertionError, match="1..32 classes"):
        DeviceReplayMemory(2, 8, 16, "cpu", logits_shape=(8, 16, CH), logits_select=[])
    with pytest.raises(AssertionError, match="1..32 classes"):
        DeviceReplayMemory(2, 8, 16, "cpu", logits_shape=(8, 16, 40), logits_select=list(range(33)))


def test_append_host_selection_is_np_take_and_reduced_logits_are_kept():
    frames, labels = _memory((8, 16), n=3, seed=2)
    mem = DeviceReplayMemory(3, 8, 16, "cpu", logits_shape=(8, 16, CH), logits_select=IDX)
    full = [_logits((8, 16, CH), seed=s) for s in range(3)]
    full[1][0, 0, :4] = (np.inf, -np.inf, np.nan, 1e-42)                           # copies: every bit pattern survives
    mem.append(frames[0], labels[0], full[0])                                       # a full NumPy array
    mem.append(frames[1], labels[1], torch.from_numpy(full[1]))                     # a full host tensor
    mem.append(frames[2], labels[2], np.take(full[2], IDX, axis=-1))                # already reduced
    for i in range(3):
        got = mem[i][2]
        assert tuple(got.shape) == (8, 16, K) and got.dtype == torch.float32
        assert np.array_equal(got.numpy().view(np.uint32), np.take(full[i], IDX, axis=-1).view(np.uint32))
    f64 = _logits((8, 16, CH), seed=9).astype(np.float64)
    mem.append(frames[0], labels[0], f64)                                           # evicts the oldest; cast to f32 as the full layout does
    assert np.array_equal(mem[2][2].numpy(), np.take(f64.astype(np.float32), IDX, axis=-1))


def test_append_shape_rule_names_both_shapes():
    frames, labels = _memory((8, 16), n=1)
    mem = DeviceReplayMemory(2, 8, 16, "cpu", logits_shape=(8, 16, CH), logits_select=IDX)
    for bad in ((8, 16, 5), (8, 16, CH + 1), (16, 8, K), (8, 16)):
        with pytest.raises(AssertionError) as e:
            mem.append(frames[0], labels[0], np.zeros(bad, np.float32))
        assert "(8, 16, 19)" in str(e.value) and "(8, 16, 6)" in str(e.value) and str(bad) in str(e.value)
    assert len(mem) == 0                                                            # refused before a slot is taken
    plain = DeviceReplayMemory(2, 8, 16, "cpu", logits_shape=(8, 16, CH))          # the full layout keeps its one shape
    with pytest.raises(AssertionError, match=r"teacher logits must be \(8, 16, 19\), got \(8, 16, 6\)"):
        plain.append(frames[0], labels[0], np.zeros((8, 16, K), np.float32))
    with pytest.raises(AssertionError, match="required then"):
        mem.append(frames[0], labels[0])


def test_k_equal_to_num_classes_means_full():
    """Every class selected, in another order: the two shapes coincide, the array is full logits and is permuted like any other."""
    perm = [3, 0, 2, 1]
    frames, labels = _memory((8, 16), n=1)
    mem = DeviceReplayMemory(1, 8, 16, "cpu", logits_shape=(8, 16, 4), logits_select=perm)
    assert mem.logits_cached_shape == (8, 16, 4) and mem.logits_layout == "selected"
    assert mem.nbytes == DeviceReplayMemory(1, 8, 16, "cpu", logits_shape=(8, 16, 4)).nbytes
    t = _logits((8, 16, 4))
    mem.append(frames[0], labels[0], t)
    assert np.array_equal(mem[0][2].numpy(), np.take(t, perm, axis=-1))
    net = _net([1], idx=perm)
    net.TOTAL_CLASSES = 4
    assert net._logits_layout(np.zeros((MB, H, 2 * H, 4), np.float32), MB) == "full"


class _DeviceTensor(torch.Tensor):
    """A host tensor that answers as one on the device: what ``append`` asks before it chooses the pack kernel."""
    is_cuda = property(lambda self: True)


def test_device_tensor_goes_through_the_pack_entry(lib):
    frames, labels = _memory((8, 16), n=1)
    mem = _SoftMemory(2, 8, 16, "cpu", logits_shape=(8, 16, CH), logits_select=IDX)
    t = torch.from_numpy(_logits((8, 16, CH)))
    mem.append(frames[0], labels[0], t.as_subclass(_DeviceTensor))
    (name, args), = lib.calls
    assert name == "ams_replay_pack_logits"
    assert args[1:4] == (8, 16, CH) and list(args[4]) == IDX and args[5:7] == (K, hip.TLOGITS_SELECTED)
    assert args[0].value == t.data_ptr() and args[7].value == mem[0][2].data_ptr()


def test_phases_on_a_selected_memory_gather_k_channels(lib):
    src = (2 * H, 4 * H)
    frames, labels = _memory(src, n=4, seed=1)
    mem = _SoftMemory(4, src[0], src[1], "cpu", logits_shape=src + (CH,), logits_select=IDX)
    for f, l in zip(frames, labels):
        mem.append(f, l, np.zeros(src + (CH,), np.float32))
    net = _net([1, 1.5], flip=True)
    _seed(5)
    net.train_with_deque(mem, None, 4)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_logits"] * 4
    for _, args in lib.calls:
        assert args[1:6] == (mem.logits_stride, mem.capacity, src[0], src[1], K) and args[8:11] == (MB, H, 2 * H)
    assert net.engine.logits_seen == [(MB, H, 2 * H, K)] * 4 and net.engine.layouts_seen == ["selected"] * 4
    # a selected low-resolution cache follows whole frames through the whole-slot entry at K channels, and keeps the whole-frames-only rule
    lib.calls.clear()
    low = _SoftMemory(4, H, 2 * H, "cpu", logits_shape=(5, 9, CH), logits_select=IDX)
    for f, l in zip(*_memory((H, 2 * H), n=4, seed=1)):
        low.append(f, l, np.zeros((5, 9, K), np.float32))
    net = _net([1])
    _seed(5)
    net.train_with_deque(low, None, 2)
    assert [name for name, _ in lib.calls] == ["ams_replay_gather_f32"] * 2
    assert [args[3:6] for _, args in lib.calls] == [(5, 9, K)] * 2
    assert net.engine.logits_seen == [(MB, 5, 9, K)] * 2
    with pytest.raises(AssertionError, match="low-resolution teacher-logit cache .5x9 logits"):
        _net([1], flip=True)._replay_plan(low, 2)


def test_memory_of_another_class_list_is_refused_with_both_lists(lib):
    other = [0, 1, 2, 10, 11, 12]
    mem = _SoftMemory(2, H, 2 * H, "cpu", logits_shape=(H, 2 * H, CH), logits_select=other)
    for f, l in zip(*_memory((H, 2 * H), n=2)):
        mem.append(f, l, np.zeros((H, 2 * H, CH), np.float32))
    net = _net([1])
    for call in (lambda: net.train_with_deque(mem, None, 1), lambda: net.evaluate_memory(mem)):
        with pytest.raises(AssertionError) as e:
            call()
        assert str(other) in str(e.value) and str(IDX) in str(e.value)
    assert lib.calls == [] and not hasattr(net.engine, "logits_seen")              # before anything is launched
    assert net.process_lock.acquire(False)
    net.process_lock.release()
    # the same classes in another order are other channels too
    swapped = _SoftMemory(2, H, 2 * H, "cpu", logits_shape=(H, 2 * H, CH), logits_select=IDX[::-1])
    with pytest.raises(AssertionError, match="class index list"):
        net._memory_layout(swapped)
    assert net._memory_layout(_SoftMemory(2, H, 2 * H, "cpu", logits_shape=(H, 2 * H, CH), logits_select=IDX)) == "selected"
    assert net._memory_layout(_SoftMemory(2, H, 2 * H, "cpu", logits_shape=(H, 2 * H, CH))) == "full"


class _FeedEngine:
    """``StudentEngine``'s own shape rule over a recorder in place of the library."""
    soft_teacher, num_classes, K, height, width, device = True, CH, K, H, 2 * H, "cpu"
    teacher_logits_layout = StudentEngine.teacher_logits_layout
    _feed_teacher_logits = StudentEngine._feed_teacher_logits

    def __init__(self):
        self.lib, self._h = _Recorder(), None


def test_explicit_arrays_are_told_apart_by_the_last_dimension():
    eng = _FeedEngine()
    eng._feed_teacher_logits(np.zeros((MB, H, 2 * H, CH), np.float32), MB)
    eng._feed_teacher_logits(np.zeros((MB, 5, 9, K), np.float32), MB)
    assert [(n, a[2:]) for n, a in eng.lib.calls] == [("ams_student_feed_teacher_logits_layout", (H, 2 * H, hip.TLOGITS_FULL)),
                                                       ("ams_student_feed_teacher_logits_layout", (5, 9, hip.TLOGITS_SELECTED))]
    with pytest.raises(AssertionError, match="19.*full.*6.*selected.*got 7 channels"):
        eng._feed_teacher_logits(np.zeros((MB, H, 2 * H, 7), np.float32), MB)
    with pytest.raises(AssertionError, match="selected layout must be .*6\\], got 19"):
        eng._feed_teacher_logits(np.zeros((MB, H, 2 * H, CH), np.float32), MB, "selected")
    with pytest.raises(AssertionError, match="'full' or 'selected'"):
        eng.teacher_logits_layout(CH, "packed")
    assert len(eng.lib.calls) == 2
    # SemanticNetwork.train_step: the same rule, before the engine is reached
    net = _net([1])
    frames, labels = torch.zeros((MB, H, 2 * H, 3), dtype=torch.uint8), torch.zeros((MB, H, 2 * H), dtype=torch.uint8)
    net.train_step(frames, labels, teacher_logits=np.zeros((MB, H, 2 * H, K), np.float32))
    net.train_step(frames, labels, teacher_logits=np.zeros((MB, 5, 9, CH), np.float32))
    assert net.engine.layouts_seen == ["selected", "full"]
    with pytest.raises(AssertionError, match=r"\[2, th, tw, 19\].*\[2, th, tw, 6\].*got \(2, 8, 16, 7\)"):
        net.train_step(frames, labels, teacher_logits=np.zeros((MB, H, 2 * H, 7), np.float32))
    assert len(net.engine.layouts_seen) == 2
