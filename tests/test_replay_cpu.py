"""Host side of the device replay memory (ams_amd/replay.py) without a GPU: the draws of `draw_samples` against `utils.mini_batch` (same
generator states afterwards, and its descriptors applied with `utils.resize_*` give mini_batch's arrays exactly), the ring against
`collections.deque(maxlen=n)`, the slack asserts, the byte budget, and `train_with_deque(memory, ...)` on the calling thread alone."""
import random
import threading
from collections import deque

import numpy as np
import pytest
import torch

from ams_amd import utils
from ams_amd.replay import DeviceReplayMemory, Ring, draw_samples
from ams_amd.semantic_network import SemanticNetwork

CROP = (32, 64)
SOURCES = {"crop": (32, 64), "double": (64, 128), "ragged": (75, 150)}
SCALES = ([1], [1, 1.25, 1.5], [2])


def apply_descriptors(images, labels, desc, crop):
    """What a descriptor table selects, from the reference arithmetic alone: cv2.resize of the whole frame to (tw, th), the crop, the flip."""
    out_img = np.empty(desc.shape[:2] + (crop[0], crop[1], 3), dtype=np.uint8)
    out_lbl = np.empty(desc.shape[:2] + (crop[0], crop[1]), dtype=np.uint8)
    for it in range(desc.shape[0]):
        for j in range(desc.shape[1]):
            slot, th, tw, top, left, flip = (int(v) for v in desc[it, j])
            img = utils.resize_linear(images[slot], tw, th)[top:top + crop[0], left:left + crop[1], :]
            lbl = utils.resize_nearest(labels[slot], tw, th)[top:top + crop[0], left:left + crop[1]]
            if flip:
                img, lbl = img[:, ::-1, :], lbl[:, ::-1]
            out_img[it, j], out_lbl[it, j] = img, lbl
    return out_img, out_lbl


def _memory(src, n=5, seed=0):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, src + (3,), dtype=np.uint8) for _ in range(n)], [rng.integers(0, 19, src, dtype=np.uint8) for _ in range(n)])


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def _states():
    k, keys, pos, has_gauss, cached = np.random.get_state()
    return random.getstate(), (k, keys.tolist(), pos, has_gauss, cached)


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("scale", SCALES, ids=lambda s: "scale" + "_".join(str(v) for v in s))
@pytest.mark.parametrize("source", sorted(SOURCES))
@pytest.mark.parametrize("seed", [0, 7])
def test_draw_samples_is_mini_batch(seed, source, scale, flip):
    src = SOURCES[source]
    images, labels = _memory(src, seed=seed)
    batch, iters = 3, 4
    _seed(seed)
    want_img, want_lbl = utils.mini_batch(images, labels, list(CROP), scale, batch, iters, flip=flip)
    want_state = _states()
    _seed(seed)
    desc = draw_samples(len(images), src, list(CROP), scale, batch, iters, flip=flip)
    assert _states() == want_state                        # both generators are where mini_batch leaves them
    assert desc.shape == (iters, batch, 6) and desc.dtype == np.int32
    got_img, got_lbl = apply_descriptors(images, labels, desc, CROP)
    assert np.array_equal(got_img.astype(np.float64), want_img)
    assert np.array_equal(got_lbl.astype(np.float64), want_lbl)
    if flip:
        assert 0 < desc[..., 5].sum() < desc[..., 5].size
    else:
        assert not desc[..., 5].any()


@pytest.mark.parametrize("src,scale", [((60, 150), [1]), ((32, 64), [0.5]), ((20, 64), [1])])
def test_slack_asserts_fire_where_mini_batch_s_do(src, scale):
    images, labels = _memory(src, n=2)
    with pytest.raises(AssertionError):
        utils.mini_batch(images, labels, list(CROP), scale, 2, 1)
    with pytest.raises(AssertionError):
        draw_samples(2, src, list(CROP), scale, 2, 1)


@pytest.mark.parametrize("capacity", [1, 3, 4])
def test_ring_is_a_deque_with_maxlen(capacity):
    ring, want = Ring(capacity), deque(maxlen=capacity)
    store = [None] * capacity                             # what the slots hold
    rng = np.random.default_rng(capacity)
    for step in range(60):
        if step in (17, 41):
            ring.clear()
            want.clear()
        else:
            store[ring.push()] = step
            want.append(step)
        assert len(ring) == len(want)
        assert [store[ring.physical(i)] for i in range(len(ring))] == list(want)              # logical 0 is the oldest, eviction in order
        if len(want):
            assert store[ring.physical(-1)] == want[-1]
            picks = rng.integers(0, len(want), 5)
            assert [store[p] for p in ring.physical(picks)] == [want[int(i)] for i in picks]
        with pytest.raises(IndexError):
            ring.physical(len(want))
    with pytest.raises(AssertionError):
        ring.physical(np.array([capacity]))


def test_memory_error_above_max_bytes():
    probe = DeviceReplayMemory(4, 32, 64, "cpu")
    assert probe.nbytes == 4 * (32 * 64 * 3 + 32 * 64)                  # 256-byte multiples already
    with pytest.raises(MemoryError):
        DeviceReplayMemory(4, 32, 64, "cpu", max_bytes=probe.nbytes - 1)
    DeviceReplayMemory(4, 32, 64, "cpu", max_bytes=probe.nbytes)
    soft = DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, 19))
    assert soft.nbytes == probe.nbytes + 4 * 32 * 64 * 19 * 4
    with pytest.raises(MemoryError):
        DeviceReplayMemory(4, 32, 64, "cpu", logits_shape=(32, 64, 19), max_bytes=probe.nbytes)
    ragged = DeviceReplayMemory(2, 5, 7, "cpu")                         # slots start at 256-byte multiples
    assert ragged.frame_stride == 256 and ragged.label_stride == 256 and ragged.nbytes == 1024


def test_memory_bookkeeping_follows_the_deque():
    mem, want_f, want_l = DeviceReplayMemory(3, 8, 16, "cpu"), deque(maxlen=3), deque(maxlen=3)
    frames, labels = _memory((8, 16), n=7)
    labels[2] = labels[2].astype(np.int32) + 300 * (labels[2] > 10)    # ids that no uint8 holds become 255, as in the engine's label rule
    for f, l in zip(frames, labels):
        mem.append(f, l)
        want_f.append(f)
        want_l.append(np.where(l < 255, l, 255).astype(np.uint8))
        assert len(mem) == len(want_f)
        for i in range(len(mem)):
            assert np.array_equal(mem[i][0].numpy(), want_f[i]) and np.array_equal(mem[i][1].numpy(), want_l[i])
    with pytest.raises(AssertionError):
        mem.append(np.zeros((8, 15, 3), np.uint8), labels[0])          # one source geometry per memory
    mem.clear()
    assert len(mem) == 0


# ---- train_with_deque(memory, ...) over stand-ins for the device touch points, in the style of tests/test_train_threads_cpu.py ----
H, MB = 8, 2


class _Spec:
    trainable = []


class _Engine:
    device = "cpu"
    spec = _Spec()

    def __init__(self):
        self.seen, self.threads = [], []

    def train_step(self, frames, labels, lr, mask):
        self.threads.append(threading.active_count())
        self.seen.append((frames.numpy().copy(), labels.numpy().copy()))
        return torch.tensor([float(len(self.seen)), 1.0], dtype=torch.float64)


class _Net(SemanticNetwork):
    def __init__(self, scale):
        self.process_lock = threading.Lock()
        self.height, self.mini_batch_size, self.scale, self.lr = H, MB, scale, 1e-3
        self.frozen, self.mask, self.verbose, self.coord_frac = False, None, False, 0.1
        self.device_masks = self.soft_teacher = self.flip = False
        self.engine = _Engine()
        self._held = None
        self.train_params = self.curr_mask = None
        self.last_losses = []

    def _model_vars(self):
        return {}


class _HostMemory(DeviceReplayMemory):
    """The memory's bookkeeping as it is; the one launch replaced by the reference arithmetic on the slots."""

    def _gather(self, samples_host, samples_dev, h, w, frames_out, labels_out):
        assert np.array_equal(samples_dev.numpy(), samples_host)
        images = {p: self._slot_views(p)[0].numpy() for p in range(self.capacity)}
        labels = {p: self._slot_views(p)[1].numpy() for p in range(self.capacity)}
        img, lbl = apply_descriptors(images, labels, samples_host[None], (h, w))
        frames_out.copy_(torch.from_numpy(img[0]))
        labels_out.copy_(torch.from_numpy(lbl[0]))


@pytest.mark.parametrize("scale", [[1], [1, 1.5]])
def test_train_with_memory_starts_no_thread(scale):
    frames, labels = _memory((16, 32), n=6, seed=3)
    mem = _HostMemory(4, 16, 32, "cpu")                    # six appends into four slots: the ring has wrapped
    for f, l in zip(frames, labels):
        mem.append(f, l)
    net = _Net(scale)
    before = threading.active_count()
    _seed(5)
    net.train_with_deque(mem, None, 7)
    assert threading.active_count() == before
    assert net.engine.threads == [before] * 7              # nor was one alive while the steps ran
    assert net.process_lock.acquire(False)
    net.process_lock.release()
    assert net.last_losses == [float(i + 1) for i in range(7)]
    _seed(5)
    want_img, want_lbl = utils.mini_batch(frames[2:], labels[2:], [H, 2 * H], scale, MB, 7)
    for it, (f, l) in enumerate(net.engine.seen):
        assert np.array_equal(f.astype(np.float64), want_img[it]) and np.array_equal(l.astype(np.float64), want_lbl[it])


def test_train_with_memory_refuses_deque_arguments():
    mem = _HostMemory(2, H, 2 * H, "cpu")
    mem.append(*[a[0] for a in _memory((H, 2 * H), n=1)])
    net = _Net([1])
    with pytest.raises(AssertionError):
        net.train_with_deque(mem, deque(), 1)
    assert net.process_lock.acquire(False)
    net.process_lock.release()
