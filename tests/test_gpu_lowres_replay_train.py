"""Soft-teacher fine-tuning from a replay memory whose teacher logits are cached on a small grid (``logits_upsample=True``): a phase on it
equals, loss for loss and bit for bit in every variable, the same phase on a full-size memory whose slots hold the NumPy restatement of the
grid's align-corners upsample (U, tests/teacher_labels_ref.py), with the same seeds.

The whole-frames phase pins the definition: there the small grid goes through the whole-slot entry and the loss kernel's own upsample, so
equality says that the restated U is the loss kernel's interpolation.  The augmented phase (two scales, flips) is the feature."""
import random

import numpy as np
import pytest

from ams_amd import exp_configs, spec as S, weights as Wt
from ams_amd.replay import DeviceReplayMemory, draw_samples
from ams_amd.semantic_network import SemanticNetwork
from teacher_labels_ref import upsample

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, BATCH, ITERS, SLOTS, SEED = 64, 2, 3, 4, 3


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


def _material(src, grid, seed):
    """Frames, blocky labels, and teacher logits on ``grid``: noise and a bump on the class of the label under each cached sample."""
    rng = np.random.default_rng(seed)
    frames = [rng.integers(0, 256, src + (3,), dtype=np.uint8) for _ in range(SLOTS)]
    labels = [np.repeat(np.repeat(rng.integers(0, 19, (src[0] // 8, src[1] // 8), dtype=np.uint8), 8, axis=0), 8, axis=1) for _ in range(SLOTS)]
    ys = np.rint(np.linspace(0, src[0] - 1, grid[0])).astype(np.int64)
    xs = np.rint(np.linspace(0, src[1] - 1, grid[1])).astype(np.int64)
    logits = []
    for l in labels:
        t = rng.standard_normal(grid + (19,)).astype(np.float32)
        cls = l[ys][:, xs][..., None].astype(np.int64)
        np.put_along_axis(t, cls, np.take_along_axis(t, cls, 2) + 3.0, axis=2)
        logits.append(t)
    return frames, labels, logits


def _phase(W0, src, scale, flip, frames, labels, logits, select=False, **memory_kw):
    """One seeded phase on a fresh network and a fresh memory holding ``logits``: (losses, variables)."""
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=scale, mini_batch_size=BATCH, lr=1e-3,
                          initial_variables=W0, soft_teacher=True, flip=flip)
    if select:
        memory_kw["logits_select"] = net.class_indices_graph.tolist()
    mem = DeviceReplayMemory(SLOTS, src[0], src[1], DEV, logits_shape=tuple(logits[0].shape), **memory_kw)
    for f, l, t in zip(frames, labels, logits):
        mem.append(f, l, t)
    _seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    losses, variables = list(net.last_losses), net.get_vars()
    net.close_model()
    return losses, variables, mem


def _assert_same_phase(a, b, W0):
    assert len(a[0]) == ITERS and all(np.isfinite(a[0]))
    assert a[0] == b[0]
    va, vb = a[1], b[1]
    assert sorted(va) == sorted(vb) and any("Adam" in k for k in va)
    assert all(np.array_equal(va[k], vb[k]) for k in va), [k for k in va if not np.array_equal(va[k], vb[k])][:5]
    assert not np.array_equal(va["aspp0/weights:0"], W0["aspp0/weights:0"])


def test_whole_frames_phase_pins_u_to_the_loss_kernels_upsample(W0):
    src, grid = (H, 2 * H), (5, 9)
    frames, labels, logits = _material(src, grid, seed=12)
    low = _phase(W0, src, [1], False, frames, labels, logits, logits_upsample=True)
    assert low[2].logits_cached_shape == grid + (19,) and not low[2].logits_at_source
    full = _phase(W0, src, [1], False, frames, labels, [upsample(t, *src) for t in logits])
    assert full[2].logits_at_source
    _assert_same_phase(low, full, W0)


@pytest.mark.parametrize("select", [False, True], ids=["full_layout", "logits_select"])
def test_augmented_phase_equals_the_phase_on_a_full_size_memory_holding_u(W0, select):
    src, grid, scale = (96, 192), (7, 13), [1, 1.5]
    _seed(SEED)
    flat = draw_samples(SLOTS, src, [H, 2 * H], scale, BATCH, ITERS, flip=True).reshape(-1, 6)
    assert 0 < flat[:, 5].sum() < len(flat)                                               # flipped and unflipped draws
    assert {tuple(d[1:3]) for d in flat} == {(64, 128), (96, 192)}                        # the 1.5x down-scale and the crop of the source
    frames, labels, logits = _material(src, grid, seed=12)
    low = _phase(W0, src, scale, True, frames, labels, logits, select=select, logits_upsample=True)
    assert low[2].logits_cached_shape == grid + ((6 if select else 19),)
    full = _phase(W0, src, scale, True, frames, labels, [upsample(t, *src) for t in logits], select=select)
    assert full[2].logits_at_source and low[2].nbytes < full[2].nbytes
    _assert_same_phase(low, full, W0)
