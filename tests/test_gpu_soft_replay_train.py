"""Soft-teacher fine-tuning on rescaled, cropped and flipped replay batches: ``train_with_deque`` over a DeviceReplayMemory whose teacher
logits are cached at the frame size, with ``scale=[1, 1.5]`` and ``flip=True``, against the same steps made by hand — descriptors from
``draw_samples``, frames and labels through ``memory.gather``, logits through the NumPy restatement of the rule — and against the f64 oracle."""
import random

import numpy as np
import pytest
import torch

from ams_amd import exp_configs, spec as S, weights as Wt
from ams_amd.replay import DeviceReplayMemory, draw_samples
from ams_amd.semantic_network import SemanticNetwork
from test_gpu_replay_logits import resample_batch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, SRC, BATCH, ITERS, SEED = 64, (96, 192), 2, 3, 3
LOSS_REL = 1e-3        # the bar of tests/test_gpu_soft_teacher.py::test_soft_teacher_step_matches_f64_oracle for a 64 x 128 step


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def test_augmented_soft_phase_equals_hand_made_steps():
    from oracle.student_torch import StudentOracle
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    rng = np.random.default_rng(12)
    frames = [rng.integers(0, 256, SRC + (3,), dtype=np.uint8) for _ in range(4)]
    labels = [np.repeat(np.repeat(rng.integers(0, 19, (SRC[0] // 8, SRC[1] // 8), dtype=np.uint8), 8, axis=0), 8, axis=1) for _ in range(4)]
    logits = []
    for l in labels:                                     # noise and a bump on the label's class, as a teacher whose argmax gave the labels
        t = rng.standard_normal(SRC + (19,)).astype(np.float32)
        np.put_along_axis(t, l[..., None].astype(np.int64), np.take_along_axis(t, l[..., None].astype(np.int64), 2) + 3.0, axis=2)
        logits.append(t)
    mem = DeviceReplayMemory(4, SRC[0], SRC[1], DEV, logits_shape=SRC + (19,))
    for f, l, t in zip(frames, labels, logits):
        mem.append(f, l, t)
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1, 1.5], mini_batch_size=BATCH, lr=1e-3, initial_variables=W0,
              soft_teacher=True, flip=True)

    net = SemanticNetwork("unused", **kw)
    _seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    assert len(net.last_losses) == ITERS and all(np.isfinite(net.last_losses))

    _seed(SEED)
    desc = draw_samples(len(mem), SRC, [H, 2 * H], [1, 1.5], BATCH, ITERS, flip=True)
    flat = desc.reshape(-1, 6)
    assert 0 < flat[:, 5].sum() < len(flat)                                               # flipped and unflipped draws
    assert {tuple(d[1:3]) for d in flat} == {(64, 128), (96, 192)}                        # the 1.5x down-scale and the crop of the source
    ref = SemanticNetwork("unused", **kw)
    want_losses, first = [], None
    for it in range(ITERS):
        f_dev, l_dev = mem.gather(desc[it], H, 2 * H)
        tl = resample_batch(logits, desc[it], H, 2 * H)
        if it == 0:
            first = (f_dev.cpu().numpy(), l_dev.cpu().numpy(), tl)
        want_losses.append(ref.train_step(f_dev, l_dev, teacher_logits=tl))
    assert net.last_losses == pytest.approx(want_losses, rel=1e-12)
    a, b = net.get_vars(), ref.get_vars()
    assert sorted(a) == sorted(b) and any("Adam" in k for k in a)
    assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])][:5]
    assert not np.array_equal(a["aspp0/weights:0"], W0["aspp0/weights:0"])

    # step 0 against the f64 oracle's soft loss on that batch
    o = StudentOracle(W0, net.class_indices_graph.tolist(), dtype=torch.float64)
    with torch.no_grad():
        z = o.reduced_logits(o.logits_full(first[0].astype(np.float32), "train"))
        _target, weight = o.label_targets(first[1])
        loss_o = float(o.soft_loss_from_reduced(z, o.soft_targets(first[2], z.shape[1], z.shape[2]), weight))
    assert net.last_losses[0] == pytest.approx(loss_o, rel=LOSS_REL)
    net.close_model()
    ref.close_model()
