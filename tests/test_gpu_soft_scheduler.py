"""The soft-teacher path end to end: a fine-tuning phase on a replay memory whose labels were derived from the teacher logits on the device
(``append(frame, None, logits)``) against the same phase on a memory given the NumPy restatement of those labels
(tests/teacher_labels_ref.py), and the scheduler with ``--soft_teacher`` / ``--labels_from_logits`` (ams_amd/run.py).  Height 32 (a 3 x 5
teacher grid), batch 2, one iteration per event, clips of a few seconds, as tests/sched_cases.py."""
import glob
import random

import numpy as np
import pytest

from ams_amd import exp_configs, run as R, spec as S, weights as Wt
from ams_amd.replay import DeviceReplayMemory
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
from ams_amd.synth import SyntheticVideo
from teacher_labels_ref import labels_from_logits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, BATCH, ITERS, SLOTS, SEED = 32, 2, 2, 4, 3


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


# ---------------------------------------------------------------------------------------------------------
# a phase on derived labels
# ---------------------------------------------------------------------------------------------------------
def _phase(W0, src, grid, scale, flip, derive):
    video = SyntheticVideo(src[0], SLOTS, seed=25)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=scale, mini_batch_size=BATCH, lr=1e-3,
                          initial_variables=W0, soft_teacher=True, flip=flip)
    mem = DeviceReplayMemory(SLOTS, src[0], src[1], DEV, logits_shape=grid + (19,), logits_upsample=True,
                             logits_select=net.class_indices_graph.tolist())
    for t in range(SLOTS):
        logits = video.teacher_logits(t, *grid)
        mem.append(video.frame(t)[0], None if derive else labels_from_logits(logits, *src), logits)
    _seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    losses, variables = list(net.last_losses), net.get_vars()
    labels = [mem[i][1].cpu().numpy() for i in range(SLOTS)]
    net.close_model()
    return losses, variables, labels


@pytest.mark.parametrize("src,grid,scale,flip", [((H, 2 * H), (3, 5), [1], False), ((48, 96), (4, 7), [1, 1.5], True)], ids=["whole_frames", "augmented"])
def test_a_phase_on_derived_labels_is_the_phase_on_restated_labels(src, grid, scale, flip):
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    derived, given = _phase(W0, src, grid, scale, flip, True), _phase(W0, src, grid, scale, flip, False)
    assert all(np.array_equal(a, b) for a, b in zip(derived[2], given[2]))
    assert len({int(v) for l in derived[2] for v in np.unique(l)}) > 2                        # the labels are a scene, not one class
    assert len(derived[0]) == ITERS and all(np.isfinite(derived[0])) and derived[0] == given[0]
    va, vb = derived[1], given[1]
    assert sorted(va) == sorted(vb) and any("Adam" in k for k in va)
    assert all(np.array_equal(va[k], vb[k]) for k in va), [k for k in va if not np.array_equal(va[k], vb[k])][:5]
    assert not np.array_equal(va["aspp0/weights:0"], W0["aspp0/weights:0"])


# ---------------------------------------------------------------------------------------------------------
# the scheduler
# ---------------------------------------------------------------------------------------------------------
FILES = ("_fps_client.npy", "_bw_uplink.npy", "_bw_downlink.npy", "_model_update_times.npy", "_train_ms.npy", "_control.npy", "_update.txt",
         "_loss.npy", "_mioucats.npy", "_mious.npy", "_mioumems.npy")
RUNS = {"derived": ["--soft_teacher", "--labels_from_logits"], "gt": ["--soft_teacher"], "hard": []}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The same seeded 8-second clip through the scheduler three times: soft teacher with derived labels, with the source's labels, and the
    hard-label path.  Events at 2, 4, 6 s; four frames uploaded per event into a memory of four."""
    out = {}
    for tag, extra in RUNS.items():
        out[tag] = str(tmp_path_factory.mktemp(tag)) + "/"
        _seed(1)
        summary = R.main(["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", out[tag],
                          "--gpu", "0", "--mode", "simple", "--height", str(H), "--batch_size", str(BATCH), "--iter", "1", "--send_period", "2",
                          "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--device_memory", "--enable_ASR"] + extra)
        assert summary["frames"] == 16
    return out


def _result(out, suffix):
    hits = glob.glob(out + "*_results*" + suffix)
    assert len(hits) == 1, (suffix, hits)
    return hits[0]


def _model(out, second):
    hits = glob.glob(out + "0__8_tp2_f2_%d_*_final.pb" % second)          # run label 0__<length>_tp<train_period>_f<send_period>, then the second
    assert len(hits) == 1, hits
    with open(hits[0], "rb") as f:
        return FrozenGraph.ParseFromString(f.read()).variables


@pytest.mark.parametrize("tag", ["derived", "gt"])
def test_soft_teacher_runs_write_every_file_and_the_soft_evaluation(runs, tag):
    out = runs[tag]
    for suffix in FILES:
        _result(out, suffix)
    times = np.load(_result(out, "_model_update_times.npy"))
    assert times.tolist() == [0.0, 2.0, 4.0, 6.0]
    soft = np.load(_result(out, "_soft_eval.npy"))
    assert soft.shape == (3, 3 + 6) and soft[:, 0].tolist() == [2.0, 4.0, 6.0]                # one row per training event: second, loss, mIoU, 6 IoUs
    assert np.isfinite(soft).all() and (soft[:, 1] > 0).all() and ((soft[:, 2:] >= 0) & (soft[:, 2:] <= 1)).all()
    assert np.allclose(soft[:, 2], soft[:, 3:].mean(axis=1), rtol=0, atol=1e-12)
    ctl = np.load(_result(out, "_control.npy"))
    assert ctl.shape == (3, 5) and np.isfinite(ctl[:, 1]).all() and ((ctl[:, 1] > 0) & (ctl[:, 1] <= 1)).all()          # ASR's phi-score
    assert np.isfinite(np.load(_result(out, "_mious.npy"))).all()


def test_the_hard_label_run_writes_no_soft_evaluation(runs):
    for suffix in FILES:
        _result(runs["hard"], suffix)
    assert glob.glob(runs["hard"] + "*_soft_eval.npy") == []


def test_the_soft_teacher_publishes_another_model(runs):
    first = {tag: _model(out, 0) for tag, out in runs.items()}
    assert all(np.array_equal(first["derived"][k], first["hard"][k]) for k in first["hard"])          # the same initial model
    soft, hard = _model(runs["derived"], 2), _model(runs["hard"], 2)
    assert sorted(soft) == sorted(hard)
    assert any(not np.array_equal(soft[k], hard[k]) for k in soft)
    assert any(not np.array_equal(soft[k], first["derived"][k]) for k in soft)                         # ... and it was trained


def test_derived_labels_are_used_in_place_of_the_sources(runs):
    """The source's labels carry sprinkled ignore pixels and a 255 id the logits cannot produce: the two soft runs see different label slots,
    so their phi-scores differ, while the edge side scores both against the source's labels over the same frames."""
    a, b = np.load(_result(runs["derived"], "_control.npy")), np.load(_result(runs["gt"], "_control.npy"))
    assert not np.array_equal(a[:, 1], b[:, 1])
    assert np.load(_result(runs["derived"], "_mioucats.npy")).shape == np.load(_result(runs["gt"], "_mioucats.npy")).shape
