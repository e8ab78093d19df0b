"""The replay memory on the device (ams_amd/replay.py, k_replay.hip) through the C ABI: the gather against `utils.mini_batch` bit for bit,
the ring against the host deque, a training phase from the memory against the phase from the deques (bit-identical model, Adam moments and
delta), the phi-score pairs against pair-by-pair `calc_cross_miou`, refused descriptors, and the scheduler with --device_memory."""
import ctypes as C
import filecmp
import glob
import gzip
import os
import random
from collections import deque

import numpy as np
import pytest
import torch

from ams_amd import exp_configs, hip, spec as S, synth, utils, weights as Wt
from ams_amd.replay import DeviceReplayMemory, draw_samples
from ams_amd.semantic_network import SemanticNetwork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CI = [0, 1, 2, 10, 11, 13]


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def _frames(src, n, seed):
    rng = np.random.default_rng(seed)
    return ([rng.integers(0, 256, tuple(src) + (3,), dtype=np.uint8) for _ in range(n)], [rng.integers(0, 19, tuple(src), dtype=np.uint8) for _ in range(n)])


def _fill(frames, labels, capacity=None):
    mem = DeviceReplayMemory(capacity or len(frames), frames[0].shape[0], frames[0].shape[1], DEV)
    for f, l in zip(frames, labels):
        mem.append(f, l)
    return mem


# (source size, crop, scale list, batch, frames in the memory)
GATHER_CASES = {
    "copy_512x1024_b8": ((512, 1024), (512, 1024), [1], 8, 5),
    "copy_crop_of_larger": ((48, 96), (32, 64), [1.5], 6, 3),              # th, tw = the source size: rows copied from a random origin
    "box_2x": ((128, 256), (64, 128), [1], 4, 3),
    "box_and_bilinear": ((64, 128), (32, 64), [1, 1.25, 1.5], 6, 3),
    "ragged_75x150": ((75, 150), (32, 64), [1, 1.25, 1.5], 6, 4),
    "ragged_1208x1920": ((1208, 1920), (512, 1024), [1, 1.25], 4, 2),
    "w_not_multiple_of_4_copy": ((31, 62), (31, 62), [1], 3, 2),
    "w_not_multiple_of_16_bilinear": ((73, 141), (33, 66), [1.1, 1.3], 4, 3),
    "one_slot_twice": ((40, 80), (32, 64), [1, 1.1], 8, 2),
}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("case", sorted(GATHER_CASES))
def test_gather_is_mini_batch_bit_for_bit(case, flip):
    src, crop, scale, batch, n_mem = GATHER_CASES[case]
    frames, labels = _frames(src, n_mem, seed=len(case))
    mem = _fill(frames, labels)
    _seed(3)
    want_img, want_lbl = utils.mini_batch(frames, labels, list(crop), scale, batch, 1, flip=flip)
    _seed(3)
    desc = draw_samples(n_mem, src, list(crop), scale, batch, 1, flip=flip)
    if case == "one_slot_twice":
        assert len(set(desc[0, :, 0].tolist())) < batch
    if flip:
        assert desc[0, :, 5].any()
    got_img, got_lbl = mem.gather(desc[0], crop[0], crop[1])
    assert got_img.dtype == torch.uint8 and tuple(got_img.shape) == (batch,) + tuple(crop) + (3,)
    assert np.array_equal(got_img.cpu().numpy().astype(np.float64), want_img[0])
    assert np.array_equal(got_lbl.cpu().numpy().astype(np.float64), want_lbl[0])


def test_ring_equals_the_host_deque():
    from ams_amd.ingest import FrameIngest
    H, capacity = 64, 4
    ing = FrameIngest(DEV)
    raw_f, raw_l = _frames((90, 170), capacity + 3, seed=2)
    mem, want_f, want_l = DeviceReplayMemory(capacity, H, 2 * H, DEV), deque(maxlen=capacity), deque(maxlen=capacity)
    for k, (f, l) in enumerate(zip(raw_f, raw_l)):
        if k % 2:                                                     # device tensors from the ingest kernel: stored without a host hop
            fd, ld = ing.frame(f, H, 2 * H), ing.label(l, H, 2 * H)
            mem.append(fd, ld)
            want_f.append(fd.cpu().numpy())
            want_l.append(ld.cpu().numpy())
        else:                                                         # host arrays
            fh, lh = utils.resize_linear(f, 2 * H, H), utils.resize_nearest(l, 2 * H, H)
            mem.append(fh, lh)
            want_f.append(fh)
            want_l.append(lh)
        assert len(mem) == len(want_f)
        for i in range(len(mem)):
            assert np.array_equal(mem[i][0].cpu().numpy(), want_f[i]) and np.array_equal(mem[i][1].cpu().numpy(), want_l[i]), (k, i)
    # a batch drawn after the wrap-around reads the same elements
    _seed(9)
    want_img, want_lbl = utils.mini_batch(want_f, want_l, [H, 2 * H], [1], 6, 1)
    _seed(9)
    got_img, got_lbl = mem.gather(draw_samples(len(mem), (H, 2 * H), [H, 2 * H], [1], 6, 1)[0], H, 2 * H)
    assert np.array_equal(got_img.cpu().numpy().astype(np.float64), want_img[0]) and np.array_equal(got_lbl.cpu().numpy().astype(np.float64), want_lbl[0])
    mem.clear()
    assert len(mem) == 0


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


def _teacher_logits(labels, rng, th, tw, nc=19):
    t = rng.standard_normal((labels.shape[0], th, tw, nc)).astype(np.float32)
    ys = np.round(np.linspace(0, labels.shape[1] - 1, th)).astype(int)
    xs = np.round(np.linspace(0, labels.shape[2] - 1, tw)).astype(int)
    low = labels[:, ys][:, :, xs].astype(np.int64)
    bi, yi, xi = np.nonzero(low < nc)
    t[bi, yi, xi, low[low < nc]] += 3.0
    return t


@pytest.mark.parametrize("config", ["full_model", "coord_desc_auto", "coord_desc_auto_device_masks", "soft_teacher_low_res"])
def test_phase_from_the_memory_equals_phase_from_the_deques(W0, config):
    """Equal seeds, scale [1]: the model, the Adam moments and the downlink delta after a phase are the host path's, bit for bit."""
    H, iters = 64, 4
    frames, labels = synth.SyntheticVideo(H, 7, CI, seed=6).clip()
    strategy = "full_model" if config in ("full_model", "soft_teacher_low_res") else "coord_desc_auto"
    soft = config == "soft_teacher_low_res"
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=3, lr=1e-3, initial_variables=W0,
              coord_frac=0.1, device_masks=config.endswith("device_masks"), soft_teacher=soft)
    tl = _teacher_logits(labels, np.random.default_rng(4), 5, 9) if soft else None
    capacity = 5                                                      # seven appends: the ring has wrapped
    mem = DeviceReplayMemory(capacity, H, 2 * H, DEV, logits_shape=(5, 9, 19) if soft else None)
    host_f, host_l, host_t = deque(maxlen=capacity), deque(maxlen=capacity), deque(maxlen=capacity)
    for k in range(len(frames)):
        mem.append(frames[k], labels[k], tl[k] if soft else None)
        host_f.append(frames[k])
        host_l.append(labels[k])
        if soft:
            host_t.append(tl[k])
    host, dev = SemanticNetwork("unused", **kw), SemanticNetwork("unused", **kw)
    import threading
    for phase in range(2):                                            # the second phase starts from the first one's Adam state
        _seed(21 + phase)
        host.train_with_deque(host_f, host_l, iters, strategy, teacher_logits_deque=host_t if soft else None)
        _seed(21 + phase)
        threads = threading.active_count()
        dev.train_with_deque(mem, None, iters, strategy)
        assert threading.active_count() == threads
        assert host.last_losses == dev.last_losses and len(dev.last_losses) == iters
        a, b = host.get_vars(), dev.get_vars()
        assert sorted(a) == sorted(b) and any("Adam" in k for k in a)
        assert all(np.array_equal(a[k], b[k]) for k in a), [k for k in a if not np.array_equal(a[k], b[k])][:5]
        assert host.delta_payload() == dev.delta_payload()
    assert not np.array_equal(host.get_vars()["aspp0/weights:0"], W0["aspp0/weights:0"])
    host.close_model()
    dev.close_model()


def test_flip_is_reachable_on_the_device_path(W0):
    H = 64
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=2).clip()
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=4, lr=1e-3, initial_variables=W0)
    mem = _fill(list(frames), list(labels))
    net = SemanticNetwork("unused", flip=True, **kw)
    _seed(2)
    net.train_with_deque(mem, None, 2)
    # the same draws, built on the host by mini_batch with flip=True and fed as explicit steps
    ref = SemanticNetwork("unused", **kw)
    _seed(2)
    img, lbl = utils.mini_batch(list(frames), list(labels), [H, 2 * H], [1], 4, 2, flip=True)
    for it in range(2):
        ref.train_step(img[it].astype(np.uint8), lbl[it].astype(np.uint8))
    a, b = net.get_vars(), ref.get_vars()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    net.close_model()
    ref.close_model()


def test_cross_miou_pairs_equals_the_loop(W0):
    H = 64
    _f, labels = synth.SyntheticVideo(H, 7, CI, seed=8).clip()
    labels = [np.ascontiguousarray(l) for l in labels]
    labels[3] = np.full_like(labels[3], 255)                          # no valid pixel: pairs (2, 3) and (3, 4) have no common valid pixel
    labels[5] = np.where(labels[4] == 0, 13, 255).astype(np.uint8)
    frames = [np.zeros((H, 2 * H, 3), np.uint8)] * len(labels)
    capacity = 6
    mem, host_l = _fill(frames, labels, capacity), deque(labels, maxlen=capacity)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=2, lr=1e-3,
                          initial_variables=W0)
    for first in (0, 2, len(host_l) - 2):
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = mem.cross_miou_pairs(net, first)
                want = [net.calc_cross_miou(np.array([host_l[k], host_l[k + 1]])) for k in range(first, len(host_l) - 1)]
        assert len(got) == len(want) == len(host_l) - 1 - first
        for g, w in zip(got, want):
            assert g[0].dtype == np.float64 and np.array_equal(g[0], w[0])
            assert np.array_equal(np.asarray(g[1], dtype=np.float64), np.asarray(w[1], dtype=np.float64), equal_nan=True)
            assert np.array_equal(g[2], w[2], equal_nan=True)
    assert any(g[0].sum() == 0 for g in mem.cross_miou_pairs(net, 0)) and any(g[0].sum() > 0 for g in mem.cross_miou_pairs(net, 0))
    assert mem.cross_miou_pairs(net, len(host_l) - 1) == []
    net.close_model()


@pytest.mark.parametrize("bad", ["slot_beyond_capacity", "crop_beyond_the_rescaled_image"])
def test_bad_descriptor_is_refused_before_the_launch(bad):
    lib = hip.lib()
    src, crop, capacity, batch = (48, 96), (32, 64), 3, 2
    mem = _fill(*_frames(src, capacity, seed=1))
    table = np.array([[0, 48, 96, 0, 0, 0], [1, 48, 96, 16, 32, 0]], dtype=np.int32)
    if bad == "slot_beyond_capacity":
        table[1, 0] = capacity
    else:
        table[1, 3] = 48 - 32 + 1                                    # top + H > th
    table_dev = torch.from_numpy(table).to(DEV)
    f_out = torch.full((batch,) + crop + (3,), 7, dtype=torch.uint8, device=DEV)
    l_out = torch.full((batch,) + crop, 7, dtype=torch.uint8, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.ams_replay_gather(C.c_void_p(mem._frames.data_ptr()), mem.frame_stride, C.c_void_p(mem._labels.data_ptr()), mem.label_stride, capacity,
                               src[0], src[1], C.c_void_p(table_dev.data_ptr()), table.ctypes.data_as(C.c_void_p), batch, crop[0], crop[1],
                               C.c_void_p(f_out.data_ptr()), C.c_void_p(l_out.data_ptr()), st)
    assert rc != 0 and b"replay_gather" in lib.ams_last_error()
    torch.cuda.synchronize()
    assert bool((f_out == 7).all()) and bool((l_out == 7).all())
    with pytest.raises((hip.AmsHipError, AssertionError)):
        mem.gather(np.array([[capacity, 48, 96, 0, 0, 0]], dtype=np.int32), crop[0], crop[1])


@pytest.mark.parametrize("strategy", ["coord_desc_auto", "full_model"])
def test_scheduler_with_device_memory_writes_the_same_files(tmp_path, strategy):
    """The tests/test_gpu_scheduler.py configuration with --gpu_ingest --enable_ASR, with and without --device_memory: the same files, byte for
    byte.  Two files carry the wall clock and cannot be: `_train_ms.npy` holds the phases' times (compared by shape), and the header of
    `_mask.dat.gz` holds the time gzip wrote it (compared by size and by the bytes it decompresses to; `_mask.dat` beside it is the same
    payload uncompressed and is compared byte for byte)."""
    from sched_cases import _main
    outs = {}
    for tag, extra in (("host", []), ("dev", ["--device_memory"])):
        out = str(tmp_path / tag) + "/"
        _seed(13)
        summary = _main(None, ["--input_video", "synthetic:25-synth:seconds=8:fps=8", "--student_checkpoint", "synthetic:0", "--output_dir", out,
                               "--gpu", "0", "--mode", "simple", "--height", "256", "--batch_size", "4", "--iter", "3", "--send_period", "1",
                               "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--train_strategy", strategy,
                               "--sampling", "per_second", "--gpu_ingest", "--enable_ASR"] + extra)
        assert summary["frames"] == 64
        outs[tag] = out
    names = sorted(os.path.basename(p) for p in glob.glob(outs["host"] + "*"))
    assert names == sorted(os.path.basename(p) for p in glob.glob(outs["dev"] + "*")) and len(names) > 10
    differ = []
    for name in names:
        a, b = outs["host"] + name, outs["dev"] + name
        if name.endswith("_train_ms.npy"):
            assert np.load(a).shape == np.load(b).shape
        elif name.endswith(".gz"):
            with gzip.open(a, "rb") as fa, gzip.open(b, "rb") as fb:
                same = fa.read() == fb.read() and os.path.getsize(a) == os.path.getsize(b)
            if not same:
                differ.append(name)
        elif not filecmp.cmp(a, b, shallow=False):
            differ.append(name)
    assert differ == [], differ
    ctl = np.load(glob.glob(outs["dev"] + "*_control.npy")[0])
    assert np.isfinite(ctl[:, 1]).any()                               # the phi-score was computed (from the device memory's labels)
