"""The selected layout of cached teacher logits (AMS_TLOGITS_SELECTED: a replay slot keeps the student's K channels alone) against the full
layout, through the C ABI and end to end.  Every stored value is a copy of an input value and every later operation is per channel, so
each bar here is equality of bit patterns: the pack kernel against ``np.take``, the gathers at K channels against ``np.take`` of the
gathers at every channel, the loss and the metric kernels on packed logits against themselves on full logits, and a training phase on
a selected memory against the same phase on a full one."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from ams_amd import exp_configs, hip, spec as S, weights as Wt
from ams_amd.replay import DeviceReplayMemory
from ams_amd.semantic_network import SemanticNetwork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)
FULL, SELECTED = hip.TLOGITS_FULL, hip.TLOGITS_SELECTED
CI6 = [0, 1, 2, 10, 11, 13]
POISON = 0x7FC12345               # a NaN pattern no kernel here produces


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def table(idx):
    return (C.c_int32 * max(1, len(idx)))(*idx)


def bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def poisoned(shape):
    return torch.full(tuple(shape), POISON, dtype=torch.int32, device=DEV).view(torch.float32)


@pytest.fixture(scope="module")
def lib():
    return hip.lib()


def _special(rng, shape):
    """Normal draws salted with both infinities, NaN patterns (quiet, signalling, with payloads), subnormals and both zeros."""
    t = (rng.standard_normal(shape) * 3).astype(np.float32)
    u = t.view(np.uint32).reshape(-1)
    salt = np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FABCDEF, 0x00000001, 0x807FFFFF, 0x00000000, 0x80000000],
                    dtype=np.uint32)
    where = rng.choice(u.size, size=min(u.size, 40 * salt.size), replace=False)
    u[where] = np.resize(salt, where.size)
    return t


def _pack(lib, t_dev, idx, layout=SELECTED, out=None):
    th, tw, nc = t_dev.shape
    out = poisoned((th, tw, len(idx))) if out is None else out
    rc = lib.ams_replay_pack_logits(P(t_dev), th, tw, nc, table(idx), len(idx), layout, P(out), stream())
    return rc, out


# ---------------------------------------------------------------------------------------------------------
# 1. the pack kernel
# ---------------------------------------------------------------------------------------------------------
PACK_CASES = [((5, 7, 19), [0]), ((5, 7, 19), [0, 5, 18]), ((5, 7, 19), CI6),
              ((16, 32, 19), [1, 4, 9, 16]), ((16, 32, 19), [0, 2, 4, 6, 8, 10, 12, 18]),          # tw * K a multiple of 4: 16-byte stores
              ((16, 32, 19), list(range(19))), ((3, 130, 21), [20, 0, 7, 3, 15])]                  # a row longer than one block's run


@pytest.mark.parametrize("offset", [0, 1])            # 1: the input starts one float behind a 16-byte boundary (per-element loads)
@pytest.mark.parametrize("shape,idx", PACK_CASES)
def test_pack_is_np_take(lib, shape, idx, offset):
    rng = np.random.default_rng(sum(shape) + len(idx))
    t = _special(rng, shape)
    n = int(np.prod(shape))
    buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    view = buf[offset:offset + n].view(shape)
    view.copy_(torch.from_numpy(t))
    assert view.data_ptr() % 16 == 4 * offset
    rc, out = _pack(lib, view, idx)
    hip.check(rc, "ams_replay_pack_logits")
    assert np.array_equal(bits(out), np.take(t, idx, axis=-1).view(np.uint32))
    assert np.array_equal(bits(view), t.view(np.uint32))                               # the input is read only


def test_pack_into_an_unaligned_slot_and_the_full_layout(lib):
    rng = np.random.default_rng(3)
    t = _special(rng, (16, 32, 19))
    td = torch.from_numpy(t).to(DEV)
    idx = [1, 4, 9, 16]
    buf = poisoned((16 * 32 * 4 + 8,))
    out = buf[1:1 + 16 * 32 * 4].view(16, 32, 4)                                       # per-element stores; the floats around stay
    hip.check(lib.ams_replay_pack_logits(P(td), 16, 32, 19, table(idx), 4, SELECTED, P(out), stream()))
    assert np.array_equal(bits(out), np.take(t, idx, axis=-1).view(np.uint32))
    assert bits(buf)[0] == POISON and (bits(buf)[1 + 16 * 32 * 4:] == POISON).all()
    rc, whole = _pack(lib, td, list(range(19)), layout=FULL)                           # a full slot is the input itself
    hip.check(rc)
    assert np.array_equal(bits(whole), t.view(np.uint32))


def test_pack_refusals_write_nothing(lib):
    td = torch.zeros((5, 7, 19), device=DEV)
    out = poisoned((5, 7, 33))
    calls = {"K = 0": ([], SELECTED), "K = 33": (list(range(19)) + list(range(14)), SELECTED), "index >= NC": ([0, 19], SELECTED),
             "negative index": ([3, -1], SELECTED), "unknown layout": (CI6, 2), "negative layout": (CI6, -1)}
    for what, (idx, layout) in calls.items():
        rc = lib.ams_replay_pack_logits(P(td), 5, 7, 19, table(idx), len(idx), layout, P(out), stream())
        assert rc == E_INVALID and lib.ams_last_error(), what
    assert lib.ams_replay_pack_logits(P(td), 5, 7, 19, None, 6, SELECTED, P(out), stream()) == E_INVALID          # a NULL table
    assert lib.ams_replay_pack_logits(None, 5, 7, 19, table(CI6), 6, SELECTED, P(out), stream()) == E_INVALID
    torch.cuda.synchronize()
    assert (bits(out) == POISON).all()


# ---------------------------------------------------------------------------------------------------------
# 2. the gathers at K channels
# ---------------------------------------------------------------------------------------------------------
def _stride(n):
    return (n + 63) // 64 * 64            # slots start at 256-byte multiples (replay.SLOT_ALIGN)


def _ring(lib, slots, idx=None):
    """A ring of the slots' logits (idx None) or of their packed twins, packed by the kernel: (device buffer, stride in floats)."""
    th, tw, nc = slots[0].shape
    ch = nc if idx is None else len(idx)
    stride = _stride(th * tw * ch)
    ring = poisoned((len(slots) * stride,))
    for p, t in enumerate(slots):
        view = ring[p * stride:p * stride + th * tw * ch].view(th, tw, ch)
        if idx is None:
            view.copy_(torch.from_numpy(t))
        else:
            hip.check(lib.ams_replay_pack_logits(P(torch.from_numpy(t).to(DEV)), th, tw, nc, table(idx), ch, SELECTED, P(view), stream()))
    return ring, stride


def _gather_logits(lib, ring, stride, n_slots, src, ch, desc, crop):
    desc = np.ascontiguousarray(desc, dtype=np.int32)
    out = poisoned((len(desc),) + tuple(crop) + (ch,))
    hip.check(lib.ams_replay_gather_logits(P(ring), stride, n_slots, src[0], src[1], ch, P(torch.from_numpy(desc).to(DEV)),
                                           desc.ctypes.data_as(C.c_void_p), len(desc), crop[0], crop[1], P(out), stream()), "ams_replay_gather_logits")
    return bits(out)


CROP = (16, 32)
# batches of four descriptors (slot, th, tw, top, left, flip) over slots of 24 x 40: the copy with an even and an odd left, the rescaled
# image 1.5 and 1.25 times the slot, each mirrored and not
COPY = [[0, 24, 40, 2, 4, 0], [1, 24, 40, 8, 4, 1], [2, 24, 40, 5, 3, 0], [1, 24, 40, 0, 7, 1]]
UP = [[0, 36, 60, 20, 28, 0], [2, 36, 60, 0, 0, 1], [1, 30, 50, 14, 18, 0], [2, 30, 50, 7, 9, 1]]
# an exact 2x down-scale that still holds a 16 x 32 crop needs slots of 32 x 64: a second ring, the same crop and batch
HALF = [[0, 16, 32, 0, 0, 0], [1, 16, 32, 0, 0, 1], [2, 16, 32, 0, 0, 0], [0, 16, 32, 0, 0, 1]]


@pytest.fixture(scope="module")
def rings(lib):
    rng = np.random.default_rng(24)
    small = [_special(rng, (24, 40, 19)) for _ in range(3)]
    large = [_special(rng, (32, 64, 19)) for _ in range(3)]
    full = {}
    for name, slots, batches in (("small", small, (COPY, UP)), ("large", large, (HALF,))):
        ring, stride = _ring(lib, slots)
        src = slots[0].shape[:2]
        full[name] = (slots, src, [(d, _gather_logits(lib, ring, stride, 3, src, 19, d, CROP).view(np.float32)) for d in batches])
    return full                       # the full ring's results, computed once


@pytest.mark.parametrize("idx", [[0, 5, 18], [1, 4, 9, 16], CI6, [0, 2, 4, 6, 8, 10, 12, 18]], ids=["K3", "K4", "K6", "K8"])
def test_gather_logits_on_the_packed_ring_is_take_of_the_full_ring(lib, rings, idx):
    with np.errstate(all="ignore"):
        for name in ("small", "large"):
            slots, src, batches = rings[name]
            ring, stride = _ring(lib, slots, idx)
            for desc, want_full in batches:
                got = _gather_logits(lib, ring, stride, 3, src, len(idx), desc, CROP)
                want = np.ascontiguousarray(np.take(want_full, idx, axis=-1)).view(np.uint32)
                assert got.shape == want.shape == (4,) + CROP + (len(idx),)
                assert np.array_equal(got, want), (name, desc, int((got != want).sum()))


def test_gather_logits_at_every_channel_count(lib):
    """channels = K for every K in 1..32, over slots of 40 classes: a copy (odd left), its mirror and an up-scale per K."""
    rng = np.random.default_rng(32)
    slots = [_special(rng, (9, 20, 40)) for _ in range(2)]
    desc = [[0, 9, 20, 1, 3, 0], [1, 9, 20, 2, 5, 1], [1, 13, 29, 4, 11, 0], [0, 13, 29, 0, 0, 1]]
    ring, stride = _ring(lib, slots)
    with np.errstate(all="ignore"):
        want_full = _gather_logits(lib, ring, stride, 2, (9, 20), 40, desc, (6, 12)).view(np.float32)
        for K in range(1, 33):
            idx = [int(c) for c in rng.choice(40, size=K, replace=False)]
            packed, pstride = _ring(lib, slots, idx)
            got = _gather_logits(lib, packed, pstride, 2, (9, 20), K, desc, (6, 12))
            assert np.array_equal(got, np.ascontiguousarray(np.take(want_full, idx, axis=-1)).view(np.uint32)), K


@pytest.mark.parametrize("idx", [[0, 5, 18], [1, 4, 9, 16], CI6, [0, 2, 4, 6, 8, 10, 12, 18]] + [list(range(k)) for k in (1, 19)],
                         ids=["K3", "K4", "K6", "K8", "K1", "K19"])
def test_gather_whole_slots_of_a_low_resolution_grid(lib, idx):
    rng = np.random.default_rng(59)
    slots = [_special(rng, (5, 9, 19)) for _ in range(3)]
    desc = np.array([[2, 5, 9, 0, 0, 0], [0, 5, 9, 0, 0, 0], [1, 5, 9, 0, 0, 0], [2, 5, 9, 0, 0, 0]], dtype=np.int32)
    outs = []
    for sel in (None, idx):
        ring, stride = _ring(lib, slots, sel)
        ch = 19 if sel is None else len(sel)
        out = poisoned((4, 5, 9, ch))
        hip.check(lib.ams_replay_gather_f32(P(ring), stride, 3, 5, 9, ch, P(torch.from_numpy(desc).to(DEV)), desc.ctypes.data_as(C.c_void_p), 4,
                                            P(out), stream()), "ams_replay_gather_f32")
        outs.append(bits(out))
    assert np.array_equal(outs[1], np.ascontiguousarray(np.take(outs[0], idx, axis=-1)))
    assert np.array_equal(outs[0], np.stack([slots[int(d[0])] for d in desc]).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# 3. / 4. the two consumers: one instantiation, two layouts
# ---------------------------------------------------------------------------------------------------------
B, LH, LW, LD, H, W = 2, 5, 9, 32, 65, 129
CONSUMER_CASES = [(19, CI6, (H, W)), (19, CI6, (LH, LW)), (21, [20, 0, 7, 3, 15], (H, W)), (21, [20, 0, 7, 3, 15], (LH, LW))]
CONSUMER_IDS = ["6of19-label_size", "6of19-5x9", "5of21-label_size", "5of21-5x9"]


def _consumer_inputs(nc, idx, grid):
    rng = np.random.default_rng(nc + grid[0])
    z = np.zeros((B, LH, LW, LD), np.float32)
    z[..., :nc] = (rng.standard_normal((B, LH, LW, nc)) * 2).astype(np.float32)
    ids = rng.integers(0, nc, (B, H, W)).astype(np.uint8)
    ids[rng.random((B, H, W)) < 0.1] = 255                                             # ignored ids
    tl = (rng.standard_normal((B,) + grid + (nc,)) * 3).astype(np.float32)
    packed = np.ascontiguousarray(np.take(tl, idx, axis=-1))
    wrong = np.ascontiguousarray(np.take(tl, idx[1:] + idx[:1], axis=-1))              # the channels of a rotated table
    dev = [torch.from_numpy(a).to(DEV) for a in (z, ids, tl, packed, wrong)]
    return dev


def _loss(lib, zd, idd, tld, nc, idx, grid, layout):
    n = lib.ams_k_ce_loss_grad_scratch(B, LH, LW, len(idx))
    scr = torch.full((n,), float("nan"), device=DEV)
    loss = torch.full((2,), float("nan"), dtype=torch.float64, device=DEV)
    dl = poisoned((B, LH, LW, LD))
    rc = lib.ams_k_ce_loss_grad_soft_layout(P(zd), B, LH, LW, LD, nc, table(idx), len(idx), H, W, P(idd), P(tld), grid[0], grid[1], layout,
                                            P(loss), P(dl), P(scr), n, stream())
    return rc, loss.cpu().numpy().view(np.uint64), bits(dl)


@pytest.mark.parametrize("nc,idx,grid", CONSUMER_CASES, ids=CONSUMER_IDS)
def test_loss_kernel_gives_the_same_bits_on_both_layouts(lib, nc, idx, grid):
    zd, idd, tld, packed, wrong = _consumer_inputs(nc, idx, grid)
    rc_f, loss_f, dl_f = _loss(lib, zd, idd, tld, nc, idx, grid, FULL)
    rc_s, loss_s, dl_s = _loss(lib, zd, idd, packed, nc, idx, grid, SELECTED)
    hip.check(rc_f), hip.check(rc_s)
    valid = int(np.isin(idd.cpu().numpy(), idx).sum())
    assert loss_f.view(np.float64)[1] == valid and 0 < valid < B * H * W and np.isfinite(loss_f.view(np.float64)[0])
    assert np.array_equal(loss_s, loss_f) and np.array_equal(dl_s, dl_f)
    assert np.isfinite(dl_f.view(np.float32)).all() and np.any(dl_f.view(np.float32)[..., idx] != 0)
    # the old entry is the full layout
    n = lib.ams_k_ce_loss_grad_scratch(B, LH, LW, len(idx))
    z_nc = zd[..., :nc].contiguous()
    scr, loss = torch.empty(n, device=DEV), torch.empty(2, dtype=torch.float64, device=DEV)
    dl = poisoned((B, LH, LW, nc))
    hip.check(lib.ams_k_ce_loss_grad_soft(P(z_nc), B, LH, LW, nc, table(idx), len(idx), H, W, P(idd), P(tld), grid[0], grid[1], P(loss), P(dl),
                                          P(scr), n, stream()))
    assert np.array_equal(loss.cpu().numpy().view(np.uint64), loss_f) and np.array_equal(bits(dl), dl_f[..., :nc])
    # the test can fail: the channels of another table give another loss and gradient
    rc_w, loss_w, dl_w = _loss(lib, zd, idd, wrong, nc, idx, grid, SELECTED)
    hip.check(rc_w)
    assert loss_w[1] == loss_f[1] and loss_w[0] != loss_f[0] and not np.array_equal(dl_w, dl_f)


def _metric(lib, zd, idd, tld, nc, idx, grid, layout):
    K = len(idx)
    stats = torch.full((B, int(lib.ams_soft_metric_stats_len(K))), -7, dtype=torch.int64, device=DEV)
    p, ce = poisoned((B, H, W, K)), poisoned((B, H, W))
    rc = lib.ams_k_upsample_soft_metric_layout(P(zd), B, LH, LW, LD, nc, table(idx), K, H, W, P(idd), P(tld), grid[0], grid[1], layout, P(stats),
                                               P(p), P(ce), stream())
    return rc, stats.cpu().numpy(), bits(p), bits(ce)


@pytest.mark.parametrize("nc,idx,grid", CONSUMER_CASES, ids=CONSUMER_IDS)
def test_soft_metric_gives_the_same_rows_and_maps_on_both_layouts(lib, nc, idx, grid):
    zd, idd, tld, packed, wrong = _consumer_inputs(nc, idx, grid)
    rc_f, stats_f, p_f, ce_f = _metric(lib, zd, idd, tld, nc, idx, grid, FULL)
    rc_s, stats_s, p_s, ce_s = _metric(lib, zd, idd, packed, nc, idx, grid, SELECTED)
    hip.check(rc_f), hip.check(rc_s)
    assert stats_f[:, 0].sum() == int(np.isin(idd.cpu().numpy(), idx).sum()) and (stats_f[:, 1] > 0).all()
    assert np.array_equal(stats_s, stats_f) and np.array_equal(p_s, p_f) and np.array_equal(ce_s, ce_f)
    assert (p_f != POISON).all() and (ce_f != POISON).all()
    rc_w, stats_w, p_w, _ce_w = _metric(lib, zd, idd, wrong, nc, idx, grid, SELECTED)
    hip.check(rc_w)
    assert not np.array_equal(stats_w, stats_f) and not np.array_equal(p_w, p_f)


def test_consumers_refuse_an_unknown_layout_and_a_bad_table(lib):
    nc, idx, grid = 19, CI6, (LH, LW)
    zd, idd, tld, packed, _wrong = _consumer_inputs(nc, idx, grid)
    K = len(idx)
    n = lib.ams_k_ce_loss_grad_scratch(B, LH, LW, K)
    scr = torch.empty(n, device=DEV)
    loss, dl = poisoned((4,)), poisoned((B, LH, LW, LD))
    stats, p, ce = poisoned((B, 2 * int(lib.ams_soft_metric_stats_len(K)))), poisoned((B, H, W, K)), poisoned((B, H, W))
    for layout, tab, k in ((2, table(idx), K), (-1, table(idx), K), (SELECTED, None, K), (SELECTED, table(idx), 0), (SELECTED, table(idx * 6), 33),
                           (SELECTED, table([0, 19]), 2)):
        assert lib.ams_k_ce_loss_grad_soft_layout(P(zd), B, LH, LW, LD, nc, tab, k, H, W, P(idd), P(packed), grid[0], grid[1], layout, P(loss), P(dl),
                                                  P(scr), n, stream()) == E_INVALID
        assert lib.ams_k_upsample_soft_metric_layout(P(zd), B, LH, LW, LD, nc, tab, k, H, W, P(idd), P(packed), grid[0], grid[1], layout, P(stats),
                                                     P(p), P(ce), stream()) == E_INVALID
    torch.cuda.synchronize()
    for out in (loss, dl, stats, p, ce):
        assert (bits(out) == POISON).all()


# ---------------------------------------------------------------------------------------------------------
# 5. end to end: a selected memory trains, evaluates and predicts as a full one does
# ---------------------------------------------------------------------------------------------------------
EH, EW, NC = 64, 128, 19


def _seed(seed):
    np.random.seed(seed)
    random.seed(seed)


def test_selected_memory_trains_and_evaluates_bit_for_bit():
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    rng = np.random.default_rng(64)
    frames = [rng.integers(0, 256, (EH, EW, 3), dtype=np.uint8) for _ in range(6)]
    labels = [np.repeat(np.repeat(rng.integers(0, NC, (EH // 8, EW // 8), dtype=np.uint8), 8, axis=0), 8, axis=1) for _ in range(6)]
    logits = []
    for l in labels:                                     # noise and a bump on the label's class, as a teacher whose argmax gave the labels
        t = rng.standard_normal((EH, EW, NC)).astype(np.float32)
        np.put_along_axis(t, l[..., None].astype(np.int64), np.take_along_axis(t, l[..., None].astype(np.int64), 2) + 3.0, axis=2)
        logits.append(t)
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=EH, scale=[1, 1.5], mini_batch_size=2, lr=1e-3, initial_variables=W0,
              soft_teacher=True, flip=True)
    nets = [SemanticNetwork("unused", **kw) for _ in range(2)]
    own = [int(c) for c in nets[0].class_indices_graph]
    assert len(own) == 6
    full = DeviceReplayMemory(6, EH, EW, DEV, logits_shape=(EH, EW, NC))
    sel = DeviceReplayMemory(6, EH, EW, DEV, logits_shape=(EH, EW, NC), logits_select=own)
    assert sel.logits_cached_shape == (EH, EW, 6) and full.nbytes - sel.nbytes == 6 * (full.logits_stride - sel.logits_stride) * 4
    assert full.logits_stride - sel.logits_stride == EH * EW * (NC - 6)                # (both are multiples of 64 floats already)
    for i, (f, l, t) in enumerate(zip(frames, labels, logits)):
        for mem in (full, sel):                          # half the appends are device tensors (the pack kernel), half NumPy arrays
            mem.append(f, l, torch.from_numpy(t).to(DEV) if i % 2 == 0 else t)
    for i, t in enumerate(logits):
        assert np.array_equal(bits(sel[i][2]), np.take(t, own, axis=-1).view(np.uint32))
        assert np.array_equal(bits(full[i][2]), t.view(np.uint32))

    # a memory built with another class list is refused before anything is launched
    other = DeviceReplayMemory(1, EH, EW, DEV, logits_shape=(EH, EW, NC), logits_select=own[:-1] + [own[-1] + 1])
    other.append(frames[0], labels[0], logits[0])
    before = nets[1].get_vars()
    with pytest.raises(AssertionError) as e:
        nets[1].train_with_deque(other, None, 1)
    assert str(own) in str(e.value) and str(list(other.logits_select)) in str(e.value)
    with pytest.raises(AssertionError, match="class index list"):
        nets[1].evaluate_memory(other)
    after = nets[1].get_vars()
    assert all(np.array_equal(before[k], after[k]) for k in before)

    for net, mem in zip(nets, (full, sel)):
        _seed(5)
        net.train_with_deque(mem, None, 3)
    assert nets[0].last_losses == nets[1].last_losses and all(np.isfinite(nets[0].last_losses))
    a, b = nets[0].get_vars(), nets[1].get_vars()
    assert sorted(a) == sorted(b) and any("Adam" in k for k in a)
    assert all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a), [k for k in a if a[k].tobytes() != b[k].tobytes()][:5]
    assert not np.array_equal(a["aspp0/weights:0"], W0["aspp0/weights:0"])

    soft_f, conf_f = nets[0].evaluate_memory(full)
    soft_s, conf_s = nets[1].evaluate_memory(sel)
    assert np.array_equal(soft_s.row, soft_f.row) and soft_f.valid > 0 and np.array_equal(conf_s, conf_f)

    fb, lb = np.stack(frames[:2]), np.stack(labels[:2])
    tb = np.stack(logits[:2])
    want = nets[0].predict_with_soft_metric(fb, lb, tb)
    got = nets[0].predict_with_soft_metric(fb, lb, np.ascontiguousarray(np.take(tb, own, axis=-1)))
    assert len(got) == len(want) == 6 and np.array_equal(got[5].row, want[5].row)
    for g, w in zip(got[:5], want[:5]):
        assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
    p_f, ce_f = nets[0].predict_soft_probabilities(fb, tb)
    p_s, ce_s = nets[0].predict_soft_probabilities(fb, torch.from_numpy(np.take(tb, own, axis=-1)).to(DEV))
    assert np.array_equal(bits(p_s), bits(p_f)) and np.array_equal(bits(ce_s), bits(ce_f))
    with pytest.raises(AssertionError, match="got"):
        nets[0].predict_with_soft_metric(fb, lb, tb[..., :7])
    for net in nets:
        net.close_model()
