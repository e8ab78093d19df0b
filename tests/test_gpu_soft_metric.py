"""Soft-teacher evaluation on the device (k_soft_metric.hip): the kernel through the C ABI against the NumPy restatement of
ams_amd/soft_metric.py, against its own maps (the integer rows, exactly) and against the label / metric kernel it shares its walk with;
then the SemanticNetwork entry points on a synthetic student, live and frozen, and evaluate_memory over a replay memory."""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import exp_configs, hip, soft_metric as SM, spec as S, synth, weights as Wt
from ams_amd.replay import DeviceReplayMemory
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x5A
ONE = 1 << 20
CI6 = [0, 1, 2, 10, 11, 13]

# (h, w, H, W, classes, NC, batch, teacher grid or None = the label size, hard ids given)
CASES = [
    (3, 5, 33, 65, CI6, 19, 1, None, True), (3, 5, 33, 65, CI6, 19, 3, None, True), (3, 5, 33, 65, CI6, 19, 3, (3, 5), True),
    (3, 5, 33, 65, CI6, 19, 1, (3, 5), False), (3, 5, 33, 65, CI6, 19, 3, None, False),
    (5, 9, 64, 128, list(range(19)), 19, 2, (9, 17), True),                      # the KMAX = 0 form; two rows per band, a third grid
    (2, 3, 17, 40, [0, 1, 2, 5, 8, 10, 11, 13], 19, 1, None, True),              # the edge of the register form
    (3, 5, 33, 65, list(range(32)), 32, 1, None, True),
    # the smallest shapes at which the walk down the columns can go wrong: a second column strip that is mostly dead threads with fewer rows
    # than bands, three frames, in both forms; a scale of 0 on either axis; the identity
    (3, 5, 7, 300, CI6, 19, 3, None, True), (3, 5, 7, 300, list(range(19)), 19, 3, (3, 5), True),
    (1, 4, 9, 33, CI6, 19, 1, None, True), (4, 1, 33, 9, list(range(19)), 19, 1, (4, 1), True), (5, 9, 5, 9, CI6, 19, 1, None, True),
    # a tenth field: the row stride of the student's logits, fed through ams_k_upsample_soft_metric_layout (32 = the student's own: its 19
    # logits lie in rows of 32 floats, the rest filled with a value no output may show), in both forms
    (5, 9, 64, 128, CI6, 19, 2, None, True, 32), (5, 9, 64, 128, list(range(19)), 19, 2, (9, 17), True, 32),
]


@pytest.fixture(scope="module")
def lib():
    return hip.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(h, w, H, W, cls, NC, B, grid):
    rng = np.random.default_rng(1000 * h + w + 7 * B + len(cls))
    logits = (rng.standard_normal((B, h, w, NC)) * 2).astype(np.float32)
    th, tw = grid or (H, W)
    tlog = (rng.standard_normal((B, th, tw, NC)) * 3).astype(np.float32)
    ids = rng.integers(0, NC, (B, H, W)).astype(np.uint8)
    ids[rng.random((B, H, W)) < 0.1] = 255
    outside = [c for c in range(NC) if c not in cls]
    ids[:, :, 1] = 255                                                           # every row holds an ignored id ...
    if outside:
        ids[:, :, 2] = outside[0]                                                # ... and one outside the subset
    return logits, tlog, ids


def _soft(lib, ld, tld, ids_dev, shape, cls, stats=True, maps=True, stride=None):
    B, h, w, H, W = shape
    K = len(cls)
    n = int(lib.ams_soft_metric_stats_len(K))
    out_stats = torch.full((B, n), -1, dtype=torch.int64, device=DEV) if stats else None
    out_p = torch.full((B, H, W, K), -7.0, dtype=torch.float32, device=DEV) if maps else None
    out_ce = torch.full((B, H, W), -7.0, dtype=torch.float32, device=DEV) if maps else None
    if stride is not None:
        NC = ld.shape[-1]
        wide = torch.full((B, h, w, stride), 1e30, dtype=torch.float32, device=DEV)
        wide[..., :NC] = ld
        hip.check(lib.ams_k_upsample_soft_metric_layout(P(wide), B, h, w, stride, NC, (C.c_int32 * K)(*cls), K, H, W, P(ids_dev), P(tld), tld.shape[1],
                                                        tld.shape[2], hip.TLOGITS_FULL, P(out_stats), P(out_p), P(out_ce), stream()),
                  "ams_k_upsample_soft_metric_layout")
        torch.cuda.synchronize()
        return out_stats, out_p, out_ce
    hip.check(lib.ams_k_upsample_soft_metric(P(ld), B, h, w, ld.shape[-1], (C.c_int32 * K)(*cls), K, H, W, P(ids_dev), P(tld), tld.shape[1], tld.shape[2],
                                             P(out_stats), P(out_p), P(out_ce), stream()), "ams_k_upsample_soft_metric")
    return out_stats, out_p, out_ce


def _labels(lib, ld, shape, cls, ids_dev=None):
    """the label kernel on the same logits: labels, and with teacher ids its int64 confusion matrix and [loss sum, valid pixels]"""
    B, h, w, H, W = shape
    K = len(cls)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    conf = torch.zeros(K * K, dtype=torch.int64, device=DEV)
    loss = torch.zeros(2, dtype=torch.float64, device=DEV)
    hip.check(lib.ams_k_upsample_argmax(P(ld), B, h, w, ld.shape[-1], (C.c_int32 * K)(*cls), K, H, W, P(ids_dev), P(labels),
                                        P(conf) if ids_dev is not None else None, P(loss) if ids_dev is not None else None, stream()))
    return labels.cpu().numpy(), conf.cpu().numpy().reshape(K, K), loss.cpu().numpy()


def test_stats_length(lib):
    for K in (1, 6, 19, 32):
        assert int(lib.ams_soft_metric_stats_len(K)) == SM.stats_len(K) == 2 + 2 * K * K


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%dx%d-K%dof%d-B%d-%s-%s%s" % (c[0], c[1], c[2], c[3], len(c[4]), c[5], c[6],
                                                                                          "full" if c[7] is None else "%dx%d" % c[7], "ids" if c[8] else "noids",
                                                                                          "-ld%d" % c[9] if len(c) > 9 else ""))
def test_kernel_against_the_reference_and_its_own_maps(lib, case):
    """Largest |p_f32 - f64| and |ce_f32 - f64| seen on MI355X per shape: DESIGN.md 4.9 (the bound is the head test's 1e-5)."""
    h, w, H, W, cls, NC, B, grid, with_ids = case[:9]
    stride = case[9] if len(case) > 9 else None
    K = len(cls)
    logits, tlog, ids = _inputs(h, w, H, W, cls, NC, B, grid)
    shape = (B, h, w, H, W)
    ld, tld = torch.from_numpy(logits).to(DEV), torch.from_numpy(tlog).to(DEV)
    idd = torch.from_numpy(ids).to(DEV) if with_ids else None
    stats, p, ce = (t.cpu().numpy() for t in _soft(lib, ld, tld, idd, shape, cls, stride=stride))
    if stride is not None:                                                       # the same bits as from rows of NC floats
        for got, want in zip((stats, p, ce), _soft(lib, ld, tld, idd, shape, cls)):
            assert np.array_equal(got, want.cpu().numpy(), equal_nan=True)
    ref, p_ref, ce_ref, arg_ref = SM.soft_metric_reference(logits, tlog, ids if with_ids else None, cls, H, W)
    labels = _labels(lib, ld, shape, cls)[0]
    assert np.array_equal(arg_ref, labels)                                       # the shared arithmetic: the label kernel's argmax, exactly
    err_p, err_ce = float(np.abs(p - p_ref).max()), float(np.abs(ce - ce_ref).max())
    print("max |p_f32 - f64| = %.3e, max |ce_f32 - f64| = %.3e" % (err_p, err_ce))
    assert err_p < 1e-5 and err_ce < 1e-5
    # the integer rows are, exactly, what NumPy forms from the kernel's own maps and the label kernel's argmax
    own = SM.stats_rows(p, ce, labels, cls, ids if with_ids else None)
    assert np.array_equal(stats, own)
    if not with_ids:
        assert (stats[:, 0] == H * W).all() and not stats[:, 2 + K * K:].any()   # prob_confmat's unmasked form: no teacher matrix
    # ... and decode to the reference within the f32 bar plus half a unit of the rounding per pixel
    got = SM.SoftMetric.sum(stats)
    assert got.valid == ref.valid
    assert abs(got.loss_soft - ref.loss_soft) < 1e-5 + 2.0 ** -21
    tol = ref.valid * (1e-5 + 2.0 ** -21)
    assert np.abs(got.prob_conf_student - ref.prob_conf_student).max() < tol and np.abs(got.prob_conf_teacher - ref.prob_conf_teacher).max() < tol
    # a frame's row does not depend on the batch it is computed in
    if B > 1:
        for b in range(B):
            alone = _soft(lib, ld[b:b + 1].contiguous(), tld[b:b + 1].contiguous(), idd[b:b + 1].contiguous() if with_ids else None,
                          (1, h, w, H, W), cls, maps=False, stride=stride)[0].cpu().numpy()
            assert np.array_equal(alone[0], stats[b]), b


def test_one_hot_teacher_logits_give_the_hard_metrics(lib):
    """60 * onehot(hard id) at the label size: the teacher's distribution is the one-hot row up to exp(-60) = 8.8e-27, which f32 represents
    (so the cold entries are that, not 0: they are 0 in the fixed point, which is what the matrices add) and the hot entry is exactly 1."""
    h, w, H, W, cls, NC, B = 3, 5, 33, 65, CI6, 19, 3
    K = len(cls)
    logits, _t, ids = _inputs(h, w, H, W, cls, NC, B, None)
    tlog = np.zeros((B, H, W, NC), dtype=np.float32)
    inside = ids < NC
    tlog[inside, ids[inside]] = 60.0
    shape = (B, h, w, H, W)
    ld, tld, idd = torch.from_numpy(logits).to(DEV), torch.from_numpy(tlog).to(DEV), torch.from_numpy(ids).to(DEV)
    stats, p, ce = (t.cpu().numpy() for t in _soft(lib, ld, tld, idd, shape, cls))
    lut = np.full(256, -1)
    lut[cls] = np.arange(K)
    target = lut[ids]
    valid = target >= 0
    hot = np.take_along_axis(p[valid], target[valid][:, None], axis=1)[:, 0]
    assert (hot == 1.0).all()
    cold = p[valid].copy()
    cold[np.arange(cold.shape[0]), target[valid]] = 0
    assert (cold >= 0).all() and cold.max() < 1e-25
    _lab, conf, loss = _labels(lib, ld, shape, cls, idd)
    total = stats.sum(axis=0)
    assert total[0] == valid.sum() == int(loss[1])
    assert np.array_equal(total[2:2 + K * K].reshape(K, K), ONE * conf)
    assert np.array_equal(total[2 + K * K:].reshape(K, K), ONE * np.diag(np.bincount(target[valid], minlength=K)))
    assert abs(total[1] / ONE / total[0] - loss[0] / loss[1]) < 1e-5 + 2.0 ** -21


def test_output_combinations_write_nothing_else(lib):
    h, w, H, W, cls, NC, B = 2, 3, 17, 40, [0, 1, 2, 5, 8, 10, 11, 13], 19, 2
    K = len(cls)
    logits, tlog, ids = _inputs(h, w, H, W, cls, NC, B, None)
    ld, tld, idd = torch.from_numpy(logits).to(DEV), torch.from_numpy(tlog).to(DEV), torch.from_numpy(ids).to(DEV)
    want = [t.cpu().numpy() for t in _soft(lib, ld, tld, idd, (B, h, w, H, W), cls)]
    n, px, pad = SM.stats_len(K), B * H * W, 256
    # one block: pad | stats | pad | p | pad | ce | pad   (offsets multiples of 8)
    sizes = [8 * B * n, 4 * px * K, 4 * px]
    offs, o = [], pad
    for sz in sizes:
        offs.append(o)
        o += sz + pad + (-sz % 8)
    ci = (C.c_int32 * K)(*cls)
    for given in ((True, False, False), (False, True, True), (False, False, False)):
        block = torch.full((o,), SENTINEL, dtype=torch.uint8, device=DEV)
        ptr = [C.c_void_p(block.data_ptr() + off) if g else None for off, g in zip(offs, given)]
        hip.check(lib.ams_k_upsample_soft_metric(P(ld), B, h, w, NC, ci, K, H, W, P(idd), P(tld), H, W, ptr[0], ptr[1], ptr[2], stream()))
        host = block.cpu().numpy()
        keep = np.ones(o, dtype=bool)
        for off, sz, g, ref, dt in zip(offs, sizes, given, want, (np.int64, np.float32, np.float32)):
            if g:
                keep[off:off + sz] = False
                assert np.array_equal(host[off:off + sz].view(dt), ref.reshape(-1)), given
        assert (host[keep] == SENTINEL).all(), given


def test_nan_pixels_are_counted_and_add_nothing(lib):
    h, w, H, W, cls, NC, B = 3, 5, 33, 65, CI6, 19, 1
    K = len(cls)
    logits, tlog, ids = _inputs(h, w, H, W, cls, NC, B, None)
    ids[0, 10:23, 20:40] = cls[1]                                                # valid pixels around both plants
    logits[0, 1, 2, cls[3]] = np.nan                                             # every pixel interpolated from this cell
    tlog[0, 5, 50, cls[0]] = np.nan
    ids[0, 5, 50] = cls[2]
    ld, tld, idd = torch.from_numpy(logits).to(DEV), torch.from_numpy(tlog).to(DEV), torch.from_numpy(ids).to(DEV)
    stats, p, ce = (t.cpu().numpy() for t in _soft(lib, ld, tld, idd, (B, h, w, H, W), cls))
    lut = np.full(256, -1)
    lut[cls] = np.arange(K)
    valid = lut[ids] >= 0
    bad = np.isnan(ce)
    assert np.isnan(ce[0, 5, 50]) and np.isnan(p[0, 5, 50]).all() and np.isnan(ce[0, 16, 32]) and not np.isnan(p[0, 16, 32]).any()
    assert (bad & valid).sum() > 10 and (~bad & valid).sum() > 100
    assert stats[0, 0] == valid.sum()                                            # counted ...
    labels = _labels(lib, ld, (B, h, w, H, W), cls)[0]
    clean_p, clean_ce = np.where(bad[..., None], 0, p), np.where(bad, 0, ce)
    want = SM.stats_rows(clean_p, clean_ce, labels, cls, ids)                    # ... and 0 everywhere else
    assert np.array_equal(stats, want) and np.array_equal(stats, SM.stats_rows(p, ce, labels, cls, ids))
    assert stats[0, 2:2 + K * K].sum() < ONE * ((~bad & valid).sum() + 1)


def test_refused_arguments_write_nothing(lib):
    h, w, H, W, cls, NC = 3, 5, 33, 65, CI6, 19
    K = len(cls)
    logits, tlog, ids = _inputs(h, w, H, W, cls, NC, 1, None)
    ld, idd = torch.from_numpy(logits).to(DEV), torch.from_numpy(ids).to(DEV)
    big = torch.zeros((1, H + 1, W, NC), dtype=torch.float32, device=DEV)
    tld = torch.from_numpy(tlog).to(DEV)
    stats = torch.full((1, SM.stats_len(32)), -1, dtype=torch.int64, device=DEV)
    p = torch.full((1, H, W, 33), -7.0, dtype=torch.float32, device=DEV)
    ce = torch.full((1, H, W), -7.0, dtype=torch.float32, device=DEV)
    many = list(range(19)) + list(range(14))
    for B, k_cls, t, th, tw in ((0, cls, tld, H, W), (1, many, tld, H, W), (1, cls, big, H + 1, W), (1, cls, tld, H, W + 1)):
        rc = lib.ams_k_upsample_soft_metric(P(ld), B, h, w, NC, (C.c_int32 * len(k_cls))(*k_cls), len(k_cls), H, W, P(idd), P(t), th, tw,
                                            P(stats), P(p), P(ce), stream())
        assert rc == -1 and lib.ams_last_error(), (B, len(k_cls), th, tw)          # AMS_E_INVALID
    torch.cuda.synchronize()
    assert bool((stats == -1).all()) and bool((p == -7.0).all()) and bool((ce == -7.0).all())
    assert int(lib.ams_soft_metric_stats_len(33)) == 0 and int(lib.ams_soft_metric_stats_len(0)) == 0


# ---------------------------------------------------------------------------------------------------- SemanticNetwork
H = 64
NC = 19


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


@pytest.fixture(scope="module")
def clip():
    frames, labels = synth.SyntheticVideo(H, 5, CI6, seed=5).clip()
    rng = np.random.default_rng(11)
    full = (rng.standard_normal((5, H, 2 * H, NC)) * 3).astype(np.float32)
    small = (rng.standard_normal((5, 5, 9, NC)) * 3).astype(np.float32)
    return frames, labels, full, small


def _edge(W0, **kw):
    return SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True, frozen_graph=FrozenGraph(W0, CI6, H, 19), **kw)


@pytest.fixture(scope="module")
def edge(W0):
    net = _edge(W0, max_batch=3)
    yield net
    net.close_model()


@pytest.fixture(scope="module")
def live(W0):
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=3, lr=1e-3, initial_variables=W0)
    yield net
    net.close_model()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
        assert np.asarray(g).dtype == np.asarray(w).dtype


@pytest.mark.parametrize("which", ["frozen", "live"])
@pytest.mark.parametrize("grid", ["full", "small"])
def test_predict_with_soft_metric(edge, live, clip, which, grid):
    net = edge if which == "frozen" else live
    n = 3
    frames, labels = clip[0][:n], clip[1][:n]
    tlog = (clip[2] if grid == "full" else clip[3])[:n]
    want = net.predict_with_metric(frames, labels)
    got = net.predict_with_soft_metric(frames, labels, tlog)
    assert len(got) == 6 and isinstance(got[5], SM.SoftMetric)
    _same(got[:5], want)
    soft = got[5]
    # the reference on the logits the pass left on the device
    eng = net.engine
    h, w = eng.lowres
    low = eng.logits_lowres.view(-1, h, w, 32)[:n].cpu().numpy()[..., :NC]
    ref, p_ref, ce_ref, _arg = SM.soft_metric_reference(low, tlog, labels, CI6, H, 2 * H)
    assert soft.valid == ref.valid == int(np.isin(labels, CI6).sum())
    assert abs(soft.loss_soft - ref.loss_soft) < 1e-5 + 2.0 ** -21
    tol = ref.valid * (1e-5 + 2.0 ** -21)
    assert np.abs(soft.prob_conf_student - ref.prob_conf_student).max() < tol and np.abs(soft.prob_conf_teacher - ref.prob_conf_teacher).max() < tol
    np.testing.assert_allclose(soft.soft_iou, ref.soft_iou, atol=1e-4)
    # device tensors give the same row
    dev = net.predict_with_soft_metric(torch.from_numpy(frames).to(DEV), torch.from_numpy(labels).to(DEV), torch.from_numpy(tlog).to(DEV))
    _same(dev[:5], want)
    assert np.array_equal(dev[5].row, soft.row)
    # frozen inference is batch-composition invariant (tests/test_gpu_fullsize.py): the rows of the three one-frame calls add up to the call's
    if which == "frozen":
        singles = [net.predict_with_soft_metric(frames[k:k + 1], labels[k:k + 1], tlog[k:k + 1])[5] for k in range(n)]
        assert np.array_equal(SM.SoftMetric.sum(singles).row, soft.row)
    # the maps
    p, ce = net.predict_soft_probabilities(frames, tlog)
    assert p.dtype == ce.dtype == np.float32 and p.shape == (n, H, 2 * H, len(CI6)) and ce.shape == (n, H, 2 * H)
    assert np.abs(p - p_ref).max() < 1e-5 and np.abs(ce - ce_ref).max() < 1e-5
    # the plain call afterwards: what it returned before
    _same(net.predict_with_metric(frames, labels), want)
    with pytest.raises(AssertionError):
        net.predict_with_soft_metric(frames, labels, tlog[:2])


def test_soft_metric_refuses_a_batch_out_of_range(lib, edge, clip):
    stats = torch.full((4, SM.stats_len(6)), -1, dtype=torch.int64, device=DEV)
    tld = torch.from_numpy(clip[3][:4]).to(DEV)
    for batch in (0, 4):
        rc = lib.ams_student_soft_metric(edge.engine._h, batch, None, P(tld), 5, 9, P(stats), None, None, stream())
        msg = lib.ams_last_error()
        assert rc == -1 and msg and b"soft_metric: batch" in msg
    torch.cuda.synchronize()
    assert bool((stats == -1).all())


def test_pipelined_edge_is_not_disturbed(W0, edge, clip):
    frames, labels, full, _small = clip
    piped = _edge(W0, pipeline_depth=2)
    try:
        want = [edge.predict_with_metric(frames[k:k + 1], labels[k:k + 1]) for k in range(3)]
        before = piped.predict_with_metric_async(frames[:1], labels[:1])
        soft = piped.predict_with_soft_metric(frames[1:2], labels[1:2], full[1:2])       # drains the pipeline first
        after = piped.predict_with_metric_async(frames[2:3], labels[2:3])
        _same(piped.collect(before), want[0])
        _same(piped.collect(after), want[2])
        _same(soft[:5], want[1])
        assert np.array_equal(soft[5].row, edge.predict_with_soft_metric(frames[1:2], labels[1:2], full[1:2])[5].row)
    finally:
        piped.close_model()


@pytest.mark.parametrize("grid", ["full", "small"])
def test_evaluate_memory_is_the_sum_of_the_slots(edge, clip, grid):
    frames, labels, full, small = clip
    tlog = full if grid == "full" else small
    memory = DeviceReplayMemory(5, H, 2 * H, DEV, logits_shape=tlog.shape[1:])
    for k in range(5):
        memory.append(frames[k], labels[k], tlog[k])
    per_slot = [edge.predict_with_soft_metric(frames[k:k + 1], labels[k:k + 1], tlog[k:k + 1]) for k in range(5)]
    soft, conf = edge.evaluate_memory(memory)                                    # passes of 3 and 2 frames
    assert np.array_equal(soft.row, SM.SoftMetric.sum([r[5] for r in per_slot]).row)
    assert conf.dtype == np.float64 and np.array_equal(conf, sum(r[1] for r in per_slot))
    some, conf2 = edge.evaluate_memory(memory, slots=[4, 1])
    assert np.array_equal(some.row, SM.SoftMetric.sum([per_slot[4][5], per_slot[1][5]]).row)
    assert np.array_equal(conf2, per_slot[4][1] + per_slot[1][1])


def test_evaluate_memory_needs_the_logits(edge, clip):
    memory = DeviceReplayMemory(2, H, 2 * H, DEV)
    memory.append(clip[0][0], clip[1][0])
    with pytest.raises(ValueError):
        edge.evaluate_memory(memory)
