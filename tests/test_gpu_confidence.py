"""The student's certainty on the device (k_confidence.hip): the kernel through the C ABI against the NumPy restatement of
ams_amd/confidence.py and against the label kernel it shares its walk with, the engine and SemanticNetwork entry points on a synthetic
frozen student, and the scheduler's --edge_confidence flag."""
import ctypes as C
import filecmp
import glob
import gzip
import os
import random

import numpy as np
import pytest
import torch

from ams_amd import confidence as Cf, exp_configs, hip, run as R, spec as S, synth, weights as Wt
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NB = Cf.NB
NC = 19
SENTINEL = 0x5A

# (h, w, H, W, classes, batch): the head test's shapes (K <= 8 in registers; 19 classes = the per-pixel path; H, W no multiples of block and
# band) and one with two column strips, the second ragged; then the smallest shapes at which the walk down the columns can go wrong: a
# second strip that is mostly dead threads with fewer rows than bands, three frames, in both forms; a scale of 0 on either axis; the identity
SHAPES = [(5, 9, 64, 128, [0, 1, 2, 10, 11, 13], 2), (3, 5, 32, 64, [2, 8, 9, 10, 11, 13], 2), (9, 17, 128, 256, list(range(19)), 2),
          (4, 7, 50, 90, [0, 15], 2), (3, 5, 40, 300, [0, 1, 2, 5, 8, 10, 11, 13], 2),
          (3, 5, 7, 300, [0, 1, 2, 10, 11, 13], 3), (3, 5, 7, 300, list(range(19)), 3), (1, 4, 9, 33, [0, 1, 2, 10, 11, 13], 2),
          (4, 1, 33, 9, list(range(19)), 2), (5, 9, 5, 9, [0, 15], 2)]


@pytest.fixture(scope="module")
def lib():
    return hip.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(h, w, H, W, B=2):
    rng = np.random.default_rng(h * w)
    logits = (rng.standard_normal((B, h, w, NC)) * 2).astype(np.float32)
    teacher = rng.integers(0, 19, (B, H, W)).astype(np.uint8)
    teacher[rng.random((B, H, W)) < 0.1] = 255
    return logits, teacher


def _confidence(lib, logits_dev, shape, cls, teacher_dev, u8=True, f32=True, stats=True):
    B, h, w, H, W = shape
    K = len(cls)
    n = int(lib.ams_confidence_stats_len())
    out_u8 = torch.full((B, H, W), SENTINEL, dtype=torch.uint8, device=DEV) if u8 else None
    out_f32 = torch.full((B, H, W), -7.0, dtype=torch.float32, device=DEV) if f32 else None
    out_stats = torch.full((B, n), -1, dtype=torch.int64, device=DEV) if stats else None
    hip.check(lib.ams_k_upsample_confidence(P(logits_dev), B, h, w, logits_dev.shape[-1], (C.c_int32 * K)(*cls), K, H, W, P(teacher_dev), P(out_u8), P(out_f32),
                                            P(out_stats), stream()), "ams_k_upsample_confidence")
    return out_u8, out_f32, out_stats


def _labels(lib, logits_dev, shape, cls):
    B, h, w, H, W = shape
    K = len(cls)
    labels = torch.empty((B, H, W), dtype=torch.int32, device=DEV)
    hip.check(lib.ams_k_upsample_argmax(P(logits_dev), B, h, w, NC, (C.c_int32 * K)(*cls), K, H, W, None, P(labels), None, None, stream()))
    return labels.cpu().numpy()


def test_stats_length(lib):
    assert int(lib.ams_confidence_stats_len()) == Cf.STATS_LEN == 4 * NB + 2 * 32 + 1 and hip.CONFIDENCE_BINS == NB


@pytest.mark.parametrize("h,w,H,W,cls,B", SHAPES, ids=["-".join(map(str, s[:4])) + "-" + "x".join(map(str, s[4])) + ("" if s[5] == 2 else "-B%d" % s[5])
                                                       for s in SHAPES])
def test_kernel_against_the_reference(lib, h, w, H, W, cls, B):
    """Largest |conf_f32 - f64 reference| seen on MI355X over these shapes: 2.6e-7 (the bound is the head test's 1e-5)."""
    K = len(cls)
    logits, teacher = _inputs(h, w, H, W, B)
    shape = (B, h, w, H, W)
    ld, td = torch.from_numpy(logits).to(DEV), torch.from_numpy(teacher).to(DEV)
    u8, f32, stats = (t.cpu().numpy() for t in _confidence(lib, ld, shape, cls, td))
    p_ref, rows_ref, arg_ref = Cf.confidence_reference(logits, cls, H, W, teacher)
    labels = _labels(lib, ld, shape, cls)
    assert np.array_equal(arg_ref, labels)                                   # the argmax of the shared arithmetic is the label kernel's, exactly
    err = float(np.abs(f32.astype(np.float64) - p_ref).max())
    print("max |conf_f32 - f64 reference| = %.3e" % err)
    assert err < 1e-5
    assert (f32 > 0).all() and (f32 <= 1).all()
    assert np.array_equal(u8, np.rint(f32 * np.float32(255)).astype(np.uint8))
    # the integer statistics, from the kernel's OWN f32 map: no pixel can sit on the wrong side of a bin edge
    lut = np.full(256, -1)
    lut[cls] = np.arange(K)
    target = lut[teacher]
    valid = target >= 0
    own = Cf.stats_rows(f32, labels, cls, teacher, ce=np.zeros((B, H, W)))
    for b in range(B):
        for name, lo in (("hist", 0), ("hist_valid", NB), ("hist_hit", 2 * NB), ("bin_sum", 3 * NB), ("sel_cnt", Cf.OFF_SEL_CNT)):
            assert np.array_equal(stats[b, lo:lo + NB], own[b, lo:lo + NB]), (b, name)
        assert stats[b, Cf.OFF_SUM_ALL] == own[b, Cf.OFF_SUM_ALL]
        assert stats[b, :NB].sum() == H * W and stats[b, NB:2 * NB].sum() == valid[b].sum()
        assert np.array_equal(stats[b, Cf.OFF_SEL_CNT:Cf.OFF_SEL_SUM], rows_ref[b, Cf.OFF_SEL_CNT:Cf.OFF_SEL_SUM])
        assert not stats[b, Cf.OFF_SEL_CNT + K:Cf.OFF_SEL_SUM].any() and not stats[b, Cf.OFF_SEL_SUM + K:Cf.OFF_SUM_ALL].any()
        cnt = stats[b, Cf.OFF_SEL_CNT:Cf.OFF_SEL_CNT + K]
        assert (cnt > 0).all()
        got = stats[b, Cf.OFF_SEL_SUM:Cf.OFF_SEL_SUM + K] / cnt
        want = rows_ref[b, Cf.OFF_SEL_SUM:Cf.OFF_SEL_SUM + K] / cnt
        assert np.abs(got / want - 1).max() < 1e-5, (b, got, want)
    # a frame's row does not depend on the batch it is computed in
    for b in range(B):
        alone = _confidence(lib, ld[b:b + 1].contiguous(), (1, h, w, H, W), cls, td[b:b + 1].contiguous(), u8=False, f32=False)[2].cpu().numpy()
        assert np.array_equal(alone[0], stats[b]), b


def test_all_ignored_teacher_and_no_teacher(lib):
    h, w, H, W, cls, _ = SHAPES[0]
    logits, _ = _inputs(h, w, H, W)
    ld = torch.from_numpy(logits).to(DEV)
    blank = torch.full((2, H, W), 255, dtype=torch.uint8, device=DEV)
    with_blank = _confidence(lib, ld, (2, h, w, H, W), cls, blank)[2].cpu().numpy()
    without = _confidence(lib, ld, (2, h, w, H, W), cls, None)[2].cpu().numpy()
    assert np.array_equal(with_blank, without)
    assert not without[:, NB:Cf.OFF_SUM_ALL].any()
    assert without[:, :NB].sum() == 2 * H * W and (without[:, Cf.OFF_SUM_ALL] > 0).all()


def test_null_outputs_write_nothing_else(lib):
    h, w, H, W, cls, _ = SHAPES[3]
    K, B = len(cls), 2
    logits, teacher = _inputs(h, w, H, W)
    ld, td = torch.from_numpy(logits).to(DEV), torch.from_numpy(teacher).to(DEV)
    want_u8, _f, want_stats = _confidence(lib, ld, (B, h, w, H, W), cls, td)
    n = Cf.STATS_LEN
    px = B * H * W
    pad = 256
    # one block: pad | stats | pad | u8 map | pad   (offsets multiples of 8)
    o_stats, o_u8 = pad, pad + 8 * B * n + pad
    o_u8 += -o_u8 % 8
    total = o_u8 + px + pad
    ci = (C.c_int32 * K)(*cls)
    for only in ("stats", "u8"):
        block = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
        base = block.data_ptr()
        hip.check(lib.ams_k_upsample_confidence(P(ld), B, h, w, NC, ci, K, H, W, P(td), C.c_void_p(base + o_u8) if only == "u8" else None, None,
                                                C.c_void_p(base + o_stats) if only == "stats" else None, stream()))
        host = block.cpu().numpy()
        lo, hi = (o_stats, o_stats + 8 * B * n) if only == "stats" else (o_u8, o_u8 + px)
        assert (host[:lo] == SENTINEL).all() and (host[hi:] == SENTINEL).all(), only
        if only == "stats":
            assert np.array_equal(host[lo:hi].view(np.int64).reshape(B, n), want_stats.cpu().numpy())
        else:
            assert np.array_equal(host[lo:hi].reshape(B, H, W), want_u8.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- engine / SemanticNetwork
H = 64
CI = [0, 1, 2, 10, 11, 13]


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


@pytest.fixture(scope="module")
def clip():
    return synth.SyntheticVideo(H, 3, CI, seed=5).clip()


def _edge(W0, **kw):
    return SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True, frozen_graph=FrozenGraph(W0, CI, H, 19), **kw)


@pytest.fixture(scope="module")
def edge(W0):
    net = _edge(W0, max_batch=3)
    yield net
    net.close_model()


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
        assert np.asarray(g).dtype == np.asarray(w).dtype


@pytest.mark.parametrize("n", [1, 3])
def test_predict_with_confidence_equals_the_plain_calls_and_the_kernel(lib, edge, clip, n):
    frames, labels = clip[0][:n], clip[1][:n]
    want = edge.predict_with_metric(frames, labels)
    got = edge.predict_with_confidence(frames, labels)
    assert len(got) == 6
    _same(got[:5], want)
    conf = got[5]
    assert conf.map.is_cuda and conf.map.dtype == torch.uint8 and tuple(conf.map.shape) == (n, H, 2 * H) and len(conf.stats) == n
    # ... the kernel itself on the logits the pass left on the device
    eng = edge.engine
    h, w = eng.lowres
    low = eng.logits_lowres.view(-1, h, w, 32)[:n].clone()
    td = torch.from_numpy(labels).to(DEV)
    u8, f32, stats = _confidence(lib, low, (n, h, w, H, 2 * H), CI, td)
    assert torch.equal(conf.map, u8)
    assert np.array_equal(np.stack([s.row for s in conf.stats]), stats.cpu().numpy())
    for s in conf.stats:
        assert s.n_pixels == H * 2 * H and s.has_teacher and 1 / len(CI) <= s.mean <= 1 and 0 <= s.ece <= 1 and len(s.sel_cnt) == len(CI)
    assert np.array_equal(conf.host(), u8.cpu().numpy())
    # probabilities_reduced on the host
    probs = edge.predict_probabilities(frames)
    assert probs.dtype == np.float32 and probs.shape == (n, H, 2 * H) and np.array_equal(probs, f32.cpu().numpy())
    p_ref = Cf.confidence_reference(low.cpu().numpy()[..., :NC], CI, H, 2 * H)[0]
    assert np.abs(probs - p_ref).max() < 1e-5
    # without a teacher: predict_input's labels and the label-free statistics
    labels_only, free = edge.predict_with_confidence(frames)
    plain = edge.predict_input(frames)
    assert np.array_equal(labels_only, plain) and labels_only.dtype == plain.dtype
    assert torch.equal(free.map, u8) and all(not s.has_teacher and np.array_equal(s.hist, t.hist) and s.sum_all == t.sum_all
                                              for s, t in zip(free.stats, conf.stats))
    # the plain call afterwards: what it returned before
    _same(edge.predict_with_metric(frames, labels), want)
    # behind a rendered pass: predict_rendered's own result, then the same confidence
    *rendered, again = edge.predict_rendered(frames, labels, views=("cross_mask",), confidence=True)
    assert len(rendered) == 6 and list(rendered[5]) == ["cross_mask"]
    _same(rendered[:5], want)
    assert torch.equal(again.map, u8) and np.array_equal(np.stack([s.row for s in again.stats]), stats.cpu().numpy())
    assert len(edge.predict_rendered(frames, labels, views=("cross_mask",))) == 6          # not asked for: the call as it was


@pytest.mark.parametrize("n", [1, 3])
def test_label_free_forms_of_the_pass(edge, clip, n):
    """Without teacher labels predict_rendered and predict_with_confidence hand back predict_input's labels, no metrics, and what does not
    depend on the labels exactly as the call with labels gives it; of the statistics only the label-free fields are populated."""
    frames, labels = clip[0][:n], clip[1][:n]
    views = ("colour_student", "overlay_student")
    plain = edge.predict_input(frames)
    full = edge.predict_rendered(frames, labels, views, confidence=True)
    assert len(full) == 7
    rendered = edge.predict_rendered(frames, None, views, confidence=True)
    certain = edge.predict_with_confidence(frames, None)
    assert len(rendered) == 3 and len(certain) == 2
    for got in (rendered, certain):
        assert np.array_equal(got[0], plain) and got[0].dtype == plain.dtype == np.int32
        conf = got[-1]
        assert torch.equal(conf.map, full[6].map) and len(conf.stats) == n
        for s, t in zip(conf.stats, full[6].stats):
            assert np.array_equal(s.hist, t.hist) and s.sum_all == t.sum_all and s.n_pixels == H * 2 * H and s.mean == t.mean
            assert not s.has_teacher and t.has_teacher
            assert not s.hist_valid.any() and not s.hist_hit.any() and not s.bin_sum.any() and not s.sel_cnt.any() and not s.sel_sum.any()
    assert list(rendered[1]) == list(views)
    for v in views:
        assert rendered[1][v].is_cuda and torch.equal(rendered[1][v], full[5][v])
    assert len(edge.predict_rendered(frames, None, views)) == 2


def test_confidence_refuses_a_batch_out_of_range(lib, edge):
    n = Cf.STATS_LEN
    stats = torch.full((4, n), -1, dtype=torch.int64, device=DEV)
    for batch in (0, 4):
        rc = lib.ams_student_confidence(edge.engine._h, batch, None, None, None, P(stats), stream())
        msg = lib.ams_last_error()
        assert rc != 0 and msg and b"confidence: batch" in msg
    torch.cuda.synchronize()
    assert bool((stats == -1).all())


def test_pipelined_confidence_gives_the_same_per_frame(W0, edge, clip):
    frames, labels = clip
    piped = _edge(W0, pipeline_depth=2)
    try:
        tickets = [piped.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1], confidence=True) for k in range(3)]
        results = [piped.collect(t) for t in tickets]                     # the third frame's pass overwrites the logits of the first two
        rows = []
        for k in range(3):                                                # frame 1 is the second frame of its pass: index 1 of map and rows
            *want, conf = edge.predict_with_confidence(frames[k:k + 1], labels[k:k + 1])
            _same(results[k], want)
            got = piped.take_confidence(tickets[k])
            assert tuple(got.map.shape) == (1, H, 2 * H) and got.map.cpu().numpy().tobytes() == conf.map.cpu().numpy().tobytes()
            assert len(got.stats) == 1 and np.array_equal(got.stats[0].row, conf.stats[0].row)
            rows.append(got.stats[0].row)
            with pytest.raises(AssertionError):
                piped.take_confidence(tickets[k])                         # once per ticket
        assert not np.array_equal(rows[0], rows[1]) and not np.array_equal(rows[1], rows[2])      # the frames differ: a wrong index would show
        # a pass in which only the second frame asks, and a ticket that did not ask
        quiet = piped.predict_with_metric_async(frames[:1], labels[:1])
        asked = piped.predict_with_metric_async(frames[2:3], labels[2:3], confidence=True)
        assert np.array_equal(piped.take_confidence(asked).stats[0].row, rows[2])
        with pytest.raises(AssertionError):
            piped.take_confidence(quiet)
        piped.collect(quiet), piped.collect(asked)
        t = piped.predict_with_metric_async(frames[:1], labels[:1], confidence=True)      # taken before the frame is collected: launched for it
        early = piped.take_confidence(t)
        first = edge.predict_with_confidence(frames[:1], labels[:1])[5]
        assert np.array_equal(early.stats[0].row, first.stats[0].row) and torch.equal(early.map, first.map)
        assert np.array_equal(piped.collect(t)[0], results[0][0])
    finally:
        piped.close_model()


def test_training_network_has_confidence_too(W0, clip):
    frames, labels = clip[0][:1], clip[1][:1]
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=1, lr=1e-3, initial_variables=W0)
    try:
        want = net.predict_with_metric(frames, labels)
        *got, conf = net.predict_with_confidence(frames, labels)
        _same(got, want)
        assert conf.stats[0].hist.sum() == H * 2 * H and conf.stats[0].n_valid == int((np.isin(labels, CI)).sum())
        assert net.predict_probabilities(frames).shape == (1, H, 2 * H)
    finally:
        net.close_model()


# ---------------------------------------------------------------------------------------------------- scheduler
ARGS = ["--input_video", "synthetic:25-demo:seconds=3", "--student_checkpoint", "synthetic:0", "--gpu", "0", "--mode", "simple", "--height", "64",
        "--batch_size", "2", "--iter", "1", "--send_period", "3", "--train_period", "2", "--first_train_time", "2", "--memory_len", "4"]


def _scheduler(out, extra):
    np.random.seed(13)
    random.seed(13)
    summary = R.main(ARGS + ["--output_dir", out] + extra)
    assert summary["frames"] == 90
    return out


def test_scheduler_logs_confidence_and_changes_no_other_file(tmp_path):
    a_dir, b_dir = _scheduler(str(tmp_path / "plain") + "/", []), _scheduler(str(tmp_path / "flagged") + "/", ["--edge_confidence"])
    names = sorted(os.path.basename(p) for p in glob.glob(a_dir + "*"))
    extra = sorted(set(os.path.basename(p) for p in glob.glob(b_dir + "*")) - set(names))
    # <results> = <label>_results_<video>_<checkpoint>_<height>
    assert len(extra) == 2 and all("_results_" in e for e in extra) and extra[0].endswith("_confidence.npy") and extra[1].endswith("_reliability.npy"), extra
    for name in names:
        a, b = a_dir + name, b_dir + name
        if name.endswith("_train_ms.npy"):                                  # wall-clock times
            assert np.load(a).shape == np.load(b).shape
        elif name.endswith(".gz"):                                          # the header holds the time it was written
            with gzip.open(a, "rb") as fa, gzip.open(b, "rb") as fb:
                assert fa.read() == fb.read() and os.path.getsize(a) == os.path.getsize(b), name
        else:
            assert filecmp.cmp(a, b, shallow=False), name
    conf, rel = np.load(b_dir + extra[0]), np.load(b_dir + extra[1])
    assert conf.shape == (90, 3) and conf.dtype == np.float64 and rel.shape == (90, 3, NB) and rel.dtype == np.int64
    K = int(exp_configs.class_weights(25).sum())
    assert (conf[:, 0] >= 1 / K).all() and (conf[:, 0] <= 1).all()
    assert (conf[:, 1] >= 0).all() and (conf[:, 1] <= 1).all() and (conf[:, 2] >= 0).all() and (conf[:, 2] <= 1).all()
    assert (rel[:, 1] <= rel[:, 0]).all() and (rel[:, 0].sum(axis=1) > 0).all()
