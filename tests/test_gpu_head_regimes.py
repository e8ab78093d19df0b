"""The head's read-out kernels (ams_k_upsample_argmax, ams_k_upsample_confidence, ams_k_upsample_soft_metric) at tied, saturated and
non-finite logits: the regimes of tests/logit_regimes.py, which tests/test_logit_regimes_cpu.py holds to what they claim.  Everything goes
through the C ABI on guarded buffers (tests/guarded.py).

The label rule is logit_regimes.first_maximum on the f32 restatement of the interpolation: a strict `>` scan from class 0, so ties and
-0.0 / +0.0 take the lower index and a NaN wins only in class 0.  All three kernels must produce that label: the label kernel in its map
and its confusion matrix, the other two in the integer statistics, which are recomputed from the kernel's OWN f32 maps with the reference
labels and must match exactly.

Loss sums are held by an absolute bound, since a confident student's pixel losses lie below the 2^-20 grid they are rounded to: per pixel
the kernel's value may differ from the f64 loss of the same f32-interpolated logits by

    2^-21 + c 2^-24 (max_k |z_k| + log K),

the rounding to the grid and c units of f32 rounding at the magnitude of the terms; a mean inherits the mean of those bounds, a sum their sum.
c per regime is twice the worst ratio measured on MI355X, rounded up to a power of two (C_BOUND below says which quantity
gave it): ties 4.329 -> 16, quantised 3.855 -> 8, saturated 1.782 -> 4, the finite pixels of the non-finite frames 0 -> 1."""
import ctypes as C

import numpy as np
import pytest
import torch

import logit_regimes as LG
from ams_amd import confidence as Cf, soft_metric as SM
from kernel_suite import P, _guarded_buffers, dev, image_guard, lib, out, run, stream  # noqa: F401

pytestmark = pytest.mark.gpu

NB = Cf.NB
Q = 1048576.0
GRID, ULP = 2.0 ** -21, 2.0 ** -24

# regime -> c of the bound above: twice the worst ratio measured on MI355X over the cases of this file, rounded up to a power of two.  The
# ratios: (|kernel - f64| - the grid term) / (2^-24 (max |z| + log K), summed like the quantity) for the label kernel's mean loss, the
# confidence rows' sel_sum and the soft metric's ce_sum, and |ce_f32 - f64| / (the same) per pixel for the soft metric's own map:
#   ties       sums 0.000, per pixel 4.329 (K = 19: nineteen products p_k (lse - z_k), each p_k through __expf)   -> 16
#   quantised  sums 0.000, per pixel 3.855                                                                        ->  8
#   saturated  sums 0.478 (sel_sum, identity resize, K = 19), per pixel 1.782                                     ->  4
#   nonfinite  sums 0.000 (the finite pixels; no per-pixel map)                                                   ->  1
# No sum ever left the grid term except in `saturated`, where the f32 value of a wrong pixel's loss is rounded at the magnitude of the margin.
C_BOUND = {"ties": 16.0, "quantised": 8.0, "saturated": 4.0, "nonfinite": 1.0}

HEAD_CASES = [c for c in LG.cases() if c[1] in LG.HEAD_SHAPES and tuple(c[4]) == tuple(c[1][2:]) and c[2] == 19]
FINITE = [c for c in HEAD_CASES if c[0] != "nonfinite"]
NONFINITE = [c for c in HEAD_CASES if c[0] == "nonfinite"]


def _id(c):
    return "%s-%s-K%d" % (c[0], "x".join(map(str, c[1])), len(c[3]))


class _Ref:
    pass


_REFS = {}


def _reference(logits, teacher, tl, cls, H, W, key=None):
    """What f64 makes of the f32-interpolated logits: labels by the rule, targets, confusion matrix, per pixel p, the hard and the soft loss and
    the scale of the bound.  Computed once per case and shared (nothing writes to it)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    r = _Ref()
    K = len(cls)
    with np.errstate(invalid="ignore"):
        z = Cf.interpolate_selected(logits, cls, H, W)
    r.z = z
    r.labels = LG.first_maximum(z).astype(np.int32)
    lut = np.full(256, -1)
    lut[cls] = np.arange(K)
    r.target = lut[teacher]
    r.valid = r.target >= 0
    r.cm = np.zeros((K, K), dtype=np.int64)
    np.add.at(r.cm, (r.target[r.valid], r.labels[r.valid]), 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        z64 = z.astype(np.float64)
        zmax = z64.max(-1)
        ssum = np.exp(z64 - zmax[..., None]).sum(-1)
        r.p = 1.0 / ssum
        lse = zmax + np.log(ssum)
        r.ce = lse - np.take_along_axis(z64, np.maximum(r.target, 0)[..., None], -1)[..., 0]
        r.scale = ULP * (np.abs(np.where(np.isfinite(z64), z64, 0.0)).max(-1) + np.log(K))      # over the finite logits of the pixel
        r.finite = np.isfinite(z).all(-1)
        if tl is not None:
            t64 = SM.interpolate_teacher(tl, cls, H, W).astype(np.float64)
            e = np.exp(t64 - t64.max(-1, keepdims=True))
            r.pt = e / e.sum(-1, keepdims=True)
            r.ce_soft = (r.pt * (lse[..., None] - z64)).sum(-1)
    if key is not None:
        _REFS[key] = r
    return r


def _key(case, tag=""):
    return (case[0], tuple(case[1]), case[2], tuple(case[3]), tuple(case[4]), tag)


def _ratio(err, pixels_scale, grid=GRID):
    """how many units of 2^-24 (max |z| + log K) an error takes beyond the rounding to the grid"""
    return max(0.0, err - grid) / pixels_scale


def _argmax(lib, logits, cls, H, W, teacher=None):
    B, h, w, NC = logits.shape
    K = len(cls)
    labels = out((B, H, W), torch.int32, guard=image_guard(W, 1))
    if teacher is None:
        run(lib.ams_k_upsample_argmax(P(dev(logits)), B, h, w, NC, (C.c_int32 * K)(*cls), K, H, W, None, P(labels), None, None, stream()))
        return labels.cpu().numpy()
    conf, loss = out(K * K, torch.int64), out(2, torch.float64)
    run(lib.ams_k_upsample_argmax(P(dev(logits)), B, h, w, NC, (C.c_int32 * K)(*cls), K, H, W, P(dev(teacher, torch.uint8)), P(labels), P(conf),
                                  P(loss), stream()))
    return labels.cpu().numpy(), conf.cpu().numpy().reshape(K, K), loss.cpu().numpy()


def _confidence(lib, logits, cls, H, W, teacher):
    """(u8, f32, stats) of ams_k_upsample_confidence.  A stored 255 is the uint8 guard pattern itself, so the map may keep the pattern exactly
    where the kernel's own f32 map rounds to 255 (which holds conf_u8 == rint(conf_f32 * 255) at those pixels as well)."""
    B, h, w, NC = logits.shape
    K = len(cls)
    u8 = out((B, H, W), torch.uint8, guard=image_guard(W, 1))
    f32 = out((B, H, W), guard=image_guard(W, 1))
    stats = out((B, int(lib.ams_confidence_stats_len())), torch.int64)
    rc = lib.ams_k_upsample_confidence(P(dev(logits)), B, h, w, NC, (C.c_int32 * K)(*cls), K, H, W,
                                       P(dev(teacher, torch.uint8)) if teacher is not None else None, P(u8), P(f32), P(stats), stream())
    keep = None
    if rc == 0:
        try:
            p = f32.cpu().numpy()
        except RuntimeError as e:                                          # a fault of the kernel surfaces at the synchronisation
            pytest.exit("ams_k_upsample_confidence: %s; nothing more runs on this device" % e, returncode=3)
        with np.errstate(invalid="ignore"):
            keep = [(u8, np.rint(p * np.float32(255)) == 255)]
    run(rc, "ams_k_upsample_confidence", untouched=keep)
    return u8.cpu().numpy(), f32.cpu().numpy(), stats.cpu().numpy()


def _soft(lib, logits, cls, H, W, teacher, tl):
    B, h, w, NC = logits.shape
    K = len(cls)
    stats = out((B, int(lib.ams_soft_metric_stats_len(K))), torch.int64)
    p = out((B, H, W, K), guard=image_guard(W, K))
    ce = out((B, H, W), guard=image_guard(W, 1))
    run(lib.ams_k_upsample_soft_metric(P(dev(logits)), B, h, w, NC, (C.c_int32 * K)(*cls), K, H, W, P(dev(teacher, torch.uint8)), P(dev(tl)), tl.shape[1],
                                       tl.shape[2], P(stats), P(p), P(ce), stream()), "ams_k_upsample_soft_metric")
    return stats.cpu().numpy(), p.cpu().numpy(), ce.cpu().numpy()


def _own_rows(f32, labels, cls, teacher):
    """the confidence row's integer fields from the kernel's own map (a NaN p: bin 0, 0 to the sums) and the reference labels"""
    return Cf.stats_rows(np.nan_to_num(f32, nan=0.0), labels, cls, teacher, ce=np.zeros(f32.shape))


_INT_FIELDS = (("hist", 0, NB), ("hist_valid", NB, NB), ("hist_hit", 2 * NB, NB), ("bin_sum", 3 * NB, NB), ("sel_cnt", Cf.OFF_SEL_CNT, Cf.MAX_K),
               ("sum_all", Cf.OFF_SUM_ALL, 1))


def _sel_reference(r, K, ce):
    """per frame and class: (f64 sum of ce over the valid pixels whose teacher class or label is k, the sum of their scales, their number)"""
    B = r.labels.shape[0]
    s, sc, n = np.zeros((B, K)), np.zeros((B, K)), np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        for k in range(K):
            m = r.valid[b] & ((r.target[b] == k) | (r.labels[b] == k))
            s[b, k], sc[b, k], n[b, k] = ce[b][m].sum(), r.scale[b][m].sum(), m.sum()
    return s, sc, n


@pytest.mark.parametrize("case", FINITE, ids=_id)
def test_labels_and_metrics(lib, case):
    """ams_k_upsample_argmax: the label map is first_maximum's exactly, with and without a teacher; the confusion matrix and the valid count are
    exact; the mean loss lies within the absolute bound of the module head."""
    regime, (h, w, H, W), NC, cls, grid = case
    logits, teacher, tl = LG.material(*case)[:3]
    r = _reference(logits, teacher, tl, cls, H, W, _key(case))
    labels, conf, loss = _argmax(lib, logits, cls, H, W, teacher)
    assert np.array_equal(labels, r.labels)
    assert np.array_equal(conf, r.cm)
    n = int(r.valid.sum())
    assert loss[1] == n > 0
    want, scale = r.ce[r.valid].mean(), r.scale[r.valid].mean()
    err = abs(loss[0] / loss[1] - want)
    print("%s: mean loss %.9g (f64 %.9g), |difference| %.3e = grid + %.3f units of the scale %.3e" % (_id(case), loss[0] / n, want, err, _ratio(err, scale), scale))
    assert err <= GRID + C_BOUND[regime] * scale
    assert np.array_equal(_argmax(lib, logits, cls, H, W), r.labels)


@pytest.mark.parametrize("case", FINITE, ids=_id)
def test_confidence(lib, case):
    """ams_k_upsample_confidence: 0 < p <= 1, conf_u8 == rint(conf_f32 * 255), |conf_f32 - f64| < 1e-5 (the existing bar), the plateau's p is
    1.f / K bit for bit, and every integer field equals what NumPy forms from the kernel's own f32 map with the REFERENCE labels: the argmax
    inside this kernel is first_maximum (hist_hit, sel_cnt).  Saturated: p == 1 occurs and the last bin holds exactly the pixels whose own p
    lies in [31/32, 1], at least a quarter of all: the clamp of the bin index runs.  sel_sum per class within the summed bound."""
    regime, (h, w, H, W), NC, cls, grid = case
    K = len(cls)
    logits, teacher, tl = LG.material(*case)[:3]
    r = _reference(logits, teacher, tl, cls, H, W, _key(case))
    u8, f32, stats = _confidence(lib, logits, cls, H, W, teacher)
    assert (f32 > 0).all() and (f32 <= 1).all()
    assert np.array_equal(u8, np.rint(f32 * np.float32(255)).astype(np.uint8))
    err = float(np.abs(f32.astype(np.float64) - r.p).max())
    print("%s: max |conf_f32 - f64| = %.3e" % (_id(case), err))
    assert err < 1e-5
    if regime == "ties":
        plateau = (r.z == r.z.max(-1, keepdims=True)).all(-1)
        assert plateau.any() and (f32[plateau].view(np.uint32) == (np.float32(1) / np.float32(K)).view(np.uint32)).all()
    own = _own_rows(f32, r.labels, cls, teacher)
    for b in range(stats.shape[0]):
        for name, lo, n in _INT_FIELDS:
            assert np.array_equal(stats[b, lo:lo + n], own[b, lo:lo + n]), (b, name)
        assert stats[b, :NB].sum() == H * W and stats[b, NB:2 * NB].sum() == r.valid[b].sum()
    if regime == "saturated":
        last = f32 >= np.float32(31.0 / 32.0)
        assert (f32 == 1).any()
        assert np.array_equal(stats[:, NB - 1], last.sum(axis=(1, 2))) and last.mean() >= 0.25
    want, scale, n = _sel_reference(r, K, r.ce)
    got = stats[:, Cf.OFF_SEL_SUM:Cf.OFF_SEL_SUM + K] / Q
    worst = max(_ratio(abs(got[b, k] - want[b, k]), scale[b, k], GRID * n[b, k]) for b in range(got.shape[0]) for k in range(K) if n[b, k])
    print("%s: sel_sum worst ratio %.3f" % (_id(case), worst))
    assert (np.abs(got - want) <= GRID * n + C_BOUND[regime] * scale).all()
    assert not stats[:, Cf.OFF_SEL_CNT + K:Cf.OFF_SEL_SUM].any() and not stats[:, Cf.OFF_SEL_SUM + K:Cf.OFF_SUM_ALL].any()


@pytest.mark.parametrize("case", FINITE, ids=_id)
def test_soft_metric(lib, case):
    """ams_k_upsample_soft_metric: the integer rows are exactly what NumPy forms from the kernel's own p and ce maps with the REFERENCE labels
    (M_stu's columns: the argmax inside this kernel is first_maximum); p within 1e-5 of f64; ce per pixel and ce_sum within the bound."""
    regime, (h, w, H, W), NC, cls, grid = case
    logits, teacher, tl = LG.material(*case)[:3]
    r = _reference(logits, teacher, tl, cls, H, W, _key(case))
    stats, p, ce = _soft(lib, logits, cls, H, W, teacher, tl)
    assert np.array_equal(stats, SM.stats_rows(p, ce, r.labels, cls, teacher))
    assert np.array_equal(stats[:, 0], r.valid.sum(axis=(1, 2)))
    assert float(np.abs(p - r.pt).max()) < 1e-5
    per_pixel = float((np.abs(ce - r.ce_soft) / r.scale).max())
    n = r.valid.sum(axis=(1, 2))
    want = np.array([r.ce_soft[b][r.valid[b]].sum() for b in range(len(n))])
    scale = np.array([r.scale[b][r.valid[b]].sum() for b in range(len(n))])
    got = stats[:, 1] / Q
    worst = max(_ratio(abs(got[b] - want[b]), scale[b], GRID * n[b]) for b in range(len(n)))
    print("%s: soft ce per pixel worst ratio %.3f, ce_sum worst ratio %.3f" % (_id(case), per_pixel, worst))
    assert (np.abs(ce - r.ce_soft) <= C_BOUND[regime] * r.scale).all()
    assert (np.abs(got - want) <= GRID * n + C_BOUND[regime] * scale).all()


# ---------------------------------------------------------------------------------------------------- non-finite logits
def _teachers(teacher, affected, cls):
    """(the teacher with every affected pixel ignored, the teacher with every affected pixel valid)"""
    ignored = np.where(affected, 255, teacher).astype(np.uint8)
    yy, xx = np.indices(teacher.shape[1:])
    fill = np.asarray(cls, dtype=np.uint8)[(yy + xx) % len(cls)]
    valid = np.where(affected & ~np.isin(teacher, cls), fill[None], teacher).astype(np.uint8)
    return ignored, valid


@pytest.mark.parametrize("case", NONFINITE, ids=_id)
def test_nonfinite_labels_and_metrics(lib, case):
    """ams_k_upsample_argmax on a frame with NaN and infinite logits: labels by the rule at every pixel; frame 1 as in a call of its own.  With
    the teacher ignoring the affected pixels the metrics are those of the call on the replaced logits, bit for bit, and the sum of the two
    frames' own calls (every sum is exact).  With the affected pixels valid they are counted in loss[1] and the confusion matrix, and loss[0]
    is not finite."""
    regime, (h, w, H, W), NC, cls, grid = case
    logits, teacher, tl, affected, replaced = LG.material(*case)
    ignored, valid = _teachers(teacher, affected, cls)
    r = _reference(logits, valid, None, cls, H, W)
    with np.errstate(invalid="ignore"):
        assert (r.labels != np.argmax(r.z, -1)).any()
    labels, conf, loss = _argmax(lib, logits, cls, H, W, valid)
    assert np.array_equal(labels, r.labels)
    assert np.array_equal(conf, r.cm) and loss[1] == r.valid.sum() and not np.isfinite(loss[0])
    labels_i, conf_i, loss_i = _argmax(lib, logits, cls, H, W, ignored)
    _l, conf_r, loss_r = _argmax(lib, replaced, cls, H, W, ignored)
    assert np.array_equal(labels_i, r.labels)
    assert np.array_equal(conf_i, conf_r) and np.array_equal(loss_i.view(np.int64), loss_r.view(np.int64)) and np.isfinite(loss_i).all()
    ri = _reference(replaced, ignored, None, cls, H, W)
    assert np.array_equal(conf_i, ri.cm) and loss_i[1] == ri.valid.sum()
    err, scale = abs(loss_i[0] / loss_i[1] - ri.ce[ri.valid].mean()), ri.scale[ri.valid].mean()
    print("%s: mean loss off by %.3e = grid + %.3f units" % (_id(case), err, _ratio(err, scale)))
    assert err <= GRID + C_BOUND[regime] * scale
    alone = [_argmax(lib, logits[b:b + 1], cls, H, W, ignored[b:b + 1]) for b in range(2)]
    assert np.array_equal(alone[1][0][0], labels[1]) and np.array_equal(alone[0][0][0], labels[0])
    assert np.array_equal(conf_i, alone[0][1] + alone[1][1]) and loss_i[0] == alone[0][2][0] + alone[1][2][0] and loss_i[1] == alone[0][2][1] + alone[1][2][1]


@pytest.mark.parametrize("case", NONFINITE, ids=_id)
def test_nonfinite_confidence(lib, case):
    """ams_k_upsample_confidence on the same frames: p is a NaN exactly where an interpolated logit is; frame 1's maps and row are those of a
    call of its own.  Teacher ignoring the affected pixels: the teacher's fields are those of the call on the replaced logits.  Affected pixels
    valid: hist, hist_valid, hist_hit, bin_sum, sel_cnt and sum_all equal what NumPy forms from the kernel's own map with a NaN p in bin 0
    adding 0 (include/ams_hip.h) and the labels of the rule; sel_sum takes 0 from a loss that is not finite."""
    regime, (h, w, H, W), NC, cls, grid = case
    K = len(cls)
    logits, teacher, tl, affected, replaced = LG.material(*case)
    ignored, valid = _teachers(teacher, affected, cls)
    r = _reference(logits, valid, None, cls, H, W)
    u8, f32, stats = _confidence(lib, logits, cls, H, W, valid)
    nan = np.isnan(f32)
    assert np.array_equal(nan, np.isnan(r.z).any(-1)) and nan[0].any() and not nan[1].any()
    assert not (nan & ~affected).any() and (u8[nan] == 0).all()
    ok = ~nan
    assert (f32[ok] > 0).all() and (f32[ok] <= 1).all() and np.array_equal(u8[ok], np.rint(f32[ok] * np.float32(255)).astype(np.uint8))
    clean = r.finite
    assert float(np.abs(f32[clean].astype(np.float64) - r.p[clean]).max()) < 1e-5
    own = _own_rows(f32, r.labels, cls, valid)
    for b in range(2):
        for name, lo, n in _INT_FIELDS:
            assert np.array_equal(stats[b, lo:lo + n], own[b, lo:lo + n]), (b, name)
        assert stats[b, :NB].sum() == H * W and stats[b, NB:2 * NB].sum() == r.valid[b].sum()
    assert stats[0, 0] >= nan[0].sum() > 0
    assert stats[0, Cf.OFF_SUM_ALL] == int(np.rint(f32[0][ok[0]].astype(np.float64) * Q).sum())
    with np.errstate(invalid="ignore"):
        ce = np.where(np.isfinite(r.ce), r.ce, 0.0)
    want, scale, n = _sel_reference(r, K, ce)
    got = stats[:, Cf.OFF_SEL_SUM:Cf.OFF_SEL_SUM + K] / Q
    assert (stats[:, Cf.OFF_SEL_SUM:Cf.OFF_SEL_SUM + K] >= 0).all()
    assert (np.abs(got - want) <= GRID * n + C_BOUND[regime] * scale).all()
    # frame 1 in a call of its own
    u8_1, f32_1, stats_1 = _confidence(lib, logits[1:], cls, H, W, valid[1:])
    assert np.array_equal(u8_1[0], u8[1]) and np.array_equal(f32_1[0].view(np.uint32), f32[1].view(np.uint32)) and np.array_equal(stats_1[0], stats[1])
    # the teacher ignores the affected pixels: its fields are those of the replaced logits
    stats_i = _confidence(lib, logits, cls, H, W, ignored)[2]
    stats_r = _confidence(lib, replaced, cls, H, W, ignored)[2]
    for name, lo, n in (("hist_valid", NB, NB), ("hist_hit", 2 * NB, NB), ("bin_sum", 3 * NB, NB), ("sel_cnt", Cf.OFF_SEL_CNT, Cf.MAX_K),
                        ("sel_sum", Cf.OFF_SEL_SUM, Cf.MAX_K)):
        assert np.array_equal(stats_i[:, lo:lo + n], stats_r[:, lo:lo + n]), name
    assert np.array_equal(stats_i[1], stats_r[1]) and not np.array_equal(stats_i[0, :NB], stats_r[0, :NB])
