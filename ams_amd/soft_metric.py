"""Evaluation of the soft-teacher objective without an optimisation step (k_soft_metric.hip): host side.

A student graph built with ``soft_teacher=True`` minimises the cross-entropy against the teacher's distribution over the selected classes
(reference utils/graph_utils.py:375-376, 403-408), and the reference defines two metrics on that distribution, ``prob_confmat`` and
``prob_confmat_star`` (utils/graph_utils.py:265-317).  The device kernel leaves one row of integer statistics per frame; ``SoftMetric``
reads such a row (or a sum of rows), ``soft_metric_reference`` restates the reference's definitions in NumPy f64.

A row (int64, ``stats_len(K)`` = 2 + 2 K K entries)::

    valid_cnt | ce_sum | M_stu[K * K] | M_star[K * K]

``valid_cnt`` counts the pixels whose hard teacher id is in the class subset (every pixel without teacher ids), ``ce_sum`` adds their
``rint(ce * 2**20)``; ``M_stu[c * K + i]`` adds ``rint(p_c * 2**20)`` over the valid pixels the student labels i, ``M_star[c * K + i]`` over
those the teacher's own hard label is i: rows are the probability class, columns the label (``mat`` after the ``reduce_sum`` of
utils/graph_utils.py:296-298 and :307-308).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np

from .confidence import interpolate_selected

MAX_K = 32                   # classes a subset can hold (kMaxK)
FIXED = float(1 << 20)       # p and the pixel loss enter the sums as integer multiples of 2^-20


def stats_len(K: int) -> int:
    """entries of a statistics row for a subset of K classes (ams_soft_metric_stats_len)"""
    assert 1 <= K <= MAX_K
    return 2 + 2 * K * K


def _soft_iou(mat: np.ndarray) -> np.ndarray:
    tp = np.diag(mat)
    with np.errstate(invalid="ignore", divide="ignore"):
        return tp / (mat.sum(axis=1) + mat.sum(axis=0) - tp)             # utils/graph_utils.py:279-282


class SoftMetric(NamedTuple):
    valid: int                          # pixels that count (weight != 0)
    loss_soft: float                    # the soft-teacher loss: mean pixel loss over them (NaN without one, as tf.reduce_mean of nothing)
    prob_conf_student: np.ndarray       # f64 [K,K]: prob_confmat_star's mat_stu ([c, i]: teacher probability of c where the student says i)
    prob_conf_teacher: np.ndarray       # f64 [K,K]: its mat_star ([c, i]: ... where the teacher's hard label is i)
    soft_iou: np.ndarray                # f64 [K]: tp / (row + col - tp) of prob_conf_student
    soft_miou: float                    # its mean (tf.reduce_mean: NaN as soon as one class has no mass)
    row: np.ndarray                     # the int64 row (or sum of rows) this was decoded from

    @classmethod
    def decode(cls, row, K: Optional[int] = None) -> "SoftMetric":
        """``row``: one int64 statistics row, or a sum of such rows.  ``K``: size of the class subset (default: what the row's length says)."""
        row = np.asarray(row, dtype=np.int64).reshape(-1)
        if K is None:
            K = int(round(np.sqrt(max(0, row.size - 2) / 2.0)))
        assert row.size == stats_len(K), "a statistics row for %d classes has %d entries, got %d" % (K, stats_len(K), row.size)
        valid = int(row[0])
        m_stu = row[2:2 + K * K].reshape(K, K) / FIXED
        m_star = row[2 + K * K:].reshape(K, K) / FIXED
        iou = _soft_iou(m_stu)
        return cls(valid, float(row[1]) / FIXED / valid if valid else float("nan"), m_stu, m_star, iou, float(np.mean(iou)), row)

    @classmethod
    def sum(cls, rows) -> "SoftMetric":
        """The metric of several frames or passes: ``rows`` (int64 rows of one length, or ``SoftMetric`` objects decoded from rows) are added
        as integers before anything is divided."""
        rows = [r.row if isinstance(r, SoftMetric) else r for r in rows]
        total = np.sum(np.asarray(rows, dtype=np.int64).reshape(len(rows), -1), axis=0, dtype=np.int64)
        return cls.decode(total)


def interpolate_teacher(teacher_logits, class_indices: Sequence[int], H: int, W: int) -> np.ndarray:
    """f32 [B,H,W,K]: the selected classes' teacher logits at the label size.  Logits that come at that size are gathered as they are; a
    smaller grid is interpolated as the student's own logits are (a pixel on a grid point takes the grid's value itself)."""
    t = np.asarray(teacher_logits, dtype=np.float32)
    sel = np.asarray(class_indices, dtype=np.int64)
    if t.shape[1:3] == (H, W):
        return np.ascontiguousarray(t[..., sel])
    from .confidence import _taps
    z = interpolate_selected(t, class_indices, H, W)
    y0, _, ty = _taps(t.shape[1], H)
    x0, _, tx = _taps(t.shape[2], W)
    on_grid = (ty == 0)[:, None] & (tx == 0)[None, :]
    return np.where(on_grid[None, :, :, None], t[:, y0][:, :, x0][..., sel], z)


def stats_rows(p, ce, arg, class_indices: Sequence[int], teacher_ids=None) -> np.ndarray:
    """int64 [B, stats_len(K)]: the kernel's integer rows from per-pixel maps ``p`` f32 [B,H,W,K] and ``ce`` f32 [B,H,W], the predictions
    ``arg`` [B,H,W] and, with ``teacher_ids`` uint8 [B,H,W], the mask and the teacher's reduced labels.  A valid pixel whose ``ce`` is not
    finite is counted and adds nothing else (a NaN in either logit vector makes it so)."""
    p = np.asarray(p, dtype=np.float32)
    ce = np.asarray(ce, dtype=np.float32)
    B, K = p.shape[0], len(class_indices)
    rows = np.zeros((B, stats_len(K)), dtype=np.int64)
    target = None
    if teacher_ids is not None:
        lut = np.full(256, -1, dtype=np.int64)
        lut[np.asarray(class_indices, dtype=np.int64)] = np.arange(K)
        target = lut[np.asarray(teacher_ids, dtype=np.int64)]
    for b in range(B):
        valid = target[b] >= 0 if target is not None else np.ones(ce[b].shape, dtype=bool)
        ok = valid & np.isfinite(ce[b])
        with np.errstate(invalid="ignore"):
            pf = np.rint(p[b][ok].astype(np.float64) * FIXED).astype(np.int64)          # [n, K]
            cf = np.rint(ce[b][ok].astype(np.float64) * FIXED).astype(np.int64)
        rows[b, 0] = int(valid.sum())
        rows[b, 1] = int(cf.sum())
        labels = [np.asarray(arg[b])[ok]] + ([target[b][ok]] if target is not None else [])
        for plane, lab in enumerate(labels):
            m = np.zeros((K, K), dtype=np.int64)
            for i in range(K):
                m[:, i] = pf[lab == i].sum(axis=0)
            rows[b, 2 + plane * K * K:2 + (plane + 1) * K * K] = m.reshape(-1)
    return rows


def soft_metric_reference(student_logits_lowres, teacher_logits, teacher_ids, class_indices: Sequence[int], H: int, W: int):
    """NumPy f64 restatement of the reference's soft-teacher loss and of prob_confmat / prob_confmat_star (utils/graph_utils.py:265-317,
    375-376, 397, 403-408), hand-derived from that text: TensorFlow is not available to this project, so no run of the reference pins it.

    ``student_logits_lowres`` f32 [B,h,w,C], ``teacher_logits`` f32 [B,th,tw,C], ``teacher_ids`` uint8 [B,H,W] or None (prob_confmat's
    unmasked form: every pixel counts and the teacher matrix is zero).  Both logit tensors are brought to [B,H,W,K] in f32 with the
    kernels' arithmetic (as ``confidence.confidence_reference`` does); everything after that is f64.

    Returns ``(metric, p, ce, arg)``: a ``SoftMetric`` over all B frames with f64 fields (``row`` is None: nothing was rounded), ``p`` f64
    [B,H,W,K] = softmax of the teacher logits, ``ce`` f64 [B,H,W] = sum_k p_k (logsumexp(z) - z_k), ``arg`` int32 [B,H,W] the student's labels."""
    K = len(class_indices)
    z = interpolate_selected(student_logits_lowres, class_indices, H, W)
    t = interpolate_teacher(teacher_logits, class_indices, H, W)
    arg = np.argmax(z, axis=-1).astype(np.int32)                         # filtered_predictions (first maximum)
    z64, t64 = z.astype(np.float64), t.astype(np.float64)
    e = np.exp(t64 - t64.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)                                # filtered_teacher_labels_probs
    zmax = z64.max(axis=-1, keepdims=True)
    lse = zmax + np.log(np.exp(z64 - zmax).sum(axis=-1, keepdims=True))
    ce = (p * (lse - z64)).sum(axis=-1)                                  # softmax_cross_entropy_with_logits(logits=z, labels=p)
    if teacher_ids is not None:
        lut = np.full(256, -1, dtype=np.int64)
        lut[np.asarray(class_indices, dtype=np.int64)] = np.arange(K)
        target = lut[np.asarray(teacher_ids, dtype=np.int64)]            # filtered_labels where weights != 0
        valid = target >= 0
    else:
        target, valid = None, np.ones(arg.shape, dtype=bool)
    m_stu = np.zeros((K, K))
    m_star = np.zeros((K, K))
    for i in range(K):
        m_stu[:, i] = p[valid & (arg == i)].sum(axis=0)
        if target is not None:
            m_star[:, i] = p[valid & (target == i)].sum(axis=0)
    n = int(valid.sum())
    iou = _soft_iou(m_stu)
    loss = float(ce[valid].mean()) if n else float("nan")
    return SoftMetric(n, loss, m_stu, m_star, iou, float(np.mean(iou)), None), p, ce, arg
