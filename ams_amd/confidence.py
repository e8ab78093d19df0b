"""The student's own certainty on the edge (k_confidence.hip): host side.

``create_student_v3`` returns ``probabilities_reduced`` (per pixel the maximum of the softmax over the selected classes) and ``loss_sel``
(the selective loss) next to the labels (reference utils/graph_utils.py:388-389, 410-418).  The device kernel leaves the map and one row
of integer statistics per frame; ``ConfidenceStats`` reads such a row, ``confidence_reference`` restates the kernel in NumPy.

A row (int64, ``STATS_LEN`` entries)::

    hist[NB] | hist_valid[NB] | hist_hit[NB] | bin_sum[NB] | sel_cnt[32] | sel_sum[32] | sum_all

``hist`` counts every pixel by ``bin = min(NB - 1, int(p * NB))`` and ``sum_all`` adds their ``rint(p * 2**20)``; the other fields cover the
pixels whose teacher label is in the class subset: their number per bin, those whose prediction is the teacher's class, their summed
``rint(p * 2**20)``, and per class k the pixels whose teacher class or prediction is k with their summed ``rint(CE * 2**20)``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

NB = 32                      # AMS_CONFIDENCE_BINS
MAX_K = 32                   # classes a subset can hold (kMaxK)
FIXED = float(1 << 20)       # p and the pixel loss enter the sums as integer multiples of 2^-20
OFF_SEL_CNT = 4 * NB
OFF_SEL_SUM = OFF_SEL_CNT + MAX_K
OFF_SUM_ALL = OFF_SEL_SUM + MAX_K
STATS_LEN = OFF_SUM_ALL + 1


class ConfidenceStats:
    """One frame's statistics row.  ``n_classes``: size of the class subset (the per-class fields are cut to it).

    Without teacher labels only ``mean``, ``hist`` and ``low_fraction`` carry information; ``has_teacher`` tells.  The calibration figures
    (``accuracy_by_bin``, ``ece``) measure the student against the TEACHER, which exists only in the emulation: a deployed edge has ``hist``."""

    def __init__(self, row, n_classes: int = MAX_K):
        row = np.asarray(row, dtype=np.int64).reshape(-1)
        assert row.size == STATS_LEN, "a statistics row has %d entries, got %d" % (STATS_LEN, row.size)
        assert 1 <= n_classes <= MAX_K
        self.row = row
        self.n_classes = int(n_classes)
        self.hist = row[:NB]
        self.hist_valid = row[NB:2 * NB]
        self.hist_hit = row[2 * NB:3 * NB]
        self.bin_sum = row[3 * NB:4 * NB]
        self.sel_cnt = row[OFF_SEL_CNT:OFF_SEL_CNT + self.n_classes]
        self.sel_sum = row[OFF_SEL_SUM:OFF_SEL_SUM + self.n_classes]
        self.sum_all = int(row[OFF_SUM_ALL])

    @property
    def n_pixels(self) -> int:
        return int(self.hist.sum())

    @property
    def n_valid(self) -> int:
        return int(self.hist_valid.sum())

    @property
    def has_teacher(self) -> bool:
        return self.n_valid > 0

    @property
    def mean(self) -> float:
        """mean confidence over all pixels (label-free)"""
        n = self.n_pixels
        return self.sum_all / (n * FIXED) if n else float("nan")

    def low_fraction(self, threshold: float) -> float:
        """Share of the pixels with p below ``threshold``, which snaps to the nearest bin edge k / NB (the histogram is all there is)."""
        n = self.n_pixels
        edge = min(NB, max(0, int(round(float(threshold) * NB))))
        return float(self.hist[:edge].sum()) / n if n else float("nan")

    @property
    def accuracy_by_bin(self) -> np.ndarray:
        """hit / valid pixels per bin (NaN where a bin holds no valid pixel)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.hist_valid > 0, self.hist_hit / self.hist_valid.astype(np.float64), np.nan)

    @property
    def confidence_by_bin(self) -> np.ndarray:
        """mean confidence of the valid pixels per bin (NaN where a bin holds none)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.hist_valid > 0, self.bin_sum / (self.hist_valid * FIXED), np.nan)

    @property
    def ece(self) -> float:
        """expected calibration error against the teacher: sum_b n_b / N |hit_b / n_b - bin_sum_b / (n_b 2^20)| over the non-empty bins"""
        n = self.n_valid
        if not n:
            return float("nan")
        m = self.hist_valid > 0
        nb = self.hist_valid[m].astype(np.float64)
        return float(np.sum(nb / n * np.abs(self.hist_hit[m] / nb - self.bin_sum[m] / (nb * FIXED))))

    @property
    def loss_sel_by_class(self) -> np.ndarray:
        """per class k the mean pixel loss over the valid pixels whose teacher class or prediction is k (NaN for a class without one)"""
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(self.sel_cnt > 0, self.sel_sum / (self.sel_cnt * FIXED), np.nan)

    @property
    def loss_sel(self) -> float:
        """The reference's selective loss: the SUM over the classes of ``loss_sel_by_class``.  It is NaN as soon as ONE class of the subset has
        no pixel in the frame (``sel_cnt == 0``): ``tf.reduce_mean`` of an empty ``boolean_mask`` is NaN and the sum keeps it
        (utils/graph_utils.py:410-418).  ``loss_sel_by_class`` is the usable form."""
        return float(np.sum(self.loss_sel_by_class))


class Confidence:
    """What ``SemanticNetwork.predict_with_confidence`` adds to its result: ``map`` the uint8 device tensor [B,H,W] (rint(p * 255)) and
    ``stats`` one ``ConfidenceStats`` per frame."""

    def __init__(self, map_u8, stats: List[ConfidenceStats]):
        self.map = map_u8
        self.stats = stats

    def host(self) -> np.ndarray:
        """the map as a uint8 ndarray [B,H,W] (one copy; synchronises)"""
        return self.map.cpu().numpy()


def _taps(n_in: int, n_out: int):
    """ResizeBilinear with align_corners in f32, as the head kernels form it: (lower tap, upper tap, weight of the upper tap)"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    src = np.arange(n_out, dtype=np.float32) * scale
    fl = np.floor(src)
    lo = fl.astype(np.int64)
    return lo, np.minimum(lo + 1, n_in - 1), (src - fl).astype(np.float32)


def interpolate_selected(logits_lowres, class_indices: Sequence[int], H: int, W: int) -> np.ndarray:
    """f32 [B,H,W,K]: the selected classes' logits at full resolution, each operation rounded to f32 in the kernels' order (horizontal, then
    vertical, unfused), so the argmax of the result is the device's label map bit for bit."""
    z = np.asarray(logits_lowres, dtype=np.float32)[..., np.asarray(class_indices, dtype=np.int64)]
    y0, y1, ty = _taps(z.shape[1], H)
    x0, x1, tx = _taps(z.shape[2], W)
    tx = tx[None, None, :, None]
    ty = ty[None, :, None, None]
    rows0, rows1 = z[:, y0], z[:, y1]
    top = rows0[:, :, x0] + (rows0[:, :, x1] - rows0[:, :, x0]) * tx
    bot = rows1[:, :, x0] + (rows1[:, :, x1] - rows1[:, :, x0]) * tx
    return top + (bot - top) * ty


def stats_rows(p, arg, class_indices: Sequence[int], teacher=None, ce=None) -> np.ndarray:
    """int64 [B, STATS_LEN]: the kernel's integer statistics from a confidence map ``p`` [B,H,W] (f32: its bins and fixed-point values are
    formed with the kernel's f32 arithmetic), the predictions ``arg`` and, with ``teacher`` uint8 [B,H,W], the per-pixel loss ``ce``."""
    p = np.asarray(p, dtype=np.float32)
    B = p.shape[0]
    K = len(class_indices)
    lut = np.full(256, -1, dtype=np.int64)
    lut[np.asarray(class_indices, dtype=np.int64)] = np.arange(K)
    rows = np.zeros((B, STATS_LEN), dtype=np.int64)
    bins = np.minimum(NB - 1, (p * np.float32(NB)).astype(np.int64))
    pf = np.rint(p.astype(np.float64) * FIXED).astype(np.int64)
    for b in range(B):
        rows[b, :NB] = np.bincount(bins[b].ravel(), minlength=NB)
        rows[b, OFF_SUM_ALL] = pf[b].sum()
        if teacher is None:
            continue
        target = lut[np.asarray(teacher[b], dtype=np.int64)]
        valid = target >= 0
        hit = valid & (arg[b] == target)
        rows[b, NB:2 * NB] = np.bincount(bins[b][valid], minlength=NB)
        rows[b, 2 * NB:3 * NB] = np.bincount(bins[b][hit], minlength=NB)
        rows[b, 3 * NB:4 * NB] = np.bincount(bins[b][valid], weights=pf[b][valid].astype(np.float64), minlength=NB).astype(np.int64)
        cf = np.rint(np.asarray(ce[b], dtype=np.float64) * FIXED).astype(np.int64)
        for k in range(K):
            m = valid & ((target == k) | (arg[b] == k))
            rows[b, OFF_SEL_CNT + k] = int(m.sum())
            rows[b, OFF_SEL_SUM + k] = int(cf[m].sum())
    return rows


def confidence_reference(logits_lowres, class_indices: Sequence[int], H: int, W: int, teacher: Optional[np.ndarray] = None):
    """NumPy restatement of k_confidence.hip.  ``logits_lowres`` f32 [B,h,w,C], ``teacher`` uint8 [B,H,W] or None.

    Returns ``(p, rows, arg)``: ``p`` the f64 confidence map [B,H,W] — the f64 softmax maximum of the f32-interpolated logits —, ``rows`` the
    int64 statistics [B, STATS_LEN] formed from ``p`` rounded to f32 and the f64 pixel loss, ``arg`` the int32 predictions [B,H,W] (first maximum).
    The device evaluates the exponentials in f32, so its map differs from ``p`` at f32 level and a pixel next to a bin edge may fall on its other side."""
    z = interpolate_selected(logits_lowres, class_indices, H, W)
    arg = np.argmax(z, axis=-1).astype(np.int32)
    z64 = z.astype(np.float64)
    zmax = z64.max(axis=-1)
    ssum = np.exp(z64 - zmax[..., None]).sum(axis=-1)
    p = 1.0 / ssum
    ce = None
    if teacher is not None:
        lut = np.full(256, -1, dtype=np.int64)
        lut[np.asarray(class_indices, dtype=np.int64)] = np.arange(len(class_indices))
        target = lut[np.asarray(teacher, dtype=np.int64)]
        zt = np.take_along_axis(z64, np.maximum(target, 0)[..., None], axis=-1)[..., 0]
        ce = (zmax + np.log(ssum)) - zt
    return p, stats_rows(p.astype(np.float32), arg, class_indices, teacher, ce), arg
