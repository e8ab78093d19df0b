"""The host side of the soft-teacher evaluation (ams_amd/soft_metric.py): the NumPy restatement of prob_confmat / prob_confmat_star and the
soft loss against values worked out by hand, its one-hot limit against the hard metrics, and the fixed-point row.  No GPU."""
import numpy as np

from ams_amd import soft_metric as SM
from ams_amd.confidence import interpolate_selected
from ams_amd.utils import calculate_miou

LN2, LN3, LN4 = np.log(2.0), np.log(3.0), np.log(4.0)


def _hand_case():
    """2 x 3 pixels at the logits' own size (the interpolation is the identity), classes [0, 2] of 3.  Selected logits per pixel:

        pixel  teacher id   student z    label   teacher t    p
        0      0 -> 0       (ln3, 0)     0       (ln3, 0)     (3/4, 1/4)
        1      2 -> 1       (0, ln3)     1       (0, 0)       (1/2, 1/2)
        2      1 (outside)  (ln3, 0)     0       (ln3, 0)     (3/4, 1/4)
        3      255          (0, ln3)     1       (0, ln3)     (1/4, 3/4)
        4      2 -> 1       (ln3, 0)     0       (0, ln3)     (1/4, 3/4)
        5      0 -> 0       (0, 0)       0       (0, ln3)     (1/4, 3/4)       (a tie: the first maximum wins)
    """
    a = np.float32(LN3)
    z_sel = np.array([[a, 0], [0, a], [a, 0], [0, a], [a, 0], [0, 0]], dtype=np.float32)
    t_sel = np.array([[a, 0], [0, 0], [a, 0], [0, a], [0, a], [0, a]], dtype=np.float32)
    z = np.full((1, 2, 3, 3), 7.0, dtype=np.float32)          # class 1 is not selected: its logits must not matter
    t = np.full((1, 2, 3, 3), -5.0, dtype=np.float32)
    z[0, :, :, [0, 2]] = z_sel.reshape(2, 3, 2).transpose(2, 0, 1)
    t[0, :, :, [0, 2]] = t_sel.reshape(2, 3, 2).transpose(2, 0, 1)
    ids = np.array([[[0, 2, 1], [255, 2, 0]]], dtype=np.uint8)
    return z, t, ids


def test_hand_made_case_masked():
    z, t, ids = _hand_case()
    m, p, ce, arg = SM.soft_metric_reference(z, t, ids, [0, 2], 2, 3)
    assert arg.reshape(-1).tolist() == [0, 1, 0, 1, 0, 0]
    np.testing.assert_allclose(p.reshape(6, 2), [[.75, .25], [.5, .5], [.75, .25], [.25, .75], [.25, .75], [.25, .75]], atol=1e-7)
    assert m.valid == 4                                          # id 1 (outside the subset) and id 255 are excluded
    # rows = probability class, columns = label: column 0 of the student's matrix collects pixels 0, 4, 5, column 1 pixel 1
    np.testing.assert_allclose(m.prob_conf_student, [[.75 + .25 + .25, .5], [.25 + .75 + .75, .5]], atol=1e-6)
    # the teacher's own labels: column 0 pixels 0 and 5, column 1 pixels 1 and 4
    np.testing.assert_allclose(m.prob_conf_teacher, [[.75 + .25, .5 + .25], [.25 + .75, .5 + .75]], atol=1e-6)
    # ce = sum_k p_k (lse - z_k): pixel 0 ln4 - 3/4 ln3, pixel 1 ln4 - 1/2 ln3, pixel 4 ln4 - 1/4 ln3, pixel 5 ln2
    np.testing.assert_allclose(ce.reshape(-1)[[0, 1, 4, 5]], [LN4 - .75 * LN3, LN4 - .5 * LN3, LN4 - .25 * LN3, LN2], atol=1e-6)
    np.testing.assert_allclose(m.loss_soft, (3 * LN4 - 1.5 * LN3 + LN2) / 4, atol=1e-6)
    # tp / (row + col - tp): rows (1.75, 2.25), columns (3, 1), diagonal (1.25, 0.5)
    np.testing.assert_allclose(m.soft_iou, [1.25 / (1.75 + 3 - 1.25), .5 / (2.25 + 1 - .5)], atol=1e-6)
    np.testing.assert_allclose(m.soft_miou, np.mean([1.25 / 3.5, .5 / 2.75]), atol=1e-6)
    # the orientation is not symmetric here: a transposed matrix fails
    assert abs(m.prob_conf_student[0, 1] - m.prob_conf_student[1, 0]) > 1


def test_hand_made_case_unmasked():
    z, t, _ = _hand_case()
    m, _p, ce, _arg = SM.soft_metric_reference(z, t, None, [0, 2], 2, 3)
    assert m.valid == 6
    np.testing.assert_allclose(m.prob_conf_student, [[.75 + .75 + .25 + .25, .5 + .25], [.25 + .25 + .75 + .75, .5 + .75]], atol=1e-6)
    assert np.all(m.prob_conf_teacher == 0)
    np.testing.assert_allclose(m.loss_soft, ce.mean(), atol=1e-12)
    np.testing.assert_allclose(m.soft_iou, [2.0 / (2.75 + 4 - 2.0), 1.25 / (3.25 + 2 - 1.25)], atol=1e-6)


def test_rows_of_the_reference_maps_decode_to_the_reference():
    """stats_rows (the kernel's integer rule in NumPy) on the reference's own maps, decoded: the f64 figures to fixed-point accuracy"""
    z, t, ids = _hand_case()
    m, p, ce, arg = SM.soft_metric_reference(z, t, ids, [0, 2], 2, 3)
    d = SM.SoftMetric.decode(SM.stats_rows(p, ce, arg, [0, 2], ids)[0])
    assert d.valid == 4
    np.testing.assert_allclose(d.prob_conf_student, m.prob_conf_student, atol=4 * 2.0 ** -21 + 1e-6)
    np.testing.assert_allclose(d.prob_conf_teacher, m.prob_conf_teacher, atol=4 * 2.0 ** -21 + 1e-6)
    np.testing.assert_allclose(d.loss_soft, m.loss_soft, atol=2.0 ** -21 + 1e-6)


def test_one_hot_limit_is_the_hard_metric():
    rng = np.random.default_rng(3)
    ci = [0, 1, 2, 10, 11, 13]
    K, NC, H, W = len(ci), 19, 9, 17
    z = rng.normal(0, 2, (2, 3, 5, NC)).astype(np.float32)
    ids = rng.choice(np.array(ci + [5, 255], dtype=np.uint8), size=(2, H, W))
    t = np.zeros((2, H, W, NC), dtype=np.float32)
    inside = ids < NC
    t[inside, ids[inside]] = 60.0                                 # 60 * onehot(hard label); id 255 has no row
    m, _p, _ce, arg = SM.soft_metric_reference(z, t, ids, ci, H, W)
    lut = np.full(256, -1)
    lut[ci] = np.arange(K)
    target = lut[ids]
    valid = target >= 0
    conf = np.zeros((K, K))                                       # rows = teacher labels, columns = student predictions (calculate_miou)
    np.add.at(conf, (target[valid], arg[valid]), 1)
    np.testing.assert_allclose(m.prob_conf_student, conf, rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.prob_conf_teacher, np.diag(np.bincount(target[valid], minlength=K).astype(np.float64)), rtol=0, atol=1e-12)
    np.testing.assert_allclose(m.soft_iou, np.asarray(calculate_miou(conf, nan=True), dtype=np.float64), rtol=0, atol=1e-12)
    z64 = interpolate_selected(z, ci, H, W).astype(np.float64)
    zmax = z64.max(axis=-1)
    hard = (zmax + np.log(np.exp(z64 - zmax[..., None]).sum(axis=-1))) - np.take_along_axis(z64, np.maximum(target, 0)[..., None], axis=-1)[..., 0]
    assert abs(m.loss_soft - hard[valid].mean()) < 1e-12


def test_fixed_point_row():
    for K in (1, 6, 19, 32):
        assert SM.stats_len(K) == 2 + 2 * K * K
    one = 1 << 20
    # K = 2: valid | ce_sum | M_stu (row-major, [c, i]) | M_star
    row = np.array([4, 6 * one, 3 * one, one // 2, one, one // 4, 2 * one, 0, 0, 2 * one], dtype=np.int64)
    m = SM.SoftMetric.decode(row)
    assert m.valid == 4 and m.loss_soft == 1.5
    assert m.prob_conf_student.tolist() == [[3.0, 0.5], [1.0, 0.25]]
    assert m.prob_conf_teacher.tolist() == [[2.0, 0.0], [0.0, 2.0]]
    np.testing.assert_allclose(m.soft_iou, [3.0 / (3.5 + 4.0 - 3.0), 0.25 / (1.25 + 0.75 - 0.25)], rtol=1e-15)
    assert m.soft_miou == np.mean(m.soft_iou)
    assert SM.SoftMetric.decode(row, 2).row.tolist() == row.tolist()
    s = SM.SoftMetric.sum([row, row, m])
    assert s.row.tolist() == (3 * row).tolist() and s.valid == 12 and s.loss_soft == 1.5
    np.testing.assert_array_equal(s.prob_conf_student, 3 * m.prob_conf_student)
    empty = SM.SoftMetric.decode(np.zeros(SM.stats_len(6), dtype=np.int64))
    assert empty.valid == 0 and np.isnan(empty.loss_soft) and np.isnan(empty.soft_miou)
