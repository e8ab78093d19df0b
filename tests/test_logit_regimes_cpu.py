"""The regimes of tests/logit_regimes.py are what they say, at every (regime, shape, subset) the GPU suites run: conditions on the inputs, asserted
on the f32 restatement of the interpolation (ams_amd.confidence.interpolate_selected), so that no GPU test of them can pass hollow."""
import numpy as np
import pytest

import logit_regimes as LG
from ams_amd.confidence import _taps, interpolate_selected

CASES = LG.cases()


def _id(c):
    regime, shape, NC, cls, grid = c
    return "%s-%s-K%d-t%dx%d" % (regime, "x".join(map(str, shape)), len(cls), grid[0], grid[1])


def _of(regime):
    return pytest.mark.parametrize("case", [c for c in CASES if c[0] == regime], ids=_id)


def _softmax64(z):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _targets(teacher, cls):
    lut = np.full(256, -1)
    lut[cls] = np.arange(len(cls))
    return lut[teacher]


def test_first_maximum_is_argmax_on_finite_input_and_the_kernels_rule_on_nan():
    rng = np.random.default_rng(0)
    z = (rng.integers(-3, 4, (4000, 7)) * 0.5).astype(np.float32)           # many ties
    z[::5, 2] = -0.0
    z[1::5, 2] = 0.0
    assert np.array_equal(LG.first_maximum(z), np.argmax(z, -1)) and LG.tied(z).mean() > 0.2
    nan = np.float32(np.nan)
    assert LG.first_maximum(np.array([nan, 5.0, 7.0], dtype=np.float32)) == 0          # a NaN in class 0 keeps label 0
    assert LG.first_maximum(np.array([1.0, nan, 0.5], dtype=np.float32)) == 0          # elsewhere it never wins
    assert LG.first_maximum(np.array([1.0, nan, 2.0, 2.0], dtype=np.float32)) == 2
    assert LG.first_maximum(np.array([-0.0, 0.0], dtype=np.float32)) == 0 and LG.first_maximum(np.array([0.0, -0.0], dtype=np.float32)) == 0
    assert LG.first_maximum(np.array([-np.inf, -np.inf], dtype=np.float32)) == 0 and LG.first_maximum(np.array([1.0, np.inf], dtype=np.float32)) == 1
    assert np.array_equal(LG.last_maximum(np.array([[1.0, 3.0, 3.0, 0.0]])), [2])


def test_generators_are_deterministic():
    a = LG.ties(5, 9, 32, 64, 19, LG.SUB6, 9, 17, seed=4)
    b = LG.ties(5, 9, 32, 64, 19, LG.SUB6, 9, 17, seed=4)
    c = LG.saturated(5, 9, 32, 64, 19, LG.SUB6, 9, 17, seed=4)
    d = LG.saturated(5, 9, 32, 64, 19, LG.SUB6, 9, 17, seed=4)
    assert all(np.array_equal(x, y) for x, y in zip(a + c, b + d))
    assert a[0].dtype == np.float32 and a[1].dtype == np.uint8 and a[2].dtype == np.float32 and a[2].shape == (2, 9, 17, 19)


@_of("ties")
def test_ties(case):
    _, (h, w, H, W), NC, cls, (th, tw) = case
    K = len(cls)
    logits, teacher, tl = LG.material(*case)
    assert logits.shape == (2, h, w, NC) and teacher.shape == (2, H, W) and tl.shape == (2, th, tw, NC)
    z = interpolate_selected(logits, cls, H, W)
    assert np.isfinite(z).all() and np.array_equal(LG.first_maximum(z), np.argmax(z, -1))
    t = LG.tied(z)
    assert t.mean() >= 0.2, t.mean()
    lo, hi = LG.first_maximum(z), LG.last_maximum(z)
    tgt = _targets(teacher, cls)
    assert (t & (tgt == lo)).sum() > 0 and (t & (tgt == hi) & (hi > lo)).sum() > 0
    assert 0.05 < (teacher == 255).mean() < 0.15
    # two pairs and a triple as the maximum, by the number of classes at the maximum and the lower index (frame 0)
    n_max = (z == z.max(-1, keepdims=True)).sum(-1)
    assert ((n_max[0] == 2) & (lo[0] == 0) & (hi[0] == 1)).any() and ((n_max[0] == 2) & (lo[0] == 2) & (hi[0] == 3)).any()
    assert ((n_max[0] == 3) & (lo[0] == 2) & (hi[0] == 4)).any()
    # the plateau: every class equal, the f32 read-out's values exact (frame 1)
    plateau = n_max[1] == K
    assert plateau.any() and (lo[1][plateau] == 0).all()
    # both signed-zero orders: cells that hold (-0, +0) and cells that hold (+0, -0) in the pair, and pixels fed by either kind alone
    # whose maximum is the pair, tied at 0
    a, b = logits[1, :, :, cls[1]], logits[1, :, :, cls[4]]
    order1 = (a == 0) & np.signbit(a) & (b == 0) & ~np.signbit(b)
    order2 = (a == 0) & ~np.signbit(a) & (b == 0) & np.signbit(b)
    y0, y1, _ = _taps(h, H)
    x0, x1, _ = _taps(w, W)
    for order in (order1, order2):
        assert order.any()
        fed = order[y0][:, x0] & order[y0][:, x1] & order[y1][:, x0] & order[y1][:, x1]
        assert fed.any() and (z[1][fed].max(-1) == 0).all() and (lo[1][fed] == 1).all() and (hi[1][fed] == 4).all()
    # the teacher logits carry ties as well, with an integer sum of exponentials in f32 at T = 1 and T = 2
    zt = interpolate_selected(tl, cls, H, W) if (th, tw) != (H, W) else tl[..., cls]
    assert LG.tied(zt).mean() >= 0.2
    for T in (1.0, 2.0):
        e = np.exp((zt - zt.max(-1, keepdims=True)) * np.float32(1 / T), dtype=np.float32).sum(-1, dtype=np.float32)
        whole = e == np.rint(e)
        assert (whole & (e >= 2)).mean() >= 0.2 and (e == K).any()


@_of("quantised")
def test_quantised(case):
    _, (h, w, H, W), NC, cls, _grid = case
    logits, teacher, tl = LG.material(*case)
    assert (h, w) == (H, W)
    z = interpolate_selected(logits, cls, H, W)
    assert np.array_equal(z, logits[..., cls])                              # the identity: the compared values are the samples themselves
    assert np.array_equal(logits * 2, np.rint(logits * 2)) and np.abs(logits).max() <= 4
    # 17 equally likely levels: the maximum of six classes is tied in 18 % of the pixels on average, of nineteen in 44 %; 90 pixels here
    assert LG.tied(z).mean() >= 0.1 and np.array_equal(LG.first_maximum(z), np.argmax(z, -1))


@_of("saturated")
def test_saturated(case):
    _, (h, w, H, W), NC, cls, (th, tw) = case
    logits, teacher, tl = LG.material(*case)
    z = interpolate_selected(logits, cls, H, W)
    assert np.isfinite(z).all()
    p = _softmax64(z)
    pmax = p.max(-1)
    assert (pmax >= 1 - 2.0 ** -25).mean() >= 0.25, (pmax >= 1 - 2.0 ** -25).mean()
    assert ((pmax > 0.5) & (pmax < 0.99)).mean() >= 0.05, ((pmax > 0.5) & (pmax < 0.99)).mean()
    assert (p < 2.0 ** -149).any()
    arg = LG.first_maximum(z)
    tgt = _targets(teacher, cls)
    valid = tgt >= 0
    assert (valid & (tgt == arg)).mean() > 0.2 and (valid & (tgt != arg)).mean() > 0.2 and 0 < (~valid).mean() < 0.2
    # cls[0] wins nowhere in frame 1 and lies far below the maximum there (at a crossing the maximum itself dips)
    assert (arg[1] != 0).all() and ((z[1].max(-1) - z[1][..., 0]) > 30).mean() >= 0.25
    zt = interpolate_selected(tl, cls, H, W) if (th, tw) != (H, W) else tl[..., cls]
    pt = _softmax64(zt).max(-1)
    assert (pt >= 1 - 2.0 ** -25).mean() >= 0.25
    differ = (LG.first_maximum(zt) != arg).mean()
    assert 0.1 < differ < 0.6, differ


@_of("nonfinite")
def test_nonfinite(case):
    _, (h, w, H, W), NC, cls, (th, tw) = case
    logits, teacher, tl, affected, replaced = LG.material(*case)
    assert np.isfinite(logits[1]).all() and np.isfinite(tl).all() and np.isfinite(replaced).all()
    # a cell's pixels are two of the grid's four row intervals by two of its eight column intervals, an eighth of the frame; the four sets
    # are disjoint: at least half of frame 0 stays out of reach of all four, and frame 1 whole
    assert affected[0].any() and not affected[1].any() and affected[0].mean() <= 0.5
    with np.errstate(invalid="ignore"):
        z = interpolate_selected(logits, cls, H, W)
    bad = ~np.isfinite(z).all(-1)
    assert bad.any() and not (bad & ~affected).any()
    with np.errstate(invalid="ignore"):
        assert (LG.first_maximum(z) != np.argmax(z, -1)).any()              # the rule is exercised: NumPy lets a NaN win anywhere
    cells = np.zeros((2, h, w), dtype=bool)
    prints = []
    for i, j, k, v in LG.NONFINITE_CELLS:
        cells[0, i, j] = True
        got = logits[0, i, j, cls[k]]
        assert (np.isnan(got) and np.isnan(v)) or got == v
        prints.append(LG.footprint(h, w, H, W, i, j))
    assert (~np.isfinite(logits)).sum() == 4
    # the four cells' pixels do not meet (the cells' own 3 x 3 neighbourhoods do, in row 2: no pixel taps rows 1 and 3 at once)
    assert (np.sum(prints, axis=0) <= 1).all() and np.array_equal(np.any(prints, axis=0), affected[0])
    assert np.array_equal(replaced[~cells].view(np.uint32), logits[~cells].view(np.uint32)) and not replaced[cells].any()
    # away from the affected pixels the two sets of logits interpolate to the same bits
    assert np.array_equal(interpolate_selected(replaced, cls, H, W)[~affected].view(np.uint32), z[~affected].view(np.uint32))
