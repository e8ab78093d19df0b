"""The guarded-buffer helper of the kernel tests (tests/guarded.py) on CPU tensors: each way a kernel can misuse a buffer is planted by a
stub "kernel" written here and must FAIL check(); a correct stub and an honoured untouched= mask must pass."""
import numpy as np
import pytest
import torch

import guarded

CPU = "cpu"


@pytest.fixture(autouse=True)
def _fresh():
    guarded.reset()
    yield
    guarded.reset()


def stub_fill(t, first, count, value=1.0):
    """a stub kernel: writes `count` elements from element `first` of t's result (negative or past the end: into the guards)"""
    w = guarded.whole(t)
    a = guarded.offset(t) + first
    w[a:a + count] = value


DTYPES = [torch.float32, torch.float64, torch.int16, torch.float16, torch.bfloat16, torch.uint8, torch.int32, torch.int64]


@pytest.mark.parametrize("dtype", DTYPES)
def test_fully_written_result_passes(dtype):
    y = guarded.out((3, 5, 7), dtype, device=CPU)
    assert y.shape == (3, 5, 7) and y.dtype == dtype and y.is_contiguous() and y.data_ptr() % 16 == 0
    assert bool(guarded.poisoned(y).all()), "the interior is poisoned too"
    assert guarded.pending() == [y] or guarded.pending()[0] is y
    stub_fill(y, 0, y.numel(), 1)
    guarded.check("stub")
    assert guarded.pending() == []


def test_patterns_are_the_documented_bits():
    assert guarded.whole(guarded.out(4, torch.float32, device=CPU)).view(torch.int32)[0].item() == 0x7FC12345
    for dt in (torch.int16, torch.float16, torch.bfloat16):
        w = guarded.whole(guarded.out(4, dt, device=CPU))
        assert w.view(torch.int16)[0].item() == 0x7FC1
        if dt != torch.int16:
            assert bool(torch.isnan(w.float()).all())
    assert guarded.whole(guarded.out(4, torch.uint8, device=CPU))[0].item() == 255
    assert guarded.whole(guarded.out(4, torch.int32, device=CPU))[0].item() == -0x12345679
    assert guarded.whole(guarded.out(4, torch.int64, device=CPU))[0].item() == -0x12345679
    assert bool(torch.isnan(guarded.whole(guarded.out(4, torch.float64, device=CPU))).all())
    guarded.reset()


def test_guard_is_at_least_4096_and_takes_the_callers_figure():
    with pytest.raises(AssertionError):
        guarded.out(8, guard=100, device=CPU)
    y = guarded.out(8, guard=5000, device=CPU)
    assert guarded.offset(y) >= 5000 and guarded.whole(y).numel() == 2 * guarded.offset(y) + 8
    guarded.reset()


@pytest.mark.parametrize("where", ["just_before", "just_behind", "far_front", "far_behind"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.int16, torch.uint8, torch.int32, torch.int64])
def test_a_write_into_a_guard_is_caught(where, dtype):
    n = 33
    y = guarded.out((n,), dtype, device=CPU)
    g = guarded.offset(y)
    stub_fill(y, 0, n, 1)
    stub_fill(y, {"just_before": -1, "just_behind": n, "far_front": -g, "far_behind": n + g - 1}[where], 1, 1)
    with pytest.raises(AssertionError, match="wrote outside"):
        guarded.check("stub")


def test_a_write_into_the_guard_of_an_operand_or_a_scratch_is_caught():
    x = guarded.inp(np.arange(10, dtype=np.float32), device=CPU)
    assert np.array_equal(x.numpy(), np.arange(10, dtype=np.float32))
    stub_fill(x, 10, 1, 0.0)
    with pytest.raises(AssertionError, match="wrote outside its inp"):
        guarded.check("stub")
    guarded.reset()
    s = guarded.scratch(10, device=CPU)
    stub_fill(s, -1, 1, 0.0)
    with pytest.raises(AssertionError, match="wrote outside its scratch"):
        guarded.check("stub")


def test_the_surroundings_of_an_operand_are_poison():
    x = guarded.inp(np.ones((4, 6), dtype=np.float32), device=CPU)
    w, g = guarded.whole(x), guarded.offset(x)
    assert bool(torch.isnan(w[:g]).all()) and bool(torch.isnan(w[g + 24:]).all()) and w.numel() == 2 * g + 24
    f = guarded.inp(np.zeros((2, 3), dtype=np.uint8), torch.uint8, device=CPU)
    w, g = guarded.whole(f), guarded.offset(f)
    assert bool((w[:g] == 255).all()) and bool((w[g + 6:] == 255).all())
    assert float((w[g - 1].float() * 0 + guarded.whole(x)[0] * 0).nan_to_num(nan=-1.0)) == -1.0, "x * 0 of a stray element is NaN, not 0"


@pytest.mark.parametrize("miss", [0, 17, 32])
def test_an_unwritten_interior_element_is_caught(miss):
    y = guarded.out((3, 11), device=CPU)
    stub_fill(y, 0, 33, 2.0)
    guarded.whole(y).view(torch.int32)[guarded.offset(y) + miss] = guarded.F32_PATTERN
    with pytest.raises(AssertionError, match="left 1 of 33 elements .* unwritten, first at flat index %d" % miss):
        guarded.check("stub")


def test_a_different_nan_in_a_guard_is_caught():
    """isnan() would let this through: the guards are compared by bits"""
    y = guarded.out((8,), device=CPU)
    stub_fill(y, 0, 8, 1.0)
    stub_fill(y, 8, 1, float("nan"))                                   # the default quiet NaN 0x7FC00000, not the pattern
    assert bool(torch.isnan(guarded.whole(y)[: guarded.offset(y)]).all()) and bool(torch.isnan(guarded.whole(y)[guarded.offset(y) + 8:]).all())
    with pytest.raises(AssertionError, match="wrote outside"):
        guarded.check("stub")


def test_a_nan_result_is_a_written_element():
    """a kernel's own NaN in the interior counts as written (the test's comparison with its reference is what rejects it)"""
    y = guarded.out((8,), device=CPU)
    stub_fill(y, 0, 8, float("nan"))
    guarded.check("stub")


def test_a_scratch_one_element_short_is_caught():
    """a stub that needs n elements of scratch, handed n - 1: its last store lands in the guard"""
    need = 100

    def stub(scr):
        stub_fill(scr, 0, need, 0.5)

    s = guarded.scratch(need, device=CPU)
    assert s.numel() == need and bool(guarded.poisoned(s).all()), "exactly n elements, never zeros"
    stub(s)
    guarded.check("stub at its minimum")
    guarded.no_poison(s, s[:need], "stub")
    guarded.reset()
    short = guarded.scratch(need - 1, device=CPU)
    stub(short)
    with pytest.raises(AssertionError, match="wrote outside its scratch .* 1 behind"):
        guarded.check("stub one element short")


def test_reported_rows_of_a_scratch_must_be_written():
    s = guarded.scratch(40, device=CPU)
    stub_fill(s, 0, 19, 1.0)
    guarded.check("stub")                                              # rows beyond the reported ones may keep the pattern
    guarded.no_poison(s, s[:19], "stub")
    with pytest.raises(AssertionError, match="1 of 20 reported elements were never written, first at 19"):
        guarded.no_poison(s, s[:20], "stub")


def test_untouched_mask_is_honoured_exactly():
    mask = np.zeros((4, 6), dtype=bool)
    mask[:, [1, 4]] = True                                             # columns the call leaves alone
    y = guarded.out((4, 6), device=CPU)
    y[:, [0, 2, 3, 5]] = 1.0
    guarded.check("stub", untouched=[(y, mask)])
    # broadcast masks (one row of columns)
    y = guarded.out((4, 6), device=CPU)
    y[:, [0, 2, 3, 5]] = 1.0
    guarded.check("stub", untouched=[(y, mask[0])])
    # a written element that should have been left alone
    y = guarded.out((4, 6), device=CPU)
    y[:, [0, 2, 3, 5]] = 1.0
    y[2, 1] = 0.0
    with pytest.raises(AssertionError, match="wrote 1 elements .* should leave alone, first at flat index 13"):
        guarded.check("stub", untouched=[(y, mask)])
    # an element left alone that should have been written
    y = guarded.out((4, 6), device=CPU)
    y[:, [0, 2, 3]] = 1.0
    y[:3, 5] = 1.0
    with pytest.raises(AssertionError, match="left 1 elements .* unwritten that it should write, first at flat index 23"):
        guarded.check("stub", untouched=[(y, mask)])
    # without the mask the same result fails
    y = guarded.out((4, 6), device=CPU)
    y[:, [0, 2, 3, 5]] = 1.0
    with pytest.raises(AssertionError, match="left 8 of 24"):
        guarded.check("stub")


def test_results_are_checked_once_and_the_rest_stays_watched():
    x = guarded.inp(np.ones(5, dtype=np.float32), device=CPU)
    y = guarded.out(5, device=CPU)
    stub_fill(y, 0, 5)
    guarded.check("first call")
    y2 = guarded.out(5, device=CPU)
    stub_fill(y2, 0, 5)
    stub_fill(x, -1, 1)                                                # the second call damages the operand's guard
    with pytest.raises(AssertionError, match="second call wrote outside its inp"):
        guarded.check("second call")
