"""Server-side model updates without a GPU: the threshold helper against np.percentile itself, a NumPy model of the three kernels of
k_select.hip against the sort-based answer, and the encode's byte layout against the reference's writer.  tests/test_gpu_select.py holds
the device to the same sort-based answers; when it fails there, the models here say which step differs."""
import numpy as np
import pytest

from ams_amd import delta as D, hip, spec as S
from ams_amd.coord_masks import percentile_cut, percentile_rank
from test_delta_layout_cpu import encode, layout_vars

SPEC19 = S.build_spec(19)
FRACTIONS = (0.1, 0.05, 0.2, 0.01, 0.37)
SIZES = (1, 2, 3, 1000, 2113043)
N_MODEL = 2113043


def change_cases(n, seed=0):
    """name -> float32 changes: random, heavy ties (<= 5 distinct values), two adjacent floats, all zeros, one NaN"""
    rng = np.random.default_rng(seed + n)
    one = np.float32(1)
    out = {
        "random": (np.abs(rng.standard_normal(n)) * 1e-3).astype(np.float32),
        "ties": (rng.integers(0, 5, n) * 0.25).astype(np.float32),
        "adjacent": np.where(rng.random(n) < 0.5, one, np.nextafter(one, np.float32(2))).astype(np.float32),
        "zeros": np.zeros(n, np.float32),
    }
    nan = out["random"].copy()
    nan[n // 2] = np.nan
    out["one_nan"] = nan
    return out


def order_statistics(x, k):
    """(a, b, nan_count) from a sort: the elements of rank k and k + 1 (k again at the end), NaNs last"""
    s = np.sort(x)
    return s[k], s[min(k + 1, x.size - 1)], int(np.isnan(x).sum())


def same_bits(a, b):
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


# ---- 1. the threshold is np.percentile's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_percentile_cut_is_numpys(n):
    for name, x in change_cases(n).items():
        s = np.sort(x)
        nans = int(np.isnan(x).sum())
        for f in FRACTIONS:
            q = 100 * (1 - f)
            k = percentile_rank(n, q)
            cut = percentile_cut(s[k], s[min(k + 1, n - 1)], n, q, nans)
            with np.errstate(invalid="ignore"):
                want = np.percentile(x, q)
            assert isinstance(cut, np.float32) and want.dtype == np.float32
            assert same_bits(cut, want) or (np.isnan(cut) and np.isnan(want)), (name, n, f, cut, want)
            assert np.array_equal(x > cut, x > want)
            if name == "ties" and n > 100:
                assert s[k] == s[k + 1]
            if name == "one_nan":
                assert np.isnan(cut) and not (x > cut).any()


def test_adjacent_floats_on_both_sides_of_gamma_one_half():
    one = np.float32(1)
    x = np.array([one] * 5 + [np.nextafter(one, np.float32(2))] * 6, np.float32)
    kept = []
    for q in (90, 80, 50, 45):
        a, b, nans = order_statistics(x, percentile_rank(x.size, q))
        cut = percentile_cut(a, b, x.size, q, nans)
        assert same_bits(cut, np.percentile(x, q)), q
        kept.append(int((x > cut).sum()))
    assert kept == [0, 0, 0, 6]
    # a < b adjacent with gamma on either side of 1/2: the cut rounds onto a or onto b
    sides = set()
    for n in (7, 11, 1000, 4097):
        x = np.array([one] * (n // 2) + [np.nextafter(one, np.float32(2))] * (n - n // 2), np.float32)
        for q in np.linspace(1, 99, 197):
            k = percentile_rank(n, q)
            a, b, _ = order_statistics(x, k)
            cut = percentile_cut(a, b, n, q)
            assert same_bits(cut, np.percentile(x, q)), (n, q)
            if a != b:
                sides.add(bool(cut == b))
    assert sides == {False, True}


def test_rank_at_the_ends():
    assert percentile_rank(1, 90.0) == 0 and percentile_rank(5, 100.0) == 4 and percentile_rank(5, 0.0) == 0
    x = np.arange(5, dtype=np.float32)
    for q in (0.0, 100.0):
        a, b, _ = order_statistics(x, percentile_rank(5, q))
        assert same_bits(percentile_cut(a, b, 5, q), np.percentile(x, q))


# ---- 2. a NumPy model of the kernels ---------------------------------------------------------------------------------------------------------
def model_select(after, before, k):
    """select_hist_kernel / select_scan_kernel x 3, select_tail_kernel, select_finish_kernel -> (a, b, nan_count)"""
    u = np.abs(after - before).view(np.uint32)
    n = u.size
    prefix, rank = 0, int(k)
    for shift, bits, above in ((21, 11, 31), (10, 11, 21), (0, 10, 10)):
        chosen = u[(u >> np.uint32(above)) == np.uint32(prefix >> above)]
        hist = np.bincount((chosen >> np.uint32(shift)) & np.uint32((1 << bits) - 1), minlength=2048)
        ends = np.cumsum(hist)
        digit = int(np.searchsorted(ends, rank, side="right"))
        rank -= int(ends[digit] - hist[digit])
        prefix |= digit << shift
    a = np.uint32(prefix)
    le = int((u <= a).sum())
    above_a = u[u > a]
    b = a if (le > k + 1 or k + 1 >= n or above_a.size == 0) else above_a.min()
    return a.view(np.float32), np.uint32(b).view(np.float32), int((u > np.uint32(0x7F800000)).sum())


def model_apply(after, before, cut):
    """select_apply_kernel -> (mask uint8, params, kept)"""
    with np.errstate(invalid="ignore"):
        m = np.abs(after - before) > np.float32(cut)
    return m.astype(np.uint8), np.where(m, after, before), int(m.sum())


def host_formulas(after, before, q):
    """semantic_network.py's host path on one flat array: threshold, mask, combined parameters, kept"""
    with np.errstate(invalid="ignore"):
        changes = np.abs(after - before)
        cut = np.percentile(changes, q)
        m = np.abs(after - before) > cut
    return cut, m, np.where(m, after, before), int(m.sum())


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097, N_MODEL))
def test_kernel_model_equals_the_sort(n):
    rng = np.random.default_rng(n)
    for name, x in change_cases(n).items():
        before = (rng.integers(-2048, 2048, n) / 1024).astype(np.float32)
        after = before + x                                     # what counts is the float32 change the two arrays really have
        with np.errstate(invalid="ignore"):
            changes = np.abs(after - before)
        for f in FRACTIONS if n < N_MODEL else (0.1, 0.01):
            q = 100 * (1 - f)
            k = percentile_rank(n, q)
            a, b, nans = model_select(after, before, k)
            wa, wb, wn = order_statistics(changes, k)
            assert nans == wn
            assert (same_bits(a, wa) or np.isnan(wa)) and (same_bits(b, wb) or np.isnan(wb)), (name, n, f, a, wa, b, wb)
            cut = percentile_cut(a, b, n, q, nans)
            mask, params, kept = model_apply(after, before, cut)
            wcut, wm, wp, wk = host_formulas(after, before, q)
            assert same_bits(cut, wcut) or (np.isnan(cut) and np.isnan(wcut))
            assert np.array_equal(mask.astype(bool), wm) and kept == wk
            assert np.array_equal(params.view(np.uint32), wp.view(np.uint32))


# ---- 3. the encode's byte layout -------------------------------------------------------------------------------------------------------------
def model_encode(layout, flat_mask, params, stats):
    """encode_kernel as NumPy: every mask BIT of the payload finds its variable by the variables' mask offsets (the kernel's binary search),
    its element inside it and, in layout order, its flat index; set bits fetch their value from params / stats.  flat_mask None = all."""
    moff = np.array([e.mask_offset for e in layout.entries], np.int64)
    count = np.array([e.count for e in layout.entries], np.int64)
    first = np.concatenate([[0], np.cumsum(count)])
    offset = np.array([e.offset for e in layout.entries], np.int64)
    region = np.array([e.region for e in layout.entries], np.int64)
    byte = np.repeat(np.arange(layout.mask_bytes, dtype=np.int64), 8)
    bit = np.tile(np.arange(8, dtype=np.int64), layout.mask_bytes)
    v = np.searchsorted(moff, byte, side="right") - 1
    e = (byte - moff[v]) * 8 + bit
    valid = e < count[v]
    flat = first[v] + e
    bits = valid.copy()
    if flat_mask is not None:
        bits[valid] = np.asarray(flat_mask)[flat[valid]] != 0
    weights = (1 << (7 - np.arange(8))).astype(np.uint8)
    mask_section = (bits.reshape(-1, 8) * weights).sum(axis=1).astype(np.uint8)
    src = np.where(region[v[bits]] == hip.REGION_PARAMS, 0, params.size) + offset[v[bits]] + e[bits]
    with np.errstate(over="ignore"):
        values = np.concatenate([params, stats])[src].astype("<f2")
    return mask_section.tobytes() + values.tobytes()


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
@pytest.mark.parametrize("density", ["zero", "one", "tenth", "all", "null"])
def test_encode_layout_model_equals_the_reference_writer(strategy, density):
    rng = np.random.default_rng(11)
    L = D.delta_layout(SPEC19, strategy)
    assert L.mask_bytes % 2 == 1 and any(e.count % 8 for e in L.entries)
    params = rng.standard_normal(SPEC19.n_trainable).astype(np.float32)
    stats = rng.standard_normal(SPEC19.n_stats).astype(np.float32)
    params[:4] = [65504.0, 65520.0, 1e5, 2.0 ** -24]
    vals = layout_vars(SPEC19, L, params, stats)
    if density in ("zero", "one"):
        masks = [np.zeros(v.size, bool) for v in vals]
        if density == "one":
            odd = next(i for i, e in enumerate(L.entries) if e.count % 8)
            masks[odd][-1] = True                                   # the last element of a variable whose count is not a multiple of 8
    elif density == "tenth":
        masks = [rng.random(v.size) < 0.1 for v in vals]
    else:
        masks = [np.ones(v.size, bool) for v in vals]
    flat = None if density == "null" else np.concatenate(masks).astype(np.uint8)
    with np.errstate(over="ignore"):
        want = encode(vals, masks)
    assert model_encode(L, flat, params, stats) == want
