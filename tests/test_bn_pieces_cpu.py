"""tests/bn_pieces_ref.py without a GPU: ams_k_col_plan reaches the path every listed shape is named for, the bars keep the rule and the cap,
every small defect made on the restatement's output fails the check it belongs to, and include/ams_hip.h states the scratch formulas."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import bn_pieces_ref as R
from ams_amd import hip


def plan(M, Cn, groups=1):
    out = (C.c_int32 * 4)()
    rc = hip.lib().ams_k_col_plan(M, groups, Cn, out)
    return rc, tuple(out)


@pytest.mark.parametrize("Cn", R.CHANNELS)
def test_col_plan_reaches_the_named_paths(Cn):
    slots = R.CHANNEL_SLOTS[Cn]
    for name in R.ROWS:
        M, chunks, rpc = R.rows_case(Cn, name)
        rc, got = plan(M, Cn)
        assert rc == 0 and got == (Cn // 4, slots, chunks, rpc) == R.col_plan(M, Cn), (Cn, name, got)
        assert (Cn // 4) * slots <= 256
    assert [R.rows_case(Cn, n)[1] for n in ("S", "S + 1", "113 S", "129 S", "241 S + 1", "1024 S + 1")] == [1, 2, 113, 129, 242, 1024]
    # the capped case: rows_per_chunk above 16 slots, and chunks that begin past the end of the tensor
    M, chunks, rpc = R.rows_case(Cn, "1024 S + 1")
    S = 16 * slots
    assert rpc == S + 1 and chunks == R.MAX_CHUNKS and chunks * rpc >= M
    if S <= 1022:
        assert (chunks - 1) * rpc >= M and R.empty_chunks(M, chunks, rpc) >= 1
    else:
        # C = 16: S = 1024 and 1023 * 1025 = 1024 * 1024 - 1 < M: no chunk is empty, the last one holds 2 rows of its 1025
        assert R.empty_chunks(M, chunks, rpc) == 0 and M - (chunks - 1) * rpc == 2


def test_col_plan_bounds():
    assert plan(17, 1024) == (0, (256, 1, 2, 9))            # C = 1024 is the bound of the launchers' check
    for Cn in (1028, 6, 0):
        assert plan(17, Cn)[0] == -1, Cn
    assert plan(0, 16)[0] == -1
    assert hip.lib().ams_k_col_plan(17, 1, 16, None) == -1


def test_reduce_batch_refuses_a_33rd_job_before_any_launch():
    lib = hip.lib()
    n = 33
    ptrs = (C.c_void_p * n)(*([0x1000] * n))                 # never dereferenced: the count is refused first
    i32, i64 = (C.c_int32 * n)(*([1] * n)), (C.c_int64 * n)(*([1] * n))
    assert lib.ams_k_reduce_batch(ptrs, i32, i64, i64, ptrs, n, None) == -1
    assert b"33 jobs" in lib.ams_last_error()
    assert lib.ams_k_reduce_batch(ptrs, i32, i64, i64, ptrs, 0, None) == -1


def test_bars_keep_the_rule_and_the_cap():
    L = R.levels()
    assert set(L) >= {"colstats", "bn_bwd_reduce", "colsum", "colstats_f64", "fold_f64", "fold_f32", "finalize.mean", "finalize.rstd",
                      "finalize.scale", "finalize.shift", "finalize.moving_mean", "finalize.moving_var", "bwd_coef.cA", "bwd_coef.cB",
                      "bwd_coef.cC", "bwd_coef.dgamma", "bwd_coef.dbeta", "bn_fold.scale", "bn_fold.shift"}
    for k, v in L.items():
        assert np.isfinite(v) and v >= R.FLOOR, k
        assert R.bar(k) == 4.0 * v and R.bar(k) <= R.BAR_CAP, (k, R.bar(k))
    print({k: "%.3g" % v for k, v in L.items()})


# ------------------------------------------------------------------------------------------------ defects
@pytest.mark.parametrize("kind", ["fwd", "bwd"])
def test_second_stage_defects_fail(kind):
    rows, Cn = 276, 24
    part, _, _, _ = R.partial_rows(rows, Cn, kind)
    flat = part.reshape(rows, 2 * Cn)
    ref, terms = flat.astype(np.float64).sum(axis=0), R.abs_sum(flat.astype(np.float64))
    bar = R.bar("fold_f64")
    for stride in (2 * Cn, 2 * Cn + 1093):
        buf = R.strided_rows(flat, stride)
        assert R.within(R.reduced_err(R.fold_f64(R.read_rows(buf, rows, 2 * Cn, stride)), ref, terms), bar)
        assert not R.within(R.reduced_err(R.fold_f64(R.read_rows(buf, rows - 1, 2 * Cn, stride)), ref, terms), bar), "the last partial row dropped"
        assert not R.within(R.reduced_err(R.fold_f64(R.read_rows(buf, rows + 1, 2 * Cn, stride)), ref, terms), bar), "row `rows` added"
    buf = R.strided_rows(flat, 2 * Cn + 1093)
    assert not R.within(R.reduced_err(R.fold_f64(R.read_rows(buf, rows, 2 * Cn, 2 * Cn)), ref, terms), bar), "columns read at stride 2 C"
    # ... and with finite values where the poison is, the dropped row alone is 1 / 276 of the sum
    assert R.reduced_err(R.fold_f64(flat[:-1]), ref, terms) > 100 * bar


@pytest.mark.parametrize("name", ["S + 1", "113 S"])
def test_a_chunk_one_row_short_fails(name):
    Cn = 16
    M, p, z, da, center = R.direct_operands(Cn, name, "half")
    act = R.ACT_RELU6
    mask = R.act_mask(R.y_f32(z, p["scale"], p["shift"]), act)
    for fam, t32, t64 in (("colstats", R.stats_terms_f32(z, center), R.stats_terms_f64(z, center)),
                          ("bn_bwd_reduce", R.bwd_terms_f32(da, z, p["scale"], p["shift"], act, p["mean"], p["rstd"]),
                           R.bwd_terms_f64(da, z, mask, p["mean"], p["rstd"]))):
        ref, terms = np.stack([t.sum(axis=0) for t in t64]), np.stack([R.abs_sum(t) for t in t64])
        good = np.stack([R.fold_f64(R.first_stage_f32(t)) for t in t32])
        assert R.within(R.reduced_err(good, ref, terms), R.bar(fam))
        chunks = R.col_plan(M, Cn)[2]
        for k in (0, chunks - 1):
            bad = np.stack([R.fold_f64(R.first_stage_f32(t, drop_last_row_of_chunk=k)) for t in t32])
            # q0 and q1 each against its own terms: the row's share of a sum is about 1 / M
            for q in range(2):
                assert not R.within(R.reduced_err(bad[q], ref[q], terms[q]), R.bar(fam)), (fam, name, k, q)


def test_finalize_defects_fail():
    Cn, n = 24, 257
    sums, p, center = R.finalize_case(Cn, n, "half")
    args = (sums, float(n), center, p["gamma"], p["beta"], R.EPS, R.ONE_MINUS_DECAY, p["moving_mean"], p["moving_var"])
    ref = R.finalize_f64(*args)
    good = R.finalize_f32(*args)
    for k in ref:
        assert R.within(R.channel_err(good[k], ref[k]), R.bar("finalize." + k)), k
    bad = R.finalize_f32(*args, n_mean=float(n - 1))                                        # n - 1 in place of n
    assert not R.within(R.channel_err(bad["mean"], ref["mean"]), R.bar("finalize.mean"))
    assert not R.within(R.channel_err(bad["rstd"], ref["rstd"]), R.bar("finalize.rstd"))
    bad = R.finalize_f32(*args, biased_moving=True)                                          # the biased variance fed to the moving variance
    assert not R.within(R.channel_err(bad["moving_var"], ref["moving_var"]), R.bar("finalize.moving_var"))
    for k in ("mean", "rstd", "scale", "shift", "moving_mean"):
        assert R.same_bits(bad[k], good[k])
    # n = 1 keeps the divisor 1: the unbiased variance is the biased one there, and finite
    sums, p, center = R.finalize_case(Cn, 1, "null")
    args = (sums, 1.0, center, p["gamma"], p["beta"], R.EPS, R.ONE_MINUS_DECAY, p["moving_mean"], p["moving_var"])
    assert R.same_bits(R.finalize_f32(*args)["moving_var"], R.finalize_f32(*args, biased_moving=True)["moving_var"])
    assert np.isfinite(R.finalize_f64(*args)["moving_var"]).all()


def test_bwd_coef_defects_fail():
    Cn, n = 24, 257
    sums, terms, p = R.bwd_coef_case(Cn, n, R.ACT_RELU6)
    ref = R.bwd_coef_f64(sums, float(n), p["gamma"], p["mean"], p["rstd"])
    good = R.bwd_coef_f32(sums, float(n), p["gamma"], p["mean"], p["rstd"])
    for k in ("cA", "cB", "cC"):
        assert R.within(R.channel_err(good[k], ref[k]), R.bar("bwd_coef." + k))
    bad = R.bwd_coef_f32(sums, float(n), p["gamma"], p["mean"], p["rstd"], no_k_mean=True)   # coefB without k mean
    assert not R.within(R.channel_err(bad["cB"], ref["cB"]), R.bar("bwd_coef.cB"))
    bad = R.bwd_coef_f32(sums, float(n), p["gamma"], p["mean"], p["rstd"], swapped=True)     # dgamma and dbeta swapped
    assert R.within(R.reduced_err(good["dgamma"], ref["dgamma"], terms[1]), R.bar("bwd_coef.dgamma"))
    assert not R.within(R.reduced_err(bad["dgamma"], ref["dgamma"], terms[1]), R.bar("bwd_coef.dgamma"))
    assert not R.within(R.reduced_err(bad["dbeta"], ref["dbeta"], terms[0]), R.bar("bwd_coef.dbeta"))


def test_the_knees_are_exact_and_a_closed_upper_knee_shows():
    Cn, M = 16, 257
    p = R.channel_params(Cn, True)
    z0, da = R.draw(M, Cn, True)
    z, scale, shift = R.plant_knees(z0, p["scale"], p["shift"])
    y32, y64 = R.y_f32(z, scale, shift), z.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    assert (y32[:, 1] == 0).all() and (y32[:, 2] == 6).all() and (y64[:, 1] == 0).all() and (y64[:, 2] == 6).all()
    a = R.bn_act_f32(z, scale, shift, R.ACT_RELU6)
    assert (a[:, 1] == 0).all() and (a[:, 2] == 6).all()
    assert R.channel_err(a, R.bn_act_f64(z, scale, shift, R.ACT_RELU6)) < 1e-5
    mk = R.act_mask(y32, R.ACT_RELU6)
    assert (mk[:, 1] == 0).all() and (mk[:, 2] == 0).all() and 0 < mk.mean() < 1               # Relu6Grad is 0 at both knees
    args = (da, z, scale, shift, R.ACT_RELU6, p["cA"], p["cB"], p["cC"])
    assert not R.same_bits(R.bwd_apply_f32(*args), R.bwd_apply_f32(*args, le6=True))          # `<= 6` in place of `< 6`
    q = R.bwd_terms_f32(da, z, scale, shift, R.ACT_RELU6, p["mean"], p["rstd"])
    q_le = R.bwd_terms_f32(da, z, scale, shift, R.ACT_RELU6, p["mean"], p["rstd"], le6=True)
    t64 = R.bwd_terms_f64(da, z, mk, p["mean"], p["rstd"])
    ref, terms = t64[0].sum(axis=0), R.abs_sum(t64[0])
    assert R.within(R.reduced_err(R.fold_f64(R.first_stage_f32(q[0])), ref, terms), R.bar("bn_bwd_reduce"))
    assert not R.within(R.reduced_err(R.fold_f64(R.first_stage_f32(q_le[0])), ref, terms), R.bar("bn_bwd_reduce"))


def test_header_states_the_scratch_formulas():
    text = (Path(__file__).resolve().parent.parent / "include" / "ams_hip.h").read_text()
    for formula in ("1024 * 2 * C", "1024 * C", "B * 1024 * C", "min(1024, ceil(M / (16 * slots)))", "rows_per_chunk = ceil(M / chunks)"):
        assert formula in text, formula
    lib = hip.lib()
    assert lib.ams_k_colstats_scratch(12345, 24) == 1024 * 2 * 24 and lib.ams_k_colsum_scratch(32) == 1024 * 32
    assert lib.ams_k_image_colsum_scratch(3, 16) == 3 * 1024 * 16 == lib.ams_k_global_mean_scratch(3, 16)
