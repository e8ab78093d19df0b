"""The BN pieces of k_elementwise.hip at the kernel level, each through its own ams_k_* entry: the column reductions, the second stages over partial
rows, the per-channel arithmetic, the apply passes and the plain folds.  Reference, cases, measure and bars: tests/bn_pieces_ref.py (held on the
CPU by tests/test_bn_pieces_cpu.py).  Every case asserts through ams_k_col_plan that it reaches the path it is named for.

BIT FOR BIT, no tolerance: ams_k_bn_act and ams_k_bn_bwd_apply (out of place, and in place) against the f32 restatement; ams_k_bn_finalize fed
ams_k_colstats_bn's sums against that entry's own scale / shift / mean / rstd / moving statistics (bn_fin.hpp = the stand-alone kernel);
ams_k_bn_bwd_coef + ams_k_bn_param_grads against ams_k_bn_bwd_reduce_coef; ams_k_partials_to_sums + the per-channel kernel against both
*_partials entries; ams_k_reduce_batch job by job against ams_k_reduce_splits where both pick the same lanes per output; every entry twice.

AGAINST F64, bar = 4 L, L = the f32 restatement's own error (at least 2^-23), the measure of DESIGN section 6.  L | bar | the engine's worst on
one MI355X:
  colstats (ams_k_colstats, _bn)                   3.0e-7 | 1.2e-6 | 3.0e-7
  bn_bwd_reduce (and _coef)                        1.2e-7 | 4.8e-7 | 9.3e-8
  colsum (ams_k_colsum, ams_k_image_colsum)        4.2e-7 | 1.7e-6 | 4.2e-7
  colstats_f64, fold_f64 | fold_f32 | l2_loss      1.2e-7 | 4.8e-7 | 0 | 3.5e-8 | 2e-16
  finalize: mean, moving_mean, moving_var          1.2e-7 | 4.8e-7 | 6.0e-8
  finalize: rstd                                   1.25e-7 | 5.0e-7 | 1.25e-7
  finalize: scale                                  1.6e-7 | 6.4e-7 | 1.6e-7
  finalize: shift                                  2.6e-7 | 1.0e-6 | 2.6e-7
  bwd_coef: cA, cB, cC                             1.2e-7 | 4.8e-7 | 5.9e-8
  bwd_coef: dgamma | dbeta                         1.2e-7 | 4.8e-7 | 3.1e-8 | 3.9e-8
  bn_fold: scale                                   1.3e-7 | 5.3e-7 | 1.3e-7
  bn_fold: shift                                   1.8e-7 | 7.2e-7 | 1.8e-7
Where the engine's figure equals L the kernel is the restatement; the f64 sums of the four direct entries are also held to the restatement's
own sums within 2^-42 of sum |terms| (RESTATED_BAR below; measured 0: f32 partial rows of one magnitude add exactly in f64).

Buffers (tests/guarded.py): results between poisoned guards, in/out tensors (moving statistics, the in-place dz) too; scratch poisoned and exactly
the entry's *_scratch(); partial rows poisoned everywhere but the [rows][2][C] cells a stage may read, and nothing but guard behind the last.
"""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import bn_pieces_ref as R
import guarded as G
from ams_amd import hip

pytestmark = pytest.mark.gpu

E_INVALID, E_HIP = -1, -2
F32, F64 = np.float32, np.float64
WORST = {}
EPS, OMD = float(R.EPS), float(R.ONE_MINUS_DECAY)          # the f32 values, as the C ABI takes them


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    R.levels()                               # the references of the direct cases and the bars, once
    yield hip.lib()
    print("\nworst per family (bar): " + ", ".join("%s %.2e (%.2e)" % (k, v, RESTATED_BAR if k.startswith("restated.") else R.bar(k))
                                                    for k, v in sorted(WORST.items())))


@pytest.fixture(autouse=True)
def _guarded_buffers():
    G.reset()
    yield
    left = G.pending()
    G.reset()
    assert not left, "results handed out and never checked: %s" % [tuple(t.shape) for t in left]


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def dev(a, dtype=torch.float32):
    """the operand on the device between poisoned guards (the reference's arrays are shared and read-only; guarded.inp copies them)"""
    if a is None:
        return None
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)
        return G.inp(a, dtype)


def out(shape, dtype=torch.float32):
    return G.out(shape, dtype)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def run(rc, what="the call"):
    if rc == E_HIP:
        pytest.exit("%s: a HIP call failed (%s); nothing more runs on this device" % (what, hip.lib().ams_last_error()), returncode=3)
    hip.check(rc, what)
    try:
        G.check(what)
    except RuntimeError as e:
        pytest.exit("%s: %s; nothing more runs on this device" % (what, e), returncode=3)


def refused(rc, what):
    assert rc == E_INVALID, "%s: expected a refusal, got %d" % (what, rc)
    G.check(what, untouched=[(t, True) for t in G.pending()])


def host(t):
    return t.cpu().numpy()


def held(key, err, what):
    WORST[key] = max(WORST.get(key, 0.0), err if err == err else float("inf"))
    assert R.within(err, R.bar(key)), "%s: %s %.3e above the bar %.3e" % (what, key, err, R.bar(key))


# The first stage adds f32 terms in an order its source fixes, and first_stage_f32 restates that order: the partial rows are the same f32 numbers.
# What is left between the entry's f64 sums and the restatement's is the ORDER in which the second stage adds at most 1024 of them in f64:
# at most 1024 * 2^-53 of sum |partial rows|, twice that as the bar.  (A row dropped from a million is 1e-6 of its sum: the f64 bar alone would
# not see it at that size; this one does.)
RESTATED_BAR = 2.0 ** -42


def restated(key, got, ref3, what):
    err = R.reduced_err(got, ref3[2], ref3[1])
    WORST["restated." + key] = max(WORST.get("restated." + key, 0.0), err if err == err else float("inf"))
    assert R.within(err, RESTATED_BAR), "%s: %s %.3e from the f32 restatement's sums (bar %.3e)" % (what, key, err, RESTATED_BAR)


def bits(a, b, what):
    assert R.same_bits(host(a) if isinstance(a, torch.Tensor) else a, host(b) if isinstance(b, torch.Tensor) else b), what


def plan(lib, M, Cn, groups=1):
    o = (C.c_int32 * 4)()
    hip.check(lib.ams_k_col_plan(M, groups, Cn, o))
    return tuple(o)


# ------------------------------------------------------------------------------------------------ the entries, each returning its results
FWD_KEYS = ("scale", "shift", "mean", "rstd", "moving_mean", "moving_var")
BWD_KEYS = ("cA", "cB", "cC", "dgamma", "dbeta")


class Chan:
    """the per-channel operands of a case on the device (uploaded once per case)"""

    def __init__(self, p, center):
        self.p, self.center = p, dev(center)
        for k in ("gamma", "beta", "scale", "shift", "mean", "rstd", "cA", "cB", "cC"):
            setattr(self, k, dev(p[k]))

    def moving(self):
        return dev(self.p["moving_mean"]), dev(self.p["moving_var"])


def fwd_outputs(Cn):
    return [out(Cn) for _ in range(4)]


def colstats_bn(lib, zd, M, Cn, ch, scr, nscr, n):
    sums, (sc, sh, mean, rstd), (mm, mv) = out((2, Cn), torch.float64), fwd_outputs(Cn), ch.moving()
    run(lib.ams_k_colstats_bn(P(zd), M, Cn, P(ch.center), P(sums), P(scr), nscr, n, P(ch.gamma), P(ch.beta), EPS, OMD, P(mm), P(mv),
                              P(sc), P(sh), P(mean), P(rstd), stream()), "colstats_bn")
    return sums, dict(zip(FWD_KEYS, (sc, sh, mean, rstd, mm, mv)))


def bn_finalize(lib, sums, n, Cn, ch):
    (sc, sh, mean, rstd), (mm, mv) = fwd_outputs(Cn), ch.moving()
    run(lib.ams_k_bn_finalize(P(sums), n, Cn, P(ch.center), P(ch.gamma), P(ch.beta), EPS, OMD, P(mm), P(mv), P(sc), P(sh), P(mean),
                              P(rstd), stream()), "bn_finalize")
    return dict(zip(FWD_KEYS, (sc, sh, mean, rstd, mm, mv)))


def bn_fwd_partials(lib, part, rows, stride, Cn, n, ch):
    sums, (sc, sh, mean, rstd), (mm, mv) = out((2, Cn), torch.float64), fwd_outputs(Cn), ch.moving()
    run(lib.ams_k_bn_fwd_partials(P(part), rows, stride, Cn, P(sums), n, P(ch.center), P(ch.gamma), P(ch.beta), EPS, OMD, P(mm), P(mv),
                                  P(sc), P(sh), P(mean), P(rstd), stream()), "bn_fwd_partials")
    return sums, dict(zip(FWD_KEYS, (sc, sh, mean, rstd, mm, mv)))


def bwd_reduce_coef(lib, dad, zd, M, Cn, act, ch, scr, nscr, n):
    sums, o = out((2, Cn), torch.float64), [out(Cn) for _ in range(5)]
    run(lib.ams_k_bn_bwd_reduce_coef(P(dad), P(zd), M, Cn, P(ch.scale), P(ch.shift), act, P(ch.mean), P(ch.rstd), P(sums), P(scr), nscr, n, P(ch.gamma),
                                     *[P(t) for t in o], stream()), "bn_bwd_reduce_coef")
    return sums, dict(zip(BWD_KEYS, o))


def bwd_coef_and_grads(lib, sums, n, Cn, ch):
    """ams_k_bn_bwd_coef without dgamma / dbeta, then ams_k_bn_param_grads: the data-parallel step's pair"""
    o = [out(Cn) for _ in range(3)]
    run(lib.ams_k_bn_bwd_coef(P(sums), n, Cn, P(ch.gamma), P(ch.mean), P(ch.rstd), P(o[0]), P(o[1]), P(o[2]), None, None, stream()), "bn_bwd_coef")
    o += [out(Cn), out(Cn)]
    run(lib.ams_k_bn_param_grads(P(sums), Cn, P(o[3]), P(o[4]), stream()), "bn_param_grads")
    return dict(zip(BWD_KEYS, o))


def bwd_partials(lib, part, rows, stride, Cn, n, ch):
    sums, o = out((2, Cn), torch.float64), [out(Cn) for _ in range(5)]
    run(lib.ams_k_bn_bwd_partials(P(part), rows, stride, Cn, P(sums), n, P(ch.gamma), P(ch.mean), P(ch.rstd), *[P(t) for t in o], stream()),
        "bn_bwd_partials")
    return sums, dict(zip(BWD_KEYS, o))


def same_dict(a, b, what):
    for k in a:
        bits(a[k], b[k], "%s: %s differs" % (what, k))


def twice(f, what):
    """every entry twice: the same bits (the file's header claims run-to-run determinism); the first run's results"""
    a, b = f(), f()
    flat = lambda r: ([r] if isinstance(r, torch.Tensor) else list(r.values()) if isinstance(r, dict) else [t for x in r for t in flat(x)])  # noqa: E731
    for x, y in zip(flat(a), flat(b)):
        bits(x, y, what + ": two runs differ")
    return a


# ------------------------------------------------------------------------------------------------ direct reductions
@pytest.mark.parametrize("name", list(R.ROWS))
@pytest.mark.parametrize("Cn", R.CHANNELS)
def test_direct_reductions(lib, Cn, name):
    """ams_k_colstats, _colstats_bn (+ ams_k_bn_finalize on its sums), _colstats_f64 (up to two chunks: one thread per channel walks the rows),
    _bn_bwd_reduce, _bn_bwd_reduce_coef (+ ams_k_bn_bwd_coef and _bn_param_grads on its sums) and ams_k_colsum at one row count of
    bn_pieces_ref.ROWS: sums against f64, the per-channel results of the fused entries bit for bit against the stand-alone kernels."""
    M, chunks, rpc = R.rows_case(Cn, name)
    slots = R.CHANNEL_SLOTS[Cn]
    assert plan(lib, M, Cn) == (Cn // 4, slots, chunks, rpc), "the case does not reach the path it is named for"
    if name == "1024 S + 1":
        assert rpc > 16 * slots
        assert (chunks - 1) * rpc >= M if 16 * slots <= 1022 else M - (chunks - 1) * rpc == 2       # empty trailing chunks (C = 16: a 2-row one)
    nscr = lib.ams_k_colstats_scratch(M, Cn)
    assert nscr == 1024 * 2 * Cn
    n = float(M)
    uploaded = {}
    for C_, name_, centre, act in R.direct_cases():
        if (C_, name_) != (Cn, name):
            continue
        what = "C=%d M=%d centre=%s act=%d" % (Cn, M, centre, act)
        _, p, z, da, center = R.direct_operands(Cn, name, centre)
        ref = R.direct_reference(Cn, name, centre, act)
        far = centre != "null"
        if far not in uploaded:
            uploaded[far] = (dev(z), dev(da))
        zd, dad = uploaded[far]
        ch = Chan(p, center)
        scr = G.scratch(nscr)

        def colstats():
            sums = out((2, Cn), torch.float64)
            run(lib.ams_k_colstats(P(zd), M, Cn, P(ch.center), P(sums), P(scr), nscr, stream()), "colstats")
            return sums
        sums = twice(colstats, what)
        held("colstats", R.reduced_err(host(sums), ref["colstats"][0], ref["colstats"][1]), what)
        restated("colstats", host(sums), ref["colstats"], what)

        sums_b, fused = twice(lambda: colstats_bn(lib, zd, M, Cn, ch, scr, nscr, n), what)
        held("colstats", R.reduced_err(host(sums_b), ref["colstats"][0], ref["colstats"][1]), what + " (colstats_bn)")
        restated("colstats", host(sums_b), ref["colstats"], what + " (colstats_bn)")
        same_dict(fused, bn_finalize(lib, sums_b, n, Cn, ch), what + ": colstats_bn against bn_finalize on its sums")

        if chunks <= 2:
            def colstats_f64():
                s = out((2, Cn), torch.float64)
                run(lib.ams_k_colstats_f64(P(zd), M, Cn, P(ch.center), P(s), stream()), "colstats_f64")
                return s
            held("colstats_f64", R.reduced_err(host(twice(colstats_f64, what)), ref["colstats"][0], ref["colstats"][1]), what)

        def bwd_reduce():
            s = out((2, Cn), torch.float64)
            run(lib.ams_k_bn_bwd_reduce(P(dad), P(zd), M, Cn, P(ch.scale), P(ch.shift), act, P(ch.mean), P(ch.rstd), P(s), P(scr), nscr, stream()),
                "bn_bwd_reduce")
            return s
        sums_r = host(twice(bwd_reduce, what))
        held("bn_bwd_reduce", R.reduced_err(sums_r, ref["bn_bwd_reduce"][0], ref["bn_bwd_reduce"][1]), what)
        restated("bn_bwd_reduce", sums_r, ref["bn_bwd_reduce"], what)
        sums_c, fused = twice(lambda: bwd_reduce_coef(lib, dad, zd, M, Cn, act, ch, scr, nscr, n), what)
        held("bn_bwd_reduce", R.reduced_err(host(sums_c), ref["bn_bwd_reduce"][0], ref["bn_bwd_reduce"][1]), what + " (reduce_coef)")
        restated("bn_bwd_reduce", host(sums_c), ref["bn_bwd_reduce"], what + " (reduce_coef)")
        same_dict(fused, bwd_coef_and_grads(lib, sums_c, n, Cn, ch), what + ": bn_bwd_reduce_coef against bn_bwd_coef + bn_param_grads on its sums")

        ncs = lib.ams_k_colsum_scratch(Cn)
        scr1 = G.scratch(ncs)

        def colsum():
            s = out(Cn)
            run(lib.ams_k_colsum(P(zd), M, Cn, Cn, P(s), P(scr1), ncs, stream()), "colsum")
            return s
        held("colsum", R.reduced_err(host(twice(colsum, what)), ref["colsum"][0][0], ref["colsum"][1][0]), what)


def test_direct_reductions_bounds_and_refusals(lib):
    """C = 1024 is the bound of the launchers' check and runs; C = 1028 and C = 6 are refused; each entry refuses a scratch one float short of its
    *_scratch(), nothing touched."""
    M = 17
    for Cn in (1024, 1028, 6):
        p = R.channel_params(Cn, True)
        z, da = R.draw(M, Cn, True)
        center = R.center_of(p, "half")
        zd, dad, ch = dev(z), dev(da), Chan(p, center)
        nscr, ncs = lib.ams_k_colstats_scratch(M, Cn), lib.ams_k_colsum_scratch(Cn)
        scr, scr1 = G.scratch(nscr), G.scratch(ncs)
        o = lambda k: [out(Cn) for _ in range(k)]  # noqa: E731
        s = lambda: out((2, Cn), torch.float64)  # noqa: E731
        mm, mv = ch.moving()
        calls = {
            "colstats": lambda ns, t: lib.ams_k_colstats(P(zd), M, Cn, P(ch.center), P(t[0]), P(scr), ns, stream()),
            "colstats_bn": lambda ns, t: lib.ams_k_colstats_bn(P(zd), M, Cn, P(ch.center), P(t[0]), P(scr), ns, float(M), P(ch.gamma), P(ch.beta), EPS,
                                                               OMD, P(mm), P(mv), *[P(x) for x in t[1:5]], stream()),
            "bn_bwd_reduce": lambda ns, t: lib.ams_k_bn_bwd_reduce(P(dad), P(zd), M, Cn, P(ch.scale), P(ch.shift), 2, P(ch.mean), P(ch.rstd), P(t[0]),
                                                                   P(scr), ns, stream()),
            "bn_bwd_reduce_coef": lambda ns, t: lib.ams_k_bn_bwd_reduce_coef(P(dad), P(zd), M, Cn, P(ch.scale), P(ch.shift), 2, P(ch.mean), P(ch.rstd),
                                                                             P(t[0]), P(scr), ns, float(M), P(ch.gamma), *[P(x) for x in t[1:6]], stream()),
        }
        nres = {"colstats": 0, "colstats_bn": 4, "bn_bwd_reduce": 0, "bn_bwd_reduce_coef": 5}
        for k, f in calls.items():
            if Cn == 1024:
                refused(f(nscr - 1, [s()] + o(nres[k])), k + " with one scratch float too few")
                run(f(nscr, [s()] + o(nres[k])), k)
            else:
                refused(f(nscr, [s()] + o(nres[k])), "%s with C = %d" % (k, Cn))
        if Cn != 1024:
            bits(mm, p["moving_mean"], "a refused call moved the moving mean")
        colsum = lambda ns, t: lib.ams_k_colsum(P(zd), M, Cn, Cn, P(t), P(scr1), ns, stream())  # noqa: E731
        if Cn == 1024:
            refused(colsum(ncs - 1, out(Cn)), "colsum with one scratch float too few")
            got = out(Cn)
            run(colsum(ncs, got), "colsum")
            held("colsum", R.reduced_err(host(got), z.astype(F64).sum(axis=0), np.abs(z.astype(F64)).sum(axis=0)), "colsum C=1024")
            q0, q1 = R.stats_terms_f64(z, center)
            got = out((2, Cn), torch.float64)
            run(lib.ams_k_colstats(P(zd), M, Cn, P(ch.center), P(got), P(scr), nscr, stream()), "colstats")
            held("colstats", R.reduced_err(host(got), np.stack([q0.sum(axis=0), q1.sum(axis=0)]), np.stack([R.abs_sum(q0), R.abs_sum(q1)])), "colstats C=1024")
        else:
            refused(colsum(ncs, out(Cn)), "colsum with C = %d" % Cn)


@pytest.mark.parametrize("B,HW,Cn,ldx", R.IMAGE_CASES + R.COLSUM_LD_CASES)
def test_image_colsum_and_colsum_ld(lib, B, HW, Cn, ldx):
    """ams_k_image_colsum with B = 1 and 3 at HW = 1, S and 113 S, and ams_k_colsum with ldx = C and ldx = C + 8 (the columns behind C hold
    poison); the scratch refusals of both."""
    slots = max(1, 256 // (Cn // 4))
    assert plan(lib, HW, Cn, B) == (Cn // 4, slots) + R.col_plan(HW, Cn)[2:]
    if (B, HW, Cn, ldx) in R.IMAGE_CASES:
        assert R.col_plan(HW, Cn)[2] == {1: 1, 16 * slots: 1, 113 * 16 * slots: 113}[HW], "the case does not reach the path it is named for"
    ref, terms, _ = R.image_colsum_reference(B, HW, Cn, ldx)
    xd = dev(R.image_colsum_x(B, HW, Cn, ldx))
    what = "B=%d HW=%d C=%d ldx=%d" % (B, HW, Cn, ldx)
    n = lib.ams_k_image_colsum_scratch(B, Cn)
    assert n == B * 1024 * Cn
    scr = G.scratch(n)
    refused(lib.ams_k_image_colsum(P(xd), B, HW, Cn, ldx, P(out((B, Cn))), P(scr), n - 1, stream()), "image_colsum with one scratch float too few")

    def image_colsum():
        y = out((B, Cn))
        run(lib.ams_k_image_colsum(P(xd), B, HW, Cn, ldx, P(y), P(scr), n, stream()), "image_colsum")
        return y
    held("colsum", R.reduced_err(host(twice(image_colsum, what)), ref, terms), what)
    if B == 1:
        n1 = lib.ams_k_colsum_scratch(Cn)
        scr1 = G.scratch(n1)

        def colsum():
            y = out(Cn)
            run(lib.ams_k_colsum(P(xd), HW, Cn, ldx, P(y), P(scr1), n1, stream()), "colsum")
            return y
        held("colsum", R.reduced_err(host(twice(colsum, what)), ref[0], terms[0]), what + " (colsum)")


# ------------------------------------------------------------------------------------------------ second stages over partial rows
@pytest.mark.parametrize("rows", R.FOLD_ROWS)
@pytest.mark.parametrize("Cn", R.FOLD_CHANNELS)
def test_second_stages_over_partial_rows(lib, Cn, rows):
    """ams_k_partials_to_sums, ams_k_bn_fwd_partials and ams_k_bn_bwd_partials over rows [rows][2][C], dense and 2 C + 1093 floats apart with
    poison between the rows and nothing but guard behind the last: the fold against f64; the fused per-channel results bit for bit against
    ams_k_partials_to_sums + ams_k_bn_finalize | ams_k_bn_bwd_coef (the same kernel template with a different Fin).  rows 113: the first the
    8-in-flight loop touches (kpart 0 alone); 276: the 8-frame stride-16 GEMM's; 2048: the cap of pointwise_red's part."""
    for kind in ("fwd", "bwd"):
        part, n, p, center = R.partial_rows(rows, Cn, kind)
        flat = part.reshape(rows, 2 * Cn)
        ref, terms = flat.astype(F64).sum(axis=0).reshape(2, Cn), R.abs_sum(flat.astype(F64)).reshape(2, Cn)
        ch = Chan(p, center if kind == "fwd" else None)
        for row_stride in (0, 2 * Cn + 1093):
            what = "%s rows=%d C=%d row_stride=%d" % (kind, rows, Cn, row_stride)
            pd = dev(R.strided_rows(flat, row_stride or 2 * Cn))

            def to_sums():
                s = out((2, Cn), torch.float64)
                run(lib.ams_k_partials_to_sums(P(pd), rows, row_stride, Cn, P(s), stream()), "partials_to_sums")
                return s
            sums = twice(to_sums, what)
            held("fold_f64", R.reduced_err(host(sums), ref, terms), what)
            if kind == "fwd":
                sums_f, fused = twice(lambda: bn_fwd_partials(lib, pd, rows, row_stride, Cn, n, ch), what)
                want = bn_finalize(lib, sums, n, Cn, ch)
            else:
                sums_f, fused = twice(lambda: bwd_partials(lib, pd, rows, row_stride, Cn, n, ch), what)
                want = bwd_coef_and_grads(lib, sums, n, Cn, ch)
            bits(sums_f, sums, what + ": the fused stage's sums against partials_to_sums")
            held("fold_f64", R.reduced_err(host(sums_f), ref, terms), what + " (fused)")
            same_dict(fused, want, what + ": the fused stage against partials_to_sums + the per-channel kernel")


def test_second_stage_refusals(lib):
    Cn, rows = 24, 17
    part, n, p, center = R.partial_rows(rows, Cn, "fwd")
    pd, ch = dev(R.strided_rows(part.reshape(rows, 2 * Cn), 2 * Cn)), Chan(p, center)
    for rws, stride in ((0, 0), (rows, 2 * Cn - 1), (rows, -1)):
        refused(lib.ams_k_partials_to_sums(P(pd), rws, stride, Cn, P(out((2, Cn), torch.float64)), stream()), "partials_to_sums rows=%d stride=%d" % (rws, stride))
    refused(lib.ams_k_partials_to_sums(None, rows, 0, Cn, P(out((2, Cn), torch.float64)), stream()), "partials_to_sums without rows")


@pytest.mark.parametrize("Cn", [24, 960])
def test_a_row_too_many_or_the_wrong_stride_reads_poison(lib, Cn):
    """What the buffers of the test above are for: told one row more than there is, or the dense stride where the rows lie 2 C + 1093 apart, the
    stage reads cells that hold the pattern (all inside the guarded buffer), and every sum it touches is NaN."""
    rows = 17
    part = R.partial_rows(rows, Cn, "fwd")[0].reshape(rows, 2 * Cn)
    for stride, told_rows, told_stride in ((2 * Cn, rows + 1, 0), (2 * Cn + 1093, rows + 1, 2 * Cn + 1093), (2 * Cn + 1093, rows, 0)):
        pd = dev(R.strided_rows(part, stride))
        sums = out((2, Cn), torch.float64)
        run(lib.ams_k_partials_to_sums(P(pd), told_rows, told_stride, Cn, P(sums), stream()), "partials_to_sums")
        assert np.isnan(host(sums)).all(), (stride, told_rows, told_stride)


# ------------------------------------------------------------------------------------------------ the per-channel arithmetic against f64
@pytest.mark.parametrize("Cn", R.CHANNELS + (1024,))
def test_per_channel_arithmetic_against_f64(lib, Cn):
    """ams_k_bn_finalize, ams_k_bn_bwd_coef (+ ams_k_bn_param_grads) and ams_k_bn_fold given the SAME f64 sums as the f64 formula: the biased
    variance in rstd, the unbiased one (n / (n - 1); n = 1: divisor 1) in the moving variance, coefB with its k mean term, dgamma and dbeta."""
    for n in R.FINALIZE_N:
        for centre in R.CENTERS:
            what = "C=%d n=%d centre=%s" % (Cn, n, centre)
            sums, p, center = R.finalize_case(Cn, n, centre)
            ch, sd = Chan(p, center), dev(sums, torch.float64)
            got = twice(lambda: bn_finalize(lib, sd, float(n), Cn, ch), what)
            ref = R.finalize_f64(sums, float(n), center, p["gamma"], p["beta"], R.EPS, R.ONE_MINUS_DECAY, p["moving_mean"], p["moving_var"])
            for k in FWD_KEYS:
                held("finalize." + k, R.channel_err(host(got[k]), ref[k]), what + " " + k)
            if n == 1:
                assert np.isfinite(host(got["moving_var"])).all()
        if n == 1:
            continue
        for act in R.ACTS:
            what = "C=%d n=%d act=%d" % (Cn, n, act)
            sums, terms, p = R.bwd_coef_case(Cn, n, act)
            ch, sd = Chan(p, None), dev(sums, torch.float64)

            def coef():
                o = [out(Cn) for _ in range(5)]
                run(lib.ams_k_bn_bwd_coef(P(sd), float(n), Cn, P(ch.gamma), P(ch.mean), P(ch.rstd), *[P(t) for t in o], stream()), "bn_bwd_coef")
                return dict(zip(BWD_KEYS, o))
            got = twice(coef, what)
            same_dict(got, twice(lambda: bwd_coef_and_grads(lib, sd, float(n), Cn, ch), what), what + ": bn_bwd_coef's dgamma / dbeta against bn_param_grads")
            ref = R.bwd_coef_f64(sums, float(n), p["gamma"], p["mean"], p["rstd"])
            for k in ("cA", "cB", "cC"):
                held("bwd_coef." + k, R.channel_err(host(got[k]), ref[k]), what + " " + k)
            held("bwd_coef.dgamma", R.reduced_err(host(got["dgamma"]), ref["dgamma"], terms[1]), what)
            held("bwd_coef.dbeta", R.reduced_err(host(got["dbeta"]), ref["dbeta"], terms[0]), what)
    p = R.channel_params(Cn, False)
    ops = [dev(p[k]) for k in ("gamma", "beta", "moving_mean", "moving_var")]

    def fold():
        sc, sh = out(Cn), out(Cn)
        run(lib.ams_k_bn_fold(*[P(t) for t in ops], EPS, Cn, P(sc), P(sh), stream()), "bn_fold")
        return dict(scale=sc, shift=sh)
    got, ref = twice(fold, "bn_fold"), R.bn_fold_f64(p["gamma"], p["beta"], p["moving_mean"], p["moving_var"], R.EPS)
    for k in ref:
        held("bn_fold." + k, R.channel_err(host(got[k]), ref[k]), "bn_fold C=%d %s" % (Cn, k))


# ------------------------------------------------------------------------------------------------ apply passes
WRAP_M = 1048576 + 5                     # at C = 4 one float4 per row: stream_grid caps the grid at 4096 blocks of 256, so the last 5 wrap


@pytest.mark.parametrize("Cn,M", [(c, m) for c in (4, 16, 24, 960) for m in (1, 3, 257)] + [(4, WRAP_M)])
def test_apply_passes_bit_for_bit(lib, Cn, M):
    """ams_k_bn_act (with and without the residual) and ams_k_bn_bwd_apply (out of place and with dz = da) against the f32 restatement, bit for
    bit, for the three activations.  Channels 1 and 2 are planted: y is exactly 0 and 6 there, a is 0 and 6, Relu6Grad is 0 at both knees."""
    p = R.channel_params(Cn, True)
    z0, da = R.draw(M, Cn, True)
    res = R.draw(M, Cn, True, seed=3)[1]
    z, scale, shift = R.plant_knees(z0, p["scale"], p["shift"])
    zd, dad, resd, scd, shd = dev(z), dev(da), dev(res), dev(scale), dev(shift)
    cA, cB, cC = dev(p["cA"]), dev(p["cB"]), dev(p["cC"])
    for act in R.ACTS:
        for r, rd in ((None, None), (res, resd)):
            what = "bn_act C=%d M=%d act=%d res=%s" % (Cn, M, act, r is not None)

            def bn_act():
                a = out((M, Cn))
                run(lib.ams_k_bn_act(P(zd), M, Cn, P(scd), P(shd), act, P(rd), P(a), stream()), "bn_act")
                return a
            a = host(twice(bn_act, what))
            bits(a, R.bn_act_f32(z, scale, shift, act, r), what + ": not the f32 restatement")
            if act == R.ACT_RELU6 and r is None:
                assert (a[:, 1] == 0).all() and (a[:, 2] == 6).all(), what
        what = "bn_bwd_apply C=%d M=%d act=%d" % (Cn, M, act)
        want = R.bwd_apply_f32(da, z, scale, shift, act, p["cA"], p["cB"], p["cC"])

        def bwd_apply():
            dz = out((M, Cn))
            run(lib.ams_k_bn_bwd_apply(P(dad), P(zd), M, Cn, P(scd), P(shd), act, P(cA), P(cB), P(cC), P(dz), stream()), "bn_bwd_apply")
            return dz
        bits(twice(bwd_apply, what), want, what + ": not the f32 restatement")
        inplace = dev(da)                    # dz = da: read and written between the same guards
        run(lib.ams_k_bn_bwd_apply(P(inplace), P(zd), M, Cn, P(scd), P(shd), act, P(cA), P(cB), P(cC), P(inplace), stream()), "bn_bwd_apply in place")
        bits(inplace, want, what + " in place: not the f32 restatement")
        if act == R.ACT_RELU6:
            assert R.same_bits(want[:, 1:3], ((0 * da[:, 1:3] + p["cB"][1:3]) + p["cC"][1:3] * z[:, 1:3]).astype(F32)), "the mask is not 0 at the knees"


def test_apply_passes_refuse(lib):
    p = R.channel_params(16, True)
    z, da = R.draw(3, 16, True)
    zd, dad, sc, sh = dev(z), dev(da), dev(p["scale"]), dev(p["shift"])
    refused(lib.ams_k_bn_act(P(zd), 8, 6, P(sc), P(sh), 2, None, P(out((3, 16))), stream()), "bn_act with C = 6")
    refused(lib.ams_k_bn_act(P(zd), 3, 16, P(sc), P(sh), 3, None, P(out((3, 16))), stream()), "bn_act with an unknown activation")
    refused(lib.ams_k_bn_bwd_apply(P(dad), P(zd), 3, 16, P(sc), P(sh), 2, P(sc), None, P(sc), P(out((3, 16))), stream()), "bn_bwd_apply without coefB")


@pytest.mark.parametrize("n", R.L2_COUNTS)
def test_l2_regularizer(lib, n):
    """ams_k_l2_regularizer with no regularised entry, one, and the whole arena: the gradient pass bit for bit against its f32 restatement (the
    entries outside the mask keep their bits), the loss term against f64; 255 doubles of scratch are refused."""
    for which in R.L2_MASKS:
        p, g, mask, n_vars, coef, loss = R.l2_case(n, which)
        what = "l2_regularizer n=%d mask=%s" % (n, which)
        pd, md = dev(p), dev(mask, torch.uint8)

        def l2(nscr=256):
            gd, ld, scr = dev(g), dev(loss, torch.float64), G.scratch(256, torch.float64)
            rc = lib.ams_k_l2_regularizer(P(pd), P(gd), P(md), n, n_vars, float(coef), P(scr), nscr, P(ld), stream())
            if nscr < 256:
                refused(rc, what + " with 255 doubles of scratch")
            else:
                run(rc, what)
            return gd, ld
        gd, ld = twice(l2, what)
        bits(gd, R.l2_grads_f32(p, g, mask, n_vars, coef), what + ": the gradients are not the f32 restatement")
        want, terms = R.l2_loss_f64(p, mask, n_vars, coef, loss)
        got = host(ld)
        assert got[1] == loss[1]
        held("l2_loss", R.reduced_err(got[0], want, terms), what)
        gd, ld = l2(255)
        bits(gd, g, what + ": a refused call changed the gradients")
        bits(ld, loss, what + ": a refused call changed the loss")


# ------------------------------------------------------------------------------------------------ plain folds
def reduce_splits(lib, pd, splits, n, stride):
    y = out(n)
    run(lib.ams_k_reduce_splits(P(pd), splits, n, stride, P(y), stream()), "reduce_splits")
    return y


@pytest.mark.parametrize("splits", R.SPLITS_LP16 + R.SPLITS_LP64)
def test_reduce_splits(lib, splits):
    """16 lanes per output below 256 splits, 64 from there on; 113 | 449 splits are the first the 8-in-flight loop of each form touches.  Counts
    one below, at and above a block's 16 outputs; stride n and n + 37 with poison between the rows."""
    for n in R.SPLIT_COUNTS:
        part = R.split_rows(splits, n)
        ref, terms = part.astype(F64).sum(axis=0), R.abs_sum(part.astype(F64))
        for stride in (n, n + 37):
            what = "splits=%d n=%d stride=%d" % (splits, n, stride)
            pd = dev(R.strided_rows(part, stride))
            held("fold_f32", R.reduced_err(host(twice(lambda: reduce_splits(lib, pd, splits, n, stride), what)), ref, terms), what)
    refused(lib.ams_k_reduce_splits(P(pd), splits, n, n - 1, P(out(n)), stream()), "reduce_splits with stride < n")


def batch_call(lib, jobs):
    """jobs: [(part on the device, splits, count, stride)] -> the results"""
    k = len(jobs)
    outs = [out(j[2]) for j in jobs]
    rc = lib.ams_k_reduce_batch((C.c_void_p * k)(*[j[0].data_ptr() for j in jobs]), (C.c_int32 * k)(*[j[1] for j in jobs]),
                                (C.c_int64 * k)(*[j[2] for j in jobs]), (C.c_int64 * k)(*[j[3] for j in jobs]),
                                (C.c_void_p * k)(*[o.data_ptr() for o in outs]), k, stream())
    return rc, outs


@pytest.mark.parametrize("k,long_sums", [(1, False), (2, False), (32, False), (1, True), (2, True), (32, True)])
def test_reduce_batch_against_reduce_splits(lib, k, long_sums):
    """1, 2 and 32 jobs with counts 1, 15, 16, 17, 288 mixed in one launch, every job below 256 splits or every job from 1024 on: there both
    entries pick the same lanes per output, and each job has ams_k_reduce_splits' bits."""
    pool = (1024, 2048) if long_sums else R.SPLITS_LP16
    jobs, parts = [], []
    for j in range(k):
        splits, n = pool[j % len(pool)], R.SPLIT_COUNTS[(j + k) % len(R.SPLIT_COUNTS)]
        stride = n + (37 if j % 2 else 0)
        part = R.split_rows(splits, n, seed=j)
        parts.append(part)
        jobs.append((dev(R.strided_rows(part, stride)), splits, n, stride))

    def batch():
        rc, outs = batch_call(lib, jobs)
        run(rc, "reduce_batch")
        return outs
    outs = twice(batch, "reduce_batch of %d jobs" % k)
    for j, (pd, splits, n, stride) in enumerate(jobs):
        what = "job %d of %d: splits=%d n=%d stride=%d" % (j, k, splits, n, stride)
        bits(outs[j], reduce_splits(lib, pd, splits, n, stride), what + ": not reduce_splits' bits")
        held("fold_f32", R.reduced_err(host(outs[j]), parts[j].astype(F64).sum(axis=0), R.abs_sum(parts[j].astype(F64))), what)


def test_reduce_batch_short_job_beside_a_long_one_and_the_33rd_job(lib):
    """3 splits beside 1024: the launch takes 64 lanes per output, of which 61 find nothing to add in the short job; held against f64.  A
    33rd job is refused before any launch."""
    jobs, parts = [], []
    for splits, n in ((3, 17), (1024, 288)):
        parts.append(R.split_rows(splits, n, seed=5))
        jobs.append((dev(R.strided_rows(parts[-1], n + 37)), splits, n, n + 37))
    rc, outs = batch_call(lib, jobs)
    run(rc, "reduce_batch")
    for j in range(2):
        held("fold_f32", R.reduced_err(host(outs[j]), parts[j].astype(F64).sum(axis=0), R.abs_sum(parts[j].astype(F64))), "short beside long, job %d" % j)
    rc, outs = batch_call(lib, [jobs[0]] * 33)
    refused(rc, "reduce_batch of 33 jobs")
