"""The BN pieces of the fine-tune step (k_elementwise.hip: column reductions, second stages over partial rows, the per-channel arithmetic, the
apply passes, the plain folds), each alone: the reference, the cases, the measure and the bars of tests/test_bn_pieces_cpu.py and
tests/test_gpu_bn_pieces.py.  A helper, not a conftest: nothing here runs a kernel.

THE REFERENCE of every piece is its formula in NumPy f64 (`*_f64`), and beside it an F32 RESTATEMENT (`*_f32`): the same formula one IEEE f32
operation at a time, in the order the kernel's source states them (the library is built with -ffp-contract=off and the packed helpers are unfused,
so an elementwise f32 quantity has one right answer).  The first reduction stage is restated too (`first_stage_f32`): a thread adds every slots-th
row of its chunk in f32, the block adds its slots' sums in f32, slot 0 first; `col_plan` is the geometry (the tests hold ams_k_col_plan to it).
The second stages add f32 partial rows in f64, so their restatement is the f64 sum, rounded once where the result is f32.

OPERANDS.  z[:, c] = mu_c + sigma_c N(0, 1) with sigma_c log-uniform over two decades [0.1, 10]; |mu_c| in [0.5, 2] sigma_c where the centre is
NULL, up to 20 sigma_c where a centre is given; the centre is NULL, mu_c or mu_c + 0.5 sigma_c: a moving mean that tracks its batch.  (Centres far
from the batch mean are out of scope: (z - c)^2 then loses the variance in f32, which is image_pooling's f64 path.)  beta has the sign opposite
to the batch mean's (gamma > 0), so `shift = beta - mean scale` does not cancel; the apply passes get shifts that put both knees of ReLU6 inside every channel,
and two planted channels (scale 0.5, shift -1, z = 2 and z = 14) whose y is EXACTLY 0 and 6 in f32 and in f64.

THE MEASURE.  Reduced quantities: max |got - ref| / max sum |terms| (`reduced_err`; dgamma and dbeta are sums and are measured
so).  Per-channel scalars: |got - ref| / |ref| per channel, the worst channel (`channel_err`); the per-channel arithmetic is always given the
SAME f64 sums as its reference, so what is measured is that arithmetic, not the conditioning of `sums[1] / n - d1^2`.

THE BARS come from the reference alone: L = the worst value of the measure for the f32 restatement against f64 over the family's cases, at least
2^-23 (one ulp of a correctly rounded sqrt or division must not fail a case whose restatement happens to be exact); bar = 4 L.  No bar may exceed
2e-5, the reduction bar of tests/test_gpu_kernels.py (a condition on the operand regime, asserted on the CPU).

DEFECTS are made on the restatement's output (test_bn_pieces_cpu.py): each must fail the check it belongs to.
"""
from __future__ import annotations

import functools
from typing import Dict, Iterator, Optional, Tuple

import numpy as np

F32, F64 = np.float32, np.float64
ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2
ACTS = (ACT_NONE, ACT_RELU, ACT_RELU6)
FLOOR, FACTOR, BAR_CAP = 2.0 ** -23, 4.0, 2e-5
MAX_CHUNKS = 1024                        # kMaxChunks of col_geom
EPS, ONE_MINUS_DECAY = F32(1e-3), F32(1.0 - 0.9997)
POISON = np.array([0x7FC12345], dtype=np.uint32).view(F32)[0]          # guarded.F32_PATTERN: a NaN


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ geometry and cases
def col_plan(M: int, C: int) -> Tuple[int, int, int, int]:
    """(CG, slots, chunks, rows_per_chunk): col_geom restated"""
    CG = C // 4
    slots = max(1, 256 // CG)
    chunks = max(1, min(MAX_CHUNKS, cdiv(M, 16 * slots)))
    return CG, slots, chunks, cdiv(M, chunks)


CHANNELS = (16, 24, 144, 576, 960)       # slots 64, 42, 7, 1, 1; block 256, 252, 252, 144, 240 threads
CHANNEL_SLOTS = {16: 64, 24: 42, 144: 7, 576: 1, 960: 1, 1024: 1}
BIG = 113                                # from this many chunks on a case counts as large: one operand variant, not all of them

# name -> (M, chunks, rows_per_chunk) as functions of (slots, S = 16 slots): the path the row count is named for
ROWS = {
    "1": (lambda sl, S: 1, lambda sl, S: 1, lambda sl, S: 1),
    "4 slots - 1": (lambda sl, S: 4 * sl - 1, lambda sl, S: 1, lambda sl, S: 4 * sl - 1),      # the four-rows-in-flight loop not entered ...
    "4 slots": (lambda sl, S: 4 * sl, lambda sl, S: 1, lambda sl, S: 4 * sl),                    # ... entered once by every slot, no tail ...
    "4 slots + 1": (lambda sl, S: 4 * sl + 1, lambda sl, S: 1, lambda sl, S: 4 * sl + 1),      # ... and a tail row for slot 0
    "S - 1": (lambda sl, S: S - 1, lambda sl, S: 1, lambda sl, S: S - 1),
    "S": (lambda sl, S: S, lambda sl, S: 1, lambda sl, S: S),
    "S + 1": (lambda sl, S: S + 1, lambda sl, S: 2, lambda sl, S: cdiv(S + 1, 2)),
    "113 S": (lambda sl, S: 113 * S, lambda sl, S: 113, lambda sl, S: S),                       # chunk 113: the 8-in-flight loop, kpart 0 alone
    "129 S": (lambda sl, S: 129 * S, lambda sl, S: 129, lambda sl, S: S),
    "241 S + 1": (lambda sl, S: 241 * S + 1, lambda sl, S: 242, lambda sl, S: cdiv(241 * S + 1, 242)),
    "1024 S + 1": (lambda sl, S: 1024 * S + 1, lambda sl, S: MAX_CHUNKS, lambda sl, S: S + 1),  # capped: rows_per_chunk above 16 slots
}


def rows_case(C: int, name: str) -> Tuple[int, int, int]:
    """(M, chunks, rows_per_chunk) the case must reach"""
    sl = CHANNEL_SLOTS[C]
    m, ch, rpc = ROWS[name]
    return m(sl, 16 * sl), ch(sl, 16 * sl), rpc(sl, 16 * sl)


def empty_chunks(M: int, chunks: int, rpc: int) -> int:
    """trailing chunks whose r_begin lies at or past the end of the tensor"""
    return chunks - cdiv(M, rpc)


CENTERS = ("null", "mean", "half")       # center == NULL | mu | mu + 0.5 sigma


def direct_cases() -> Iterator[Tuple[int, str, str, int]]:
    """(C, rows name, centre, act): every row count with every channel count; the small ones with every centre and every activation, the
    large ones (BIG chunks or more) with one of each, rotating."""
    i = 0
    for C in CHANNELS:
        for name in ROWS:
            i += 1
            for v in range(3 if rows_case(C, name)[1] < BIG else 1):
                yield C, name, CENTERS[(v + i) % 3], ACTS[(2 * v + i) % 3]


# ------------------------------------------------------------------------------------------------ operands
def _ro(a: np.ndarray) -> np.ndarray:
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def channel_params(C: int, far: bool) -> Dict[str, np.ndarray]:
    """per-channel operands, f32.  far: |mu| up to 20 sigma (for use with a centre)"""
    rng = np.random.default_rng(7 * C + (1 if far else 0))
    sigma = 10.0 ** rng.uniform(-1.0, 1.0, C)
    sign = np.where(rng.random(C) < 0.5, -1.0, 1.0)
    mu = sign * sigma * rng.uniform(0.5, 20.0 if far else 2.0, C)
    gamma = rng.uniform(0.5, 1.5, C)
    p = dict(sigma=sigma, mu=mu, gamma=gamma, beta=-sign * rng.uniform(0.1, 1.0, C),
             moving_mean=mu + 0.3 * sigma * rng.standard_normal(C), moving_var=sigma ** 2 * rng.uniform(0.5, 2.0, C),
             gscale=10.0 ** rng.uniform(-1.0, 1.0, C))
    p = {k: _ro(v.astype(F32)) for k, v in p.items()}
    # what the backward pieces and the apply passes are handed: saved statistics near the batch's, y = gamma xhat + b with b in (0, 6)
    p["mean"] = p["mu"]
    p["rstd"] = _ro((F32(1.0) / p["sigma"]).astype(F32))
    p["scale"] = _ro((p["gamma"] * p["rstd"]).astype(F32))
    p["shift"] = _ro((rng.uniform(0.5, 5.5, C).astype(F32) - p["mean"] * p["scale"]).astype(F32))
    p["cA"] = p["scale"]
    p["cB"] = _ro((rng.standard_normal(C) * p["gscale"] * 0.1).astype(F32))
    p["cC"] = _ro((rng.standard_normal(C) * p["gscale"] / p["sigma"] * 0.1).astype(F32))
    return p


def center_of(p: Dict[str, np.ndarray], mode: str) -> Optional[np.ndarray]:
    if mode == "null":
        return None
    return p["mu"] if mode == "mean" else (p["mu"] + F32(0.5) * p["sigma"]).astype(F32)


def draw(M: int, C: int, far: bool, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """(z, da) [M, C] f32"""
    p = channel_params(C, far)
    rng = np.random.default_rng(M * 131 + C + (5 if far else 0) + seed)
    z = rng.standard_normal((M, C), dtype=F32)
    z *= p["sigma"]
    z += p["mu"]
    da = rng.standard_normal((M, C), dtype=F32)
    da *= p["gscale"]
    return _ro(z), _ro(da)


def plant_knees(z: np.ndarray, scale: np.ndarray, shift: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """channels 1 and 2: scale 0.5, shift -1, z = 2 | 14: y = 0 | 6 exactly"""
    z, scale, shift = z.copy(), scale.copy(), shift.copy()
    scale[1:3], shift[1:3] = 0.5, -1.0
    z[:, 1], z[:, 2] = 2.0, 14.0
    return _ro(z), _ro(scale), _ro(shift)


# ------------------------------------------------------------------------------------------------ elementwise pieces
def y_f32(z, scale, shift):
    assert z.dtype == F32 and scale.dtype == F32 and shift.dtype == F32
    return (z * scale) + shift                               # two f32 operations


def act_mask(y, act, le6=False):
    """Relu6Grad: 0 < y < 6, strictly.  le6: the defect `<= 6`"""
    if act == ACT_RELU6:
        return ((y > 0) & ((y <= 6) if le6 else (y < 6))).astype(y.dtype)
    if act == ACT_RELU:
        return (y > 0).astype(y.dtype)
    return np.ones_like(y)


def apply_act(y, act):
    if act == ACT_RELU6:
        return np.minimum(np.maximum(y, y.dtype.type(0)), y.dtype.type(6))
    return np.maximum(y, y.dtype.type(0)) if act == ACT_RELU else y


def bn_act_f32(z, scale, shift, act, res=None):
    a = apply_act(y_f32(z, scale, shift), act)
    return a if res is None else a + res


def bn_act_f64(z, scale, shift, act, res=None):
    a = apply_act(z.astype(F64) * scale.astype(F64) + shift.astype(F64), act)
    return a if res is None else a + res.astype(F64)


def bwd_apply_f32(da, z, scale, shift, act, cA, cB, cC, le6=False):
    mk = act_mask(y_f32(z, scale, shift), act, le6)
    return ((cA * (da * mk)) + cB) + (cC * z)


def stats_terms_f32(z, center):
    q0 = z if center is None else z - center                 # (z - 0 = z exactly)
    return q0, q0 * q0


def stats_terms_f64(z, center):
    q0 = z.astype(F64) if center is None else z.astype(F64) - center.astype(F64)
    return q0, q0 * q0


def bwd_terms_f32(da, z, scale, shift, act, mean, rstd, le6=False):
    q0 = da * act_mask(y_f32(z, scale, shift), act, le6)
    return q0, (q0 * (z - mean)) * rstd


def bwd_terms_f64(da, z, mask, mean, rstd):
    """mask: the f32 restatement's (the bit-for-bit test of the apply pass pins the kernel's mask to it)"""
    q0 = da.astype(F64) * mask.astype(F64)
    return q0, q0 * (z.astype(F64) - mean.astype(F64)) * rstd.astype(F64)


# ------------------------------------------------------------------------------------------------ reductions
def first_stage_f32(terms: np.ndarray, drop_last_row_of_chunk: Optional[int] = None) -> np.ndarray:
    """[M, C] f32 terms -> the partial rows [chunks, C] f32 of col_reduce_kernel, its order of additions"""
    M, C = terms.shape
    _, slots, chunks, rpc = col_plan(M, C)
    steps = cdiv(rpc, slots)
    pad = np.zeros((chunks, steps * slots, C), F32)          # (x + 0 = x: padding changes no sum)
    full = M // rpc
    pad[:full, :rpc] = terms[:full * rpc].reshape(full, rpc, C)
    if full * rpc < M:
        pad[full, :M - full * rpc] = terms[full * rpc:]
    if drop_last_row_of_chunk is not None:
        k = drop_last_row_of_chunk
        pad[k, min(rpc, M - k * rpc) - 1] = 0
    pad = pad.reshape(chunks, steps, slots, C)
    acc = np.zeros((chunks, slots, C), F32)
    for s in range(steps):
        acc += pad[:, s]
    tot = np.zeros((chunks, C), F32)
    for sl in range(slots):
        tot += acc[:, sl]
    return tot


def fold_f64(rows: np.ndarray) -> np.ndarray:
    """sum over the leading axis in f64"""
    return rows.astype(F64).sum(axis=0)


def abs_sum(terms64: np.ndarray) -> np.ndarray:
    return np.abs(terms64).sum(axis=0)


def strided_rows(rows: np.ndarray, stride: int) -> np.ndarray:
    """[R, n] -> a flat buffer (R - 1) stride + n long: row r at r * stride, POISON everywhere else (nothing behind the last row)"""
    R, n = rows.shape
    assert stride >= n
    buf = np.full((R - 1) * stride + n, POISON, F32)
    idx = (np.arange(R)[:, None] * stride + np.arange(n)[None, :]).reshape(-1)
    buf[idx] = rows.reshape(-1)
    return buf


def read_rows(buf: np.ndarray, R: int, n: int, stride: int) -> np.ndarray:
    """what a stage reading R rows of n floats `stride` apart sees; POISON behind the buffer's end (the guard)"""
    idx = np.arange(R)[:, None] * stride + np.arange(n)[None, :]
    ext = np.concatenate([buf, np.full(max(0, int(idx.max()) + 1 - buf.size), POISON, F32)])
    return ext[idx]


# ------------------------------------------------------------------------------------------------ per-channel arithmetic
def _n_unbiased(n: float) -> float:
    return n / (n - 1.0) if n > 1.5 else 1.0


def finalize_f64(sums, n, center, gamma, beta, eps, omd, moving_mean, moving_var, n_mean=None, biased_moving=False):
    """sums [2][C] f64 -> dict of f64.  n_mean, biased_moving: the defects `n - 1 in place of n` and `the biased variance in the moving one`"""
    d = F64
    nn = n if n_mean is None else n_mean
    ctr = 0.0 if center is None else center.astype(d)
    d1, d2 = sums[0] / nn, sums[1] / nn
    var = np.maximum(d2 - d1 * d1, 0.0)
    mean = ctr + d1
    rstd = 1.0 / np.sqrt(var + d(eps))
    scale = gamma.astype(d) * rstd
    unb = var * (1.0 if biased_moving else _n_unbiased(n))
    return dict(mean=mean, rstd=rstd, scale=scale, shift=beta.astype(d) - mean * scale,
                moving_mean=moving_mean.astype(d) - (moving_mean.astype(d) - mean) * d(omd),
                moving_var=moving_var.astype(d) - (moving_var.astype(d) - unb) * d(omd))


def finalize_f32(sums, n, center, gamma, beta, eps, omd, moving_mean, moving_var, n_mean=None, biased_moving=False):
    """BnFwdFin / bn_finalize_kernel: f64 up to the variance, then f32 one operation at a time"""
    nn = n if n_mean is None else n_mean
    ctr = 0.0 if center is None else center.astype(F64)
    d1, d2 = sums[0] / nn, sums[1] / nn
    var = np.maximum(d2 - d1 * d1, 0.0)
    mean = (ctr + d1).astype(F32)
    rstd = F32(1.0) / np.sqrt(var.astype(F32) + F32(eps))
    scale = gamma * rstd
    unb = (var * (1.0 if biased_moving else _n_unbiased(n))).astype(F32)
    out = dict(mean=mean, rstd=rstd, scale=scale, shift=beta - mean * scale,
               moving_mean=moving_mean - (moving_mean - mean) * F32(omd), moving_var=moving_var - (moving_var - unb) * F32(omd))
    assert all(v.dtype == F32 for v in out.values())
    return out


def bwd_coef_f64(sums, n, gamma, mean, rstd, no_k_mean=False, swapped=False):
    """coefA, coefB, coefC of dz = A dy + B + C z, and dgamma = sums[1], dbeta = sums[0]; the defects `coefB without k mean`, `swapped`"""
    d = F64
    A = gamma.astype(d) * rstd.astype(d)
    k = A * (sums[1] / n) * rstd.astype(d)
    cB = -A * (sums[0] / n) + (0.0 if no_k_mean else k * mean.astype(d))
    dg, db = (sums[0], sums[1]) if swapped else (sums[1], sums[0])
    return dict(cA=A, cB=cB, cC=-k, dgamma=dg.copy(), dbeta=db.copy())


def bwd_coef_f32(sums, n, gamma, mean, rstd, **defect):
    """BnBwdFin / bn_bwd_coef_kernel: f64 throughout, rounded once"""
    return {k: v.astype(F32) for k, v in bwd_coef_f64(sums, n, gamma, mean, rstd, **defect).items()}


def bn_fold_f64(gamma, beta, mean, var, eps):
    sc = gamma.astype(F64) / np.sqrt(var.astype(F64) + F64(eps))
    return dict(scale=sc, shift=beta.astype(F64) - mean.astype(F64) * sc)


def bn_fold_f32(gamma, beta, mean, var, eps):
    sc = gamma * (F32(1.0) / np.sqrt(var + F32(eps)))
    return dict(scale=sc, shift=beta - mean * sc)


def l2_grads_f32(p, g, mask, n_vars, coef):
    """g + (coef / n_vars) p where the mask is set, two f32 operations; g elsewhere"""
    gs = F32(coef) / F32(n_vars)
    return np.where(mask != 0, g + gs * p, g)


def l2_loss_f64(p, mask, n_vars, coef, loss):
    """(loss[0] + 0.5 coef / n_vars sum_mask p^2 loss[1], the sum of the two terms' magnitudes); coef at its f32 value"""
    add = 0.5 * F64(F32(coef)) / n_vars * (p.astype(F64) ** 2)[mask != 0].sum() * loss[1]
    return loss[0] + add, abs(loss[0]) + abs(add)


L2_COUNTS = (1, 65536 + 3, 3 * 65536 + 77)       # the launch has 256 blocks of 256 threads: one entry, one wrap and a few
L2_MASKS = ("none", "one", "all")


def l2_case(n: int, which: str):
    rng = np.random.default_rng(n)
    p, g = rng.standard_normal(n, dtype=F32), rng.standard_normal(n, dtype=F32) * F32(0.01)
    mask = np.full(n, 255 if which == "all" else 0, np.uint8)
    if which == "one":
        mask[n // 2] = 1
    return _ro(p), _ro(g), _ro(mask), 7, F32(0.01), np.array([12.5, 4096.0])


# ------------------------------------------------------------------------------------------------ the measure
def reduced_err(got, ref, abs_terms) -> float:
    """max |got - ref| / max sum |terms|; NaN if anything is not finite"""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if not np.isfinite(got).all():
        return float("nan")
    return float(np.abs(got - ref).max() / max(float(np.max(abs_terms)), 1e-300))


def channel_err(got, ref) -> float:
    """|got - ref| / |ref| per channel (the last axis; max over the others of each), the worst channel.  A channel whose reference is zero
    must be zero."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    if not np.isfinite(got).all():
        return float("nan")
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    num, den = np.abs(got - ref).max(axis=0), np.abs(ref).max(axis=0)
    r = np.where(den > 0, num / np.where(den > 0, den, 1.0), np.where(num > 0, np.inf, 0.0))
    return float(r.max())


def within(err: float, bar: float) -> bool:
    return bool(err <= bar)                 # False for NaN


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool(np.array_equal(a.view(np.uint8), b.view(np.uint8)))


# ------------------------------------------------------------------------------------------------ levels and bars
def direct_operands(C: int, name: str, centre: str):
    """(M, p, z, da, center) of a direct-reduction case"""
    M = rows_case(C, name)[0]
    far = centre != "null"
    p = channel_params(C, far)
    z, da = draw(M, C, far)
    return M, p, z, da, center_of(p, centre)


@functools.lru_cache(maxsize=None)
def direct_reference(C: int, name: str, centre: str, act: int) -> Dict[str, Tuple[np.ndarray, np.ndarray, np.ndarray]]:
    """family -> (f64 sums [NQ][C], sum |terms| [NQ][C], the f32 restatement's sums [NQ][C]) of one case"""
    M, p, z, da, center = direct_operands(C, name, centre)
    out = {}
    for fam, t32, t64 in (
            ("colstats", stats_terms_f32(z, center), stats_terms_f64(z, center)),
            ("bn_bwd_reduce", bwd_terms_f32(da, z, p["scale"], p["shift"], act, p["mean"], p["rstd"]),
             bwd_terms_f64(da, z, act_mask(y_f32(z, p["scale"], p["shift"]), act), p["mean"], p["rstd"])),
            ("colsum", (z,), (z.astype(F64),))):
        f32 = np.stack([fold_f64(first_stage_f32(np.ascontiguousarray(t))) for t in t32])
        out[fam] = (np.stack([t.sum(axis=0) for t in t64]), np.stack([abs_sum(t) for t in t64]),
                    f32.astype(F32) if fam == "colsum" else f32)              # (ams_k_colsum's result is f32: rounded once more)
    return out


# B, HW, C, ldx of ams_k_image_colsum (S = 1024 rows at 16 channels, 112 at 144) and M, C, ldx of ams_k_colsum beyond the direct cases (B = 1 here);
# 257 x 32 at ldx 32 is the engine's own use, on dlogits
IMAGE_CASES = tuple((B, HW, Cn, Cn + (8 if B == 3 else 0)) for Cn in (16, 144) for B in (1, 3) for HW in (1, 16 * CHANNEL_SLOTS[Cn], 113 * 16 * CHANNEL_SLOTS[Cn]))
COLSUM_LD_CASES = ((1, 257, 32, 32), (1, 257, 32, 40), (1, 1025, 16, 24), (1, 113 * 112, 144, 152))


@functools.lru_cache(maxsize=None)
def image_colsum_x(B: int, HW: int, C: int, ldx: int) -> np.ndarray:
    """x [B HW, ldx] f32: the first C columns hold values, the others POISON"""
    x = np.full((B * HW, ldx), POISON, F32)
    x[:, :C] = draw(B * HW, C, False, seed=23)[0]
    return _ro(x)


@functools.lru_cache(maxsize=None)
def image_colsum_reference(B: int, HW: int, C: int, ldx: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(f64 sums [B][C], sum |terms| [B][C], the f32 restatement [B][C] f32)"""
    x = image_colsum_x(B, HW, C, ldx)[:, :C].reshape(B, HW, C)
    return (x.astype(F64).sum(axis=1), np.abs(x.astype(F64)).sum(axis=1),
            np.stack([fold_f64(first_stage_f32(np.ascontiguousarray(x[b]))) for b in range(B)]).astype(F32))


FINALIZE_N = (1, 2, 257, 16384)          # n = 1 keeps the divisor 1; 2 is the largest n / (n - 1)


def finalize_case(C: int, n: int, centre: str):
    """(sums f64 [2][C] of a batch of n rows about the centre, p, center): the SAME sums go to the kernel and to the reference"""
    far = centre != "null"
    p = channel_params(C, far)
    center = center_of(p, centre)
    z, _ = draw(n, C, far, seed=11)
    q0, q1 = stats_terms_f64(z, center)
    # beta against the sign of THIS batch's mean (a batch of one or two rows can lie on the other side of zero than mu)
    batch_mean = z.astype(F64).mean(axis=0)
    p = dict(p, beta=_ro((-np.sign(batch_mean) * np.abs(p["beta"])).astype(F32)))
    return np.stack([q0.sum(axis=0), q1.sum(axis=0)]), p, center


def bwd_coef_case(C: int, n: int, act: int):
    p = channel_params(C, True)
    z, da = draw(n, C, True, seed=13)
    q0, q1 = bwd_terms_f64(da, z, act_mask(y_f32(z, p["scale"], p["shift"]), act), p["mean"], p["rstd"])
    return np.stack([q0.sum(axis=0), q1.sum(axis=0)]), np.stack([abs_sum(q0), abs_sum(q1)]), p


FOLD_ROWS = (1, 15, 16, 17, 112, 113, 128, 129, 241, 276, 2048)      # 276: the 8-frame stride-16 GEMM's rows; 2048: the cap of pointwise_red's part
FOLD_CHANNELS = (16, 24, 960)
SPLITS_LP16 = (1, 15, 16, 17, 112, 113, 128, 129, 255)
SPLITS_LP64 = (256, 448, 449, 512, 513, 1024, 2048)
SPLIT_COUNTS = (1, 15, 16, 17, 288)
GROUP = 4                                # rows of z behind one partial row


@functools.lru_cache(maxsize=8)
def partial_rows(rows: int, C: int, kind: str, act: int = ACT_RELU6):
    """partial rows [rows][2][C] f32 as a fused kernel leaves them (each the f32 sums of GROUP rows of a batch of n = GROUP rows), with
    (n, p, center): kind "fwd" (about the centre mu + 0.5 sigma) or "bwd" """
    p = channel_params(C, True)
    center = center_of(p, "half")
    z, da = draw(rows * GROUP, C, True, seed=17)
    q0, q1 = stats_terms_f32(z, center) if kind == "fwd" else bwd_terms_f32(da, z, p["scale"], p["shift"], act, p["mean"], p["rstd"])
    part = np.stack([q0.reshape(rows, GROUP, C), q1.reshape(rows, GROUP, C)], axis=1)          # [rows, 2, GROUP, C]
    acc = np.zeros((rows, 2, C), F32)
    for g in range(GROUP):
        acc += part[:, :, g]
    return _ro(acc), float(rows * GROUP), p, center


def split_rows(splits: int, n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(splits * 1000 + n + seed)
    return _ro((rng.standard_normal((splits, n), dtype=F32) + F32(0.25)) * F32(3.0))


@functools.lru_cache(maxsize=None)
def levels() -> Dict[str, float]:
    """L per quantity: the f32 restatement against f64 under the measure, over the family's cases, at least FLOOR"""
    L: Dict[str, float] = {}

    def note(key, e):
        L[key] = max(L.get(key, FLOOR), e)

    for C, name, centre, act in direct_cases():
        for fam, (ref, terms, f32) in direct_reference(C, name, centre, act).items():
            note(fam, reduced_err(f32, ref, terms))
    for case in IMAGE_CASES + COLSUM_LD_CASES:
        ref, terms, f32 = image_colsum_reference(*case)
        note("colsum", reduced_err(f32, ref, terms))
    note("l2_loss", 0.0)                 # f64 throughout, like the reference: the floor
    note("colstats_f64", 0.0)            # every operation in f64, like the reference: the floor
    for C in FOLD_CHANNELS:              # f32 partial rows added in f64; f32 results rounded once
        for rows in FOLD_ROWS:
            for kind in ("fwd", "bwd"):
                part = partial_rows(rows, C, kind)[0]
                note("fold_f64", reduced_err(fold_f64(part), part.astype(F64).sum(axis=0), abs_sum(part.astype(F64))))
    for splits in SPLITS_LP16 + SPLITS_LP64:
        for n in SPLIT_COUNTS:
            part = split_rows(splits, n)
            note("fold_f32", reduced_err(fold_f64(part).astype(F32), part.astype(F64).sum(axis=0), abs_sum(part.astype(F64))))
    for C in CHANNELS + (1024,):
        for n in FINALIZE_N:
            for centre in CENTERS:
                sums, p, center = finalize_case(C, n, centre)
                args = (sums, float(n), center, p["gamma"], p["beta"], EPS, ONE_MINUS_DECAY, p["moving_mean"], p["moving_var"])
                r64, r32 = finalize_f64(*args), finalize_f32(*args)
                for k in r64:
                    note("finalize." + k, channel_err(r32[k], r64[k]))
        for n in FINALIZE_N[1:]:
            for act in ACTS:
                sums, terms, p = bwd_coef_case(C, n, act)
                r64, r32 = bwd_coef_f64(sums, float(n), p["gamma"], p["mean"], p["rstd"]), bwd_coef_f32(sums, float(n), p["gamma"], p["mean"], p["rstd"])
                for k in ("cA", "cB", "cC"):
                    note("bwd_coef." + k, channel_err(r32[k], r64[k]))
                note("bwd_coef.dgamma", reduced_err(r32["dgamma"], r64["dgamma"], terms[1]))
                note("bwd_coef.dbeta", reduced_err(r32["dbeta"], r64["dbeta"], terms[0]))
        p = channel_params(C, False)
        f64, f32 = bn_fold_f64(p["gamma"], p["beta"], p["moving_mean"], p["moving_var"], EPS), bn_fold_f32(p["gamma"], p["beta"], p["moving_mean"], p["moving_var"], EPS)
        for k in f64:
            note("bn_fold." + k, channel_err(f32[k], f64[k]))
    return L


def bar(key: str) -> float:
    return FACTOR * levels()[key]
