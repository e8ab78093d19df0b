"""The fine-tune loss and its gradient (ams_k_ce_loss_grad in its hard, soft, kd, weighted and mined forms, and the two-pass route
ams_k_upsample_argmax + ams_k_ce_grad) at tied, saturated and non-finite logits: the regimes of tests/logit_regimes.py, which
tests/test_logit_regimes_cpu.py holds to what they claim.

Reference: loss_ref.objective in f64 torch autograd on the f32-interpolated logits (ams_amd.confidence.interpolate_selected; the teacher's by
ams_amd.soft_metric.interpolate_teacher); the gradient reaches the low-resolution logits through the f64 transpose of the interpolation, which
is linear.

The loss is held by the absolute bound of tests/test_gpu_head_regimes.py: per pixel 2^-21 + c 2^-24 m, with m the largest magnitude that
enters the pixel's value,

    m = alpha T^2 (max |z| / T + log K) + (1 - alpha) (max |z| + log K),

times the pixel's weight under class weights and conf_gamma; the mean inherits the (weighted) mean of those bounds.  c per regime is twice the
worst ratio measured on MI355X, rounded up to a power of two (C_BOUND below says which quantity gave it): ties 2.971 -> 8,
saturated 1.882 -> 4, the call on the replaced logits of the non-finite frames 0 -> 1.  The gradient keeps the bars of the forms'
own tests: max |d - d64| / max |d64| < 2e-5 for the hard forms, 3e-5 for the others."""
import ctypes as C

import numpy as np
import pytest
import torch

import logit_regimes as LG
import loss_ref as LR
from ams_amd import confidence as Cf, hip, soft_metric as SM
from ams_amd.utils import mining_rank
from kernel_suite import P, _guarded_buffers, dev, lib, out, run, scratch, stream  # noqa: F401
from loss_ref import rel_err, same
from test_gpu_loss_mining import MIN_GAP, gap_rank, mined_call

pytestmark = pytest.mark.gpu

GRID, ULP = 2.0 ** -21, 2.0 ** -24
h, w, H, W = LG.LOSS_SHAPE

# regime -> c: twice the worst ratio measured on MI355X over the cases of this file, rounded up to a power of two.  The ratios: (|mean loss -
# f64| - the grid term) / (the weighted mean of 2^-24 w m) over every form, and |key_f32 - f64| / (2^-24 m) per pixel for the mined form's key map:
#   ties       means 0.000, per pixel 2.971 (K = 19)                                            -> 8
#   saturated  means 0.066 (weighted, K = 19, teacher logits on 9 x 17), per pixel 1.882         -> 4
#   nonfinite  means 0.000 (the call on the replaced logits)                                    -> 1
C_BOUND = {"ties": 8.0, "saturated": 4.0, "nonfinite": 1.0}


def _weights(K):
    return LR.CW6 if K == 6 else np.random.default_rng(K).choice([0.5, 1.0, 2.0, 4.0], K).tolist()


# form -> (entry, T, alpha, class weights?, gamma, reads teacher logits, gradient bar)
FORMS = {"hard": ("hard", 1.0, 0.0, False, 0.0, False, 2e-5), "soft": ("soft", 1.0, 1.0, False, 0.0, True, 3e-5),
         "kd-T2-a0.5": ("kd", 2.0, 0.5, False, 0.0, True, 3e-5), "kd-T0.5-a1": ("kd", 0.5, 1.0, False, 0.0, True, 3e-5),
         "weighted": ("weighted", 2.0, 0.5, True, 2.0, True, 3e-5), "two-pass": ("two-pass", 1.0, 0.0, False, 0.0, False, 2e-5)}

CASES = []
for _regime in ("ties", "saturated"):
    for _cls in (LG.SUB6, LG.SUB19):
        for _form, _f in FORMS.items():
            for _grid in (LG.LOSS_GRIDS if _f[5] else LG.LOSS_GRIDS[:1]):
                CASES.append((_regime, _form, 19, _cls, _grid))
    CASES.append((_regime, "kd-T2-a0.5", 21, LG.SUB21, LG.LOSS_GRIDS[1]))          # the 32 tier


def _id(c):
    return "%s-%s-K%d-t%dx%d" % (c[0], c[1], len(c[3]), c[4][0], c[4][1])


class _Ref:
    pass


_REFS = {}


def _reference(key, logits, teacher, tl, cls, T, alpha, cw, gamma, kept=None):
    """f64 autograd of loss_ref.objective on the f32-interpolated logits over the valid pixels (or over `kept`): computed once per key."""
    if key in _REFS:
        return _REFS[key]
    from oracle.student_torch import resize_bilinear_align_corners
    r = _Ref()
    K = len(cls)
    valid_np, y_np = LR.targets(teacher, cls)
    r.valid_all = valid_np
    if kept is not None:
        valid_np = kept
    z32 = Cf.interpolate_selected(logits, cls, H, W)
    z = torch.as_tensor(z32).double().requires_grad_(True)
    t = torch.as_tensor(SM.interpolate_teacher(tl, cls, H, W)).double() if tl is not None else None
    y, valid = torch.as_tensor(y_np), torch.as_tensor(valid_np)
    cwt = torch.as_tensor(np.asarray(cw if cw is not None else [1.0] * K, dtype=np.float64))
    loss, sum_w = LR.objective(z, t, y, valid, T, alpha, cwt, gamma)
    loss.backward()
    lt = torch.as_tensor(np.asarray(logits)).double().requires_grad_(True)
    resize_bilinear_align_corners(lt, H, W)[..., cls].backward(z.grad)
    r.loss, r.sum_w, r.d64, r.valid, r.y, r.z32 = float(loss.detach()), float(sum_w), lt.grad.numpy(), valid_np, y_np, z32
    zmag = np.abs(z32.astype(np.float64)).max(-1)
    m = alpha * T * T * (zmag / T + np.log(K)) + (1 - alpha) * (zmag + np.log(K))
    w64 = LR.pixel_weights(t, y, cwt, T, gamma).numpy()
    r.w64 = w64
    r.m = m
    r.scale = float((w64 * ULP * m)[valid_np].sum() / w64[valid_np].sum())      # the weighted mean of 2^-24 w m
    r.grid = float(GRID * valid_np.sum() / w64[valid_np].sum())                  # each pixel is rounded once, whatever its weight
    if gamma:
        r.sum_wq = float(LR.quantised(w64[valid_np]).sum())
        w32 = LR.weights_f32(t.numpy().astype(np.float32), y_np, cw, T, gamma)[valid_np]
        r.err32 = float(np.abs(LR.quantised(w32) - LR.quantised(w64[valid_np])).sum())
    _REFS[key] = r
    return r


def _two_pass(lib, logits, teacher, cls, NC):
    """ams_k_upsample_argmax (the loss pair) followed by ams_k_ce_grad: (loss pair, dlogits), on guarded buffers"""
    B, K = logits.shape[0], len(cls)
    ci = (C.c_int32 * K)(*cls)
    ld, td = dev(logits), dev(teacher, torch.uint8)
    conf, loss = out(K * K, torch.int64), out(2, torch.float64)
    run(lib.ams_k_upsample_argmax(P(ld), B, h, w, NC, ci, K, H, W, P(td), None, P(conf), P(loss), stream()), "ams_k_upsample_argmax")
    dl = out((B, h, w, NC))
    run(lib.ams_k_ce_grad(P(ld), B, h, w, NC, ci, K, H, W, P(td), P(loss), P(dl), stream()), "ams_k_ce_grad")
    return loss.cpu().numpy(), dl.cpu().numpy()


def _guarded_loss_call(lib, entry, logits, teacher, tl, cls, NC, T=1.0, alpha=1.0):
    """loss_ref.loss_call's "hard" and "kd" entries on guarded buffers with an exact, poisoned scratch"""
    B, K = logits.shape[0], len(cls)
    ci = (C.c_int32 * K)(*cls)
    n = lib.ams_k_ce_loss_grad_scratch(B, h, w, K)
    scr, loss, dl = scratch(n), out(2, torch.float64), out((B, h, w, NC))
    ld, td = dev(logits), dev(teacher, torch.uint8)
    if entry == "hard":
        rc = lib.ams_k_ce_loss_grad(P(ld), B, h, w, NC, ci, K, H, W, P(td), P(loss), P(dl), P(scr), n, stream())
    else:
        rc = lib.ams_k_ce_loss_grad_kd(P(ld), B, h, w, NC, NC, ci, K, H, W, P(td), P(dev(tl)), tl.shape[1], tl.shape[2], hip.TLOGITS_FULL, P(loss), P(dl),
                                       P(scr), n, stream(), C.c_float(T), C.c_float(alpha))
    run(rc, "ams_k_ce_loss_grad (%s)" % entry)
    return loss.cpu().numpy(), dl.cpu().numpy()


def _call(lib, form, logits, teacher, tl, cls, NC):
    entry, T, alpha, weighted, gamma, soft, _bar = FORMS[form]
    if entry == "two-pass":
        return _two_pass(lib, logits, teacher, cls, NC)
    return LR.loss_call(lib, entry, logits, teacher, tl if soft else None, cls, NC, H, W, T, alpha, _weights(len(cls)) if weighted else None, gamma)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def _quiet_cells(r, teacher, cls):
    """bool [B, h, w]: the cells every contributing valid pixel of which (a tap of whatever weight) is correct and whose contributing valid
    pixels' summed 1 - max softmax (f64) stays below 2^-25; the tap weights are at most 1, so sum_pixels weight |softmax_k - onehot_k| does."""
    z = r.z32.astype(np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    miss = 1.0 - p.max(-1)
    correct = LG.first_maximum(r.z32) == r.y
    quiet = np.zeros((z.shape[0], h, w), dtype=bool)
    for b in range(z.shape[0]):
        for i in range(h):
            for j in range(w):
                px = LG.footprint(h, w, H, W, i, j) & r.valid[b]
                quiet[b, i, j] = px.any() and correct[b][px].all() and miss[b][px].sum() <= 2.0 ** -25
    return quiet


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_loss_and_gradient(lib, case):
    """Loss pair within the absolute bound, weight sum as test_weighted_loss_and_gradient_kernel holds it, dlogits against f64 at the form's bar,
    unselected columns exactly 0, two runs identical.  Saturated, hard forms: a cell all of whose contributing valid pixels are correct, with
    their 1 - max softmax summing to at most 2^-25, has |d| <= 2^-24 / valid in every class (a stray 1 / N from a wrong one-hot index is
    2^24 times that)."""
    regime, form, NC, cls, grid = case
    entry, T, alpha, weighted, gamma, soft, bar = FORMS[form]
    logits, teacher, tl = LG.material(regime, LG.LOSS_SHAPE, NC, cls, grid)[:3]
    cw = _weights(len(cls)) if weighted else None
    r = _reference(("all",) + tuple(map(str, case)), logits, teacher, tl if soft else None, cls, T, alpha, cw, gamma)
    outs = [_call(lib, form, logits, teacher, tl, cls, NC) for _ in range(2)]
    got, d = outs[0]
    err = abs(got[0] / got[1] - r.loss)
    print("%s: loss %.9g (f64 %.9g), |difference| %.3e = grid + %.3f units of the scale %.3e; gradient err %.2e"
          % (_id(case), got[0] / got[1], r.loss, err, max(0.0, err - r.grid) / r.scale, r.scale, rel_err(d, r.d64)))
    if not gamma:
        assert got[1] == r.sum_w
    else:
        assert abs(got[1] - r.sum_wq) <= 4 * r.err32
    assert got[1] * LR.Q == np.rint(got[1] * LR.Q)
    assert err <= r.grid + C_BOUND[regime] * r.scale
    assert rel_err(d, r.d64) < bar
    unsel = [c for c in range(NC) if c not in cls]
    assert np.all(d[..., unsel] == 0)
    assert same(outs[0], outs[1])
    if regime == "saturated" and form in ("hard", "two-pass"):
        quiet = _quiet_cells(r, teacher, cls)
        assert quiet.sum() >= 4
        assert np.abs(d[quiet]).max() <= 2.0 ** -24 / got[1]


@pytest.mark.parametrize("cls", [LG.SUB6, LG.SUB19], ids=["K6", "K19"])
@pytest.mark.parametrize("regime", ["ties", "saturated"])
def test_mined_hard_form(lib, regime, cls):
    """ams_k_ce_loss_grad_mined, hard form at top_k = 0.25.  The key map is held per pixel to the f64 key by the absolute bound (in `saturated`
    half of the keys are exactly 0 in f32, far below the threshold).  The selection is exact on the kernel's OWN key map: the threshold is its
    k-th largest key, every key at or above it is kept, the counts and the mined label map say so.  Where the f64 keys have a relative gap of
    at least 5e-4 within 2 % of the rank (tests/test_gpu_loss_mining.py places the rank there: no f32 rounding closes it) the kept set is the
    f64 reference's exactly; the tied keys of six classes lie too dense for that (widest gap 1e-4 over a dozen seeds), there every pixel
    whose f64 key is further from the f64 threshold than twice the key bound is on its side.  Loss over the kept set within the bound,
    dlogits against f64, two runs identical."""
    NC, grid = 19, LG.LOSS_GRIDS[0]
    logits, teacher, _tl = LG.material(regime, LG.LOSS_SHAPE, NC, cls, grid)[:3]
    K = len(cls)
    valid, y = LR.targets(teacher, cls)
    z64 = Cf.interpolate_selected(logits, cls, H, W).astype(np.float64)
    zmax = z64.max(-1)
    key = np.maximum((zmax + np.log(np.exp(z64 - zmax[..., None]).sum(-1))) - np.take_along_axis(z64, y[..., None], -1)[..., 0], 0.0)
    n = int(valid.sum())
    k, gap, thr = gap_rank(key, valid, 0.25)
    gapped = gap >= MIN_GAP
    assert gapped or (regime, K) == ("ties", 6)
    if not gapped:
        k = mining_rank(0.25, n)
        thr = float(np.sort(key[valid])[::-1][k - 1])
    top_k = float(np.float32((k + 0.5) / n)) if gapped else 0.25
    assert mining_rank(top_k, n) == k
    outs = [mined_call(lib, logits, teacher, None, cls, NC, H, W, 1.0, 0.0, None, 0.0, top_k) for _ in range(2)]
    (got, d), labels, keys, res = outs[0]
    m = ULP * (np.abs(z64).max(-1) + np.log(K))
    per_pixel = float((np.abs(keys - key)[valid] / m[valid]).max())
    assert np.array_equal(keys < 0, ~valid)
    own = np.sort(keys[valid])[::-1][k - 1]
    kept = valid & (keys >= own)
    assert (res["valid"], res["rank"], res["kept"]) == (n, k, int(kept.sum())) and res["threshold"] == float(own)
    assert np.array_equal(labels, np.where(kept, teacher, 255).astype(np.uint8))
    r = _reference(("mined", regime, K), logits, teacher, None, cls, 1.0, 0.0, None, 0.0, kept=kept)
    err = abs(got[0] / got[1] - r.loss)
    print("mined-%s-K%d: n %d, k %d (gap %.2e), kept %d; keys: %d exactly 0, per pixel worst ratio %.3f; loss %.9g (f64 %.9g) = grid + %.3f units; gradient err %.2e"
          % (regime, K, n, k, gap, res["kept"], int((keys[valid] == 0).sum()), per_pixel, got[0] / got[1], r.loss, max(0.0, err - r.grid) / r.scale,
             rel_err(d, r.d64)))
    assert (np.abs(keys - key)[valid] <= C_BOUND[regime] * m[valid]).all()
    if gapped:
        assert np.array_equal(kept, valid & (key >= thr)) and res["kept"] == k
    else:
        tol = 2 * C_BOUND[regime] * float(m[valid].max())
        assert kept[valid & (key > thr + tol)].all() and not kept[valid & (key < thr - tol)].any() and res["kept"] >= k
    assert got[1] == res["kept"] and err <= r.grid + C_BOUND[regime] * r.scale
    assert rel_err(d, r.d64) < 3e-5
    assert np.all(d[..., [c for c in range(NC) if c not in cls]] == 0)
    assert same(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]


# ---------------------------------------------------------------------------------------------------- non-finite logits
# (route, subset, teacher grid): the hard routes read no teacher logits
NONFINITE = [(route, cls, grid) for route in ("hard", "two-pass", "kd") for cls in (LG.SUB6, LG.SUB19)
             for grid in (LG.LOSS_GRIDS if route == "kd" else LG.LOSS_GRIDS[:1])]


@pytest.mark.parametrize("route,cls,grid", NONFINITE, ids=["%s-K%d-t%dx%d" % (r, len(c), g[0], g[1]) for r, c, g in NONFINITE])
def test_nonfinite(lib, route, cls, grid):
    """A frame with NaN and infinite logits.  Teacher ignoring the affected pixels: the loss pair and the whole of dlogits are those of the call
    on the replaced logits, bit for bit (an ignored pixel contributes nothing, whatever its logits hold), and the loss is the f64 one within
    the bound.  Affected pixels valid: loss[1] still counts them, loss[0] is not finite, and dlogits equals the replaced call's bit for bit at
    every cell no affected pixel has a tap on, all of frame 1 among them; only such cells may hold a non-finite value; no guard is touched."""
    NC = 19
    logits, teacher, tl, affected, replaced = LG.material("nonfinite", LG.LOSS_SHAPE, NC, cls, grid)
    ignored = np.where(affected, 255, teacher).astype(np.uint8)
    yy, xx = np.indices((H, W))
    fill = np.asarray(cls, dtype=np.uint8)[(yy + xx) % len(cls)]
    valid = np.where(affected & ~np.isin(teacher, cls), fill[None], teacher).astype(np.uint8)
    T, alpha = (2.0, 0.5) if route == "kd" else (1.0, 0.0)

    def call(lg, tc):
        if route == "two-pass":
            return _two_pass(lib, lg, tc, cls, NC)
        return _guarded_loss_call(lib, route, lg, tc, tl, cls, NC, T, alpha)

    got_i, d_i = call(logits, ignored)
    got_r, d_r = call(replaced, ignored)
    assert np.array_equal(_bits(got_i), _bits(got_r)) and np.array_equal(_bits(d_i), _bits(d_r)) and np.isfinite(d_i).all()
    r = _reference(("nonfinite", route, len(cls), grid), replaced, ignored, tl if route == "kd" else None, cls, T, alpha, None, 0.0)
    err = abs(got_i[0] / got_i[1] - r.loss)
    print("nonfinite-%s-K%d: loss off by %.3e = grid + %.3f units; gradient err %.2e" % (route, len(cls), err, max(0.0, err - r.grid) / r.scale, rel_err(d_i, r.d64)))
    assert got_i[1] == r.sum_w and err <= r.grid + C_BOUND["nonfinite"] * r.scale and rel_err(d_i, r.d64) < (3e-5 if route == "kd" else 2e-5)
    got_v, d_v = call(logits, valid)
    got_rv, d_rv = call(replaced, valid)
    assert got_v[1] == got_rv[1] == LR.targets(valid, cls)[0].sum() and not np.isfinite(got_v[0]) and np.isfinite(got_rv).all()
    touched = LG.cells_of(h, w, H, W, affected)
    assert touched[0].any() and not touched[0].all() and not touched[1].any()
    assert np.array_equal(_bits(d_v[~touched]), _bits(d_rv[~touched]))
    assert np.isfinite(d_v[~touched]).all() and not np.isfinite(d_v[touched]).all()
