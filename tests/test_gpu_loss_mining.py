"""Hard-pixel mining for the fine-tune loss (ams_k_ce_loss_grad_mined, ams_student_set_loss_mining): the step keeps the fraction top_k of the valid
pixels whose objective value

    key = max(0, w_q (alpha T^2 sum_k p_k (lse(z / T) - z_k / T) + (1 - alpha)(lse(z) - z_y)))

is largest, ties at the threshold all kept, and takes the loss of loss_ref.objective over those alone.  Kernel level against f64 with the kept set
exact (the rank is placed in a gap of the f64 keys that f32 cannot close), the relabel identity bit for bit, ties, edges, the student's step, and
the SemanticNetwork / scheduler surface."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

import loss_ref as LR
from ams_amd import exp_configs, hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine
from ams_amd.replay import draw_samples
from ams_amd.semantic_network import SemanticNetwork
from ams_amd.utils import mining_fraction, mining_rank
from loss_ref import CI, CW6, DEV, P, rel_err, same

pytestmark = pytest.mark.gpu

SHAPE0 = (5, 9, 64, 128, 19, CI, 64, 128)
CW_ZERO = [1.0, 0.0, 1.0, 4.0, 4.0, 2.0]
MIN_GAP = 5e-4


def _drawn_weights(K):
    return np.random.default_rng(K).choice([0.5, 1.0, 2.0, 4.0], K).tolist()


def mined_call(lib, logits, teacher, tl, cls, NC, H, W, T, alpha, cw, gamma, top_k, want_keys=True, layout=hip.TLOGITS_FULL):
    """One ams_k_ce_loss_grad_mined call on host arrays: ((loss pair, dlogits), mined labels, key map or None, result dict).  tl None = NULL
    teacher logits; the outputs start as NaN / 7 / -7 so that what the call leaves alone shows."""
    ld, td = torch.as_tensor(logits).to(DEV), torch.as_tensor(teacher).to(DEV)
    tld = torch.as_tensor(tl).to(DEV) if tl is not None else None
    th, tw = (tl.shape[1], tl.shape[2]) if tl is not None else (0, 0)
    B, h, w, _ = ld.shape
    K = len(cls)
    ci = (C.c_int32 * K)(*cls)
    n = lib.ams_k_ce_loss_grad_scratch(B, h, w, K)
    scr = torch.full((n,), np.nan, device=DEV)
    loss = torch.full((2,), np.nan, dtype=torch.float64, device=DEV)
    dl = torch.full((B, h, w, NC), np.nan, device=DEV)
    nm = lib.ams_k_loss_mining_scratch(B, H, W)
    mscr = torch.zeros(nm, dtype=torch.uint8, device=DEV)
    lab = torch.full((B, H, W), 7, dtype=torch.uint8, device=DEV)
    keys = torch.full((B, H, W), -7.0, device=DEV) if want_keys else None
    res = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    cwp = (C.c_float * K)(*[float(v) for v in cw]) if cw is not None else None
    hip.check(lib.ams_k_ce_loss_grad_mined(P(ld), B, h, w, NC, NC, ci, K, H, W, P(td), P(tld), th, tw, layout, P(loss), P(dl), P(scr), n, LR.stream(),
                                           C.c_float(T), C.c_float(alpha), cwp, C.c_float(gamma), C.c_float(top_k), P(lab), P(keys), P(res), P(mscr), nm))
    r = res.cpu().numpy()
    result = {"threshold": float(r[:1].view(np.float32)[0]), "valid": int(r[1]), "rank": int(r[2]), "kept": int(r[3])}
    return (loss.cpu().numpy(), dl.cpu().numpy()), lab.cpu().numpy(), keys.cpu().numpy() if want_keys else None, result


def keys64(logits, teacher, tl, cls, H, W, T, alpha, cw, gamma):
    """The f64 key map (NaN at a pixel that is not valid), and z, t, y for the loss over a kept set."""
    from oracle.student_torch import resize_bilinear_align_corners
    valid_np, y_np = LR.targets(teacher, cls)
    y = torch.as_tensor(y_np)
    lt = torch.as_tensor(logits).double().requires_grad_(True)
    z = resize_bilinear_align_corners(lt, H, W)[..., cls]
    t = None
    if tl is not None:
        t = torch.as_tensor(tl).double()
        if t.shape[1:3] != (H, W):
            t = resize_bilinear_align_corners(t, H, W)
        t = t[..., cls]
    cwt = torch.as_tensor(np.asarray(cw if cw is not None else [1.0] * len(cls), dtype=np.float64))
    with torch.no_grad():
        pixel = (1 - alpha) * (torch.logsumexp(z, -1) - torch.gather(z, -1, y.unsqueeze(-1)).squeeze(-1))
        if alpha:
            p = torch.softmax(t / T, -1)
            pixel = pixel + alpha * T * T * (p * (torch.logsumexp(z / T, -1, keepdim=True) - z / T)).sum(-1)
        wq = LR.quantised(LR.pixel_weights(t, y, cwt, T, gamma).numpy())
        valid_np = valid_np & (wq > 0)
        key = np.where(valid_np, np.maximum(wq * pixel.numpy(), 0.0), np.nan)
    return key, valid_np, (lt, z, t, y, cwt)


def gap_rank(key, valid, target):
    """The rank k within +-2 % of n around target n whose relative gap to the next f64 key is widest: (k, gap, threshold key).  The test's own
    precondition: a gap f32 keys cannot close, so that the kept set is a property of the inputs and not of a rounding."""
    ks = np.sort(key[valid])[::-1]
    n = ks.size
    lo, hi = max(1, int(np.floor((target - 0.02) * n))), min(n - 1, int(np.ceil((target + 0.02) * n)))
    cand = np.arange(lo, hi + 1)
    gaps = (ks[cand - 1] - ks[cand]) / ks[cand - 1]
    k = int(cand[np.argmax(gaps)])
    return k, float(gaps.max()), float(ks[k - 1])


def reference(logits, teacher, tl, cls, H, W, T, alpha, cw, gamma, target):
    key, valid, (lt, z, t, y, cwt) = keys64(logits, teacher, tl, cls, H, W, T, alpha, cw, gamma)
    n = int(valid.sum())
    k, gap, thr = gap_rank(key, valid, target)
    kept = valid & (key >= thr)
    loss, _ = LR.objective(z, t, y, torch.as_tensor(kept), T, alpha, cwt, gamma)
    loss.backward()
    return dict(key=key, valid=valid, n=n, k=k, gap=gap, kept=kept, labels=np.where(kept, teacher, 255).astype(np.uint8), loss=float(loss.detach()),
                d64=lt.grad.numpy(), top_k=float(np.float32((k + 0.5) / n)))


# (shape, form, T, alpha, cw, gamma, seed or None = the weighted-loss tests' own); form "hard" feeds no teacher logits
KERNEL_CASES = [
    (SHAPE0, "hard", 1.0, 0.0, None, 0.0, None),
    (SHAPE0, "soft", 1.0, 1.0, None, 0.0, None),
    (SHAPE0, "soft", 2.0, 0.5, CW6, 2.0, None),
    (SHAPE0, "soft", 2.0, 0.5, CW_ZERO, 0.0, None),
    (SHAPE0, "hard", 1.0, 0.0, CW_ZERO, 0.0, None),
    ((3, 5, 32, 64, 21, list(range(21)), 32, 64), "soft", 2.0, 0.5, _drawn_weights(21), 2.0, None),       # KMAX 32
    ((3, 5, 32, 64, 21, list(range(21)), 32, 64), "hard", 1.0, 0.0, None, 0.0, None),
    ((4, 7, 50, 90, 19, [0, 15], 13, 31), "soft", 2.0, 0.5, _drawn_weights(2), 2.0, None),               # odd sizes, a teacher off its grid points
    ((5, 9, 64, 128, 19, list(range(19)), 64, 128), "soft", 2.0, 0.5, _drawn_weights(19), 2.0, 20)]      # KMAX 20
# the hard form at KMAX 20: one frame (at 15 k pixels of 19 classes the hard keys' widest gaps are 4e-4, below the precondition)
HARD20 = ((5, 9, 64, 128, 19, list(range(19)), 64, 128), "hard", 1.0, 0.0, None, 0.0, 21)
_REFS = {}


def _case(shape, form, T, alpha, cw, gamma, seed, target, B=2):
    """The case's material and f64 reference, computed once and shared (nothing writes to either)."""
    key = (shape[:5] + (tuple(shape[5]),) + shape[6:], form, T, alpha, tuple(cw) if cw is not None else None, gamma, seed, target, B)
    if key not in _REFS:
        h, w, H, W, NC, cls, th, tw = shape
        logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th if seed is None else seed, B=B)
        feed = tl if form == "soft" else None
        _REFS[key] = (logits, teacher, feed, reference(logits, teacher, feed, cls, H, W, T, alpha, cw, gamma, target))
    return _REFS[key]


def _check_against_f64(shape, T, alpha, cw, gamma, logits, teacher, feed, ref):
    h, w, H, W, NC, cls, th, tw = shape
    lib = hip.lib()
    assert ref["gap"] >= MIN_GAP, "precondition on the inputs: widest relative gap %.2e in the window" % ref["gap"]
    assert mining_rank(ref["top_k"], ref["n"]) == ref["k"]
    outs = [mined_call(lib, logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma, ref["top_k"]) for _ in range(2)]
    (got, d), labels, keys, res = outs[0]
    v = ref["valid"]
    key_err = float(np.max(np.abs(keys[v] - ref["key"][v]) / np.maximum(ref["key"][v], 1e-30)))
    print("mined kernel (K=%d, T=%g, alpha=%g, gamma=%g, top_k=%.6f): n %d, k %d (gap %.2e), device valid %d rank %d kept %d threshold %.6f; "
          "key map max rel err %.2e; loss %.6f (f64 %.6f, rel %.2e), gradient err %.2e"
          % (len(cls), T, alpha, gamma, ref["top_k"], ref["n"], ref["k"], ref["gap"], res["valid"], res["rank"], res["kept"], res["threshold"], key_err,
             got[0] / got[1], ref["loss"], abs(got[0] / got[1] - ref["loss"]) / abs(ref["loss"]), rel_err(d, ref["d64"])))
    assert res["valid"] == ref["n"] and res["rank"] == ref["k"] and res["kept"] == ref["k"]
    assert np.array_equal(keys < 0, ~v)                              # the sentinel exactly at the pixels that are not valid
    assert np.array_equal(labels, ref["labels"])
    assert got[0] / got[1] == pytest.approx(ref["loss"], rel=2e-5)
    assert rel_err(d, ref["d64"]) < 3e-5
    unsel = [c for c in range(NC) if c not in cls]
    assert np.all(d[..., unsel] == 0)
    assert same(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2]) and outs[0][3] == outs[1][3]
    return outs[0]


@pytest.mark.parametrize("target", [0.25, 0.5])
@pytest.mark.parametrize("shape,form,T,alpha,cw,gamma,seed", KERNEL_CASES)
def test_mined_kernel_against_f64_with_the_kept_set_exact(shape, form, T, alpha, cw, gamma, seed, target):
    """The kept set, the three counts and the mined label map equal the f64 reference's exactly, given a rank placed in a relative gap of the f64
    keys of at least 5e-4; mean loss rel 2e-5 and gradient error 3e-5 against f64 autograd of the objective over the kept set (the bars of
    test_weighted_loss_and_gradient_kernel), unselected columns exactly 0, two runs identical.  The key map's largest relative error against f64
    is printed: a measurement, the bar is the kept set."""
    logits, teacher, feed, ref = _case(shape, form, T, alpha, cw, gamma, seed, target)
    _check_against_f64(shape, T, alpha, cw, gamma, logits, teacher, feed, ref)


@pytest.mark.parametrize("target", [0.25, 0.5])
def test_mined_kernel_hard_form_of_the_20_class_tier(target):
    shape, form, T, alpha, cw, gamma, seed = HARD20
    logits, teacher, feed, ref = _case(shape, form, T, alpha, cw, gamma, seed, target, B=1)
    _check_against_f64(shape, T, alpha, cw, gamma, logits, teacher, feed, ref)


@pytest.mark.parametrize("shape,form,T,alpha,cw,gamma,seed", KERNEL_CASES)
def test_relabel_identity_bit_for_bit(shape, form, T, alpha, cw, gamma, seed):
    """The mined call is ams_k_ce_loss_grad_weighted on the label map it returns, in loss pair and dlogits; without a key output too; top_k = 1
    is the unmined entry with labels_out a copy of the input, the key map and the result block untouched."""
    h, w, H, W, NC, cls, th, tw = shape
    lib = hip.lib()
    logits, teacher, feed, ref = _case(shape, form, T, alpha, cw, gamma, seed, 0.25)
    out, labels, _keys, res = mined_call(lib, logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma, ref["top_k"])
    plain = LR.loss_call(lib, "weighted", logits, labels, feed, cls, NC, H, W, T, alpha, cw, gamma)
    assert same(out, plain)
    assert 0 < res["kept"] < res["valid"] and int((labels != 255).sum()) == res["kept"] and np.array_equal(labels[labels != 255], teacher[labels != 255])
    nokeys = mined_call(lib, logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma, ref["top_k"], want_keys=False)
    assert same(nokeys[0], out) and np.array_equal(nokeys[1], labels) and nokeys[3] == res
    off, labels1, keys1, res1 = mined_call(lib, logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma, 1.0)
    assert same(off, LR.loss_call(lib, "weighted", logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma))
    assert np.array_equal(labels1, teacher) and np.all(keys1 == -7.0) and res1["valid"] == res1["rank"] == res1["kept"] == -7
    assert not same(off, out)


def test_selected_layout_is_the_full_one():
    shape, form, T, alpha, cw, gamma, seed = KERNEL_CASES[2]
    h, w, H, W, NC, cls, th, tw = shape
    logits, teacher, feed, ref = _case(shape, form, T, alpha, cw, gamma, seed, 0.25)
    full = mined_call(hip.lib(), logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma, ref["top_k"])
    sel = np.ascontiguousarray(np.take(feed, cls, axis=-1))
    got = mined_call(hip.lib(), logits, teacher, sel, cls, NC, H, W, T, alpha, cw, gamma, ref["top_k"], layout=hip.TLOGITS_SELECTED)
    assert same(got[0], full[0]) and np.array_equal(got[1], full[1]) and np.array_equal(got[2], full[2]) and got[3] == full[3]


def test_ties_at_the_threshold_are_all_kept():
    """Logits identical in every low-resolution cell: the interpolation returns them exactly and the hard key takes K distinct values, one per
    label class.  With the rank inside the second-hardest class, the threshold is that class's key and kept is the label histogram's count of the
    two hardest classes: exact, and greater than k."""
    h, w, H, W, NC, cls, th, tw = SHAPE0
    rng = np.random.default_rng(3)
    row = (rng.standard_normal(NC) * 2).astype(np.float32)
    logits = np.broadcast_to(row, (2, h, w, NC)).copy()
    teacher = rng.integers(0, NC, (2, H, W)).astype(np.uint8)
    teacher[rng.random((2, H, W)) < 0.1] = 255
    sel = row[cls].astype(np.float64)
    key_of = np.log(np.exp(sel - sel.max()).sum()) + sel.max() - sel               # lse - z_y per label class
    order = np.argsort(-key_of)
    counts = np.array([(teacher == c).sum() for c in cls])
    n = int(counts.sum())
    k = int(counts[order[0]] + counts[order[1]] // 2)
    top_k = float(np.float32((k + 0.5) / n))
    assert mining_rank(top_k, n) == k
    out, labels, keys, res = mined_call(hip.lib(), logits, teacher, None, cls, NC, H, W, 1.0, 0.0, None, 0.0, top_k)
    class_keys = [np.unique(keys[teacher == c]) for c in cls]
    assert all(u.size == 1 for u in class_keys) and len({float(u[0]) for u in class_keys}) == len(cls)
    assert res["valid"] == n and res["rank"] == k
    assert res["kept"] == counts[order[0]] + counts[order[1]] > k
    assert res["threshold"] == float(class_keys[order[1]][0])
    assert np.array_equal(labels, np.where(np.isin(teacher, [cls[order[0]], cls[order[1]]]), teacher, 255))
    assert out[0][1] == res["kept"]


def test_edges():
    """One valid pixel: k = kept = 1.  No valid pixel: valid = kept = 0, NaN loss, an all-zero gradient, as the unmined kernel.  A top_k so small
    that k = 1: the one hardest pixel.  B = 1 and B = 3 against f64."""
    lib = hip.lib()
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    one = np.full_like(teacher, 255)
    one[1, 37, 71] = cls[4]
    out, labels, keys, res = mined_call(lib, logits, one, tl, cls, NC, H, W, 2.0, 0.5, CW6, 2.0, 0.25)
    assert (res["valid"], res["rank"], res["kept"]) == (1, 1, 1) and np.array_equal(labels, one) and res["threshold"] == keys[1, 37, 71] > 0
    assert same(out, LR.loss_call(lib, "weighted", logits, one, tl, cls, NC, H, W, 2.0, 0.5, CW6, 2.0))
    none = np.full_like(teacher, 255)
    none[0, :8] = 3                                                   # a class outside the subset
    out, labels, keys, res = mined_call(lib, logits, none, None, cls, NC, H, W, 1.0, 0.0, None, 0.0, 0.25)
    assert res["valid"] == 0 and res["kept"] == 0 and np.all(labels == 255) and np.all(keys == -1.0)
    with np.errstate(invalid="ignore"):
        assert out[0][1] == 0 and np.isnan(out[0][0] / out[0][1])
    assert np.all(out[1] == 0)
    key, valid, _ = keys64(logits, teacher, None, cls, H, W, 1.0, 0.0, None, 0.0)
    n = int(valid.sum())
    ks = np.sort(key[valid])[::-1]
    assert (ks[0] - ks[1]) / ks[0] > 1e-5                              # the hardest pixel is alone at the top, beyond f32 rounding
    out, labels, keys, res = mined_call(lib, logits, teacher, None, cls, NC, H, W, 1.0, 0.0, None, 0.0, 0.5 / n)
    assert (res["valid"], res["rank"], res["kept"]) == (n, 1, 1) and mining_rank(0.5 / n, n) == 1
    assert np.array_equal(labels != 255, key == ks[0]) and out[0][1] == 1
    for B in (1, 3):
        a = (SHAPE0, "soft", 2.0, 0.5, CW6, 2.0, 40 + B, 0.25)
        lg, tc, feed, ref = _case(*a, B=B)
        assert lg.shape[0] == B
        _check_against_f64(SHAPE0, 2.0, 0.5, CW6, 2.0, lg, tc, feed, ref)


# ---------------------------------------------------------------------------------------------------------
# one fine-tune step
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


def _engine(W0, H, B, soft):
    eng = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W0)
    if soft:
        eng.set_soft_teacher(True)
        eng.set_kd(2.0, 0.5)
        eng.set_loss_weights(CW6, 2.0)
    return eng


def _same_state(a, b):
    va, vb = a.get_variables(), b.get_variables()
    return sorted(va) == sorted(vb) and all(np.array_equal(va[k], vb[k]) for k in va) and torch.equal(a.adam_m, b.adam_m) and \
        torch.equal(a.adam_v, b.adam_v) and torch.equal(a.grads, b.grads)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft_teacher"])
def test_mined_step_is_the_plain_step_on_the_mined_labels(W0, soft):
    """64 x 128, B = 2.  set_loss_mining(1.0): loss, gradients and parameters after a step are those of a student that never called it, bit for
    bit.  top_k = 0.25: the step's loss pair and every parameter equal, bit for bit, an unmined twin's stepping on the label map the first one
    reports, and kept >= rank == mining_rank(0.25, valid).  A data-parallel callback step with top_k < 1 is refused in words, nothing launched."""
    H, B, lr = 64, 2, 1e-3
    frames, labels = synth.SyntheticVideo(H, B, CI, seed=5).clip()
    kw = dict(teacher_logits=LR.teacher_logits(labels.astype(np.int64), np.random.default_rng(17), th=9, tw=17)) if soft else {}
    never, off, mined, twin = (_engine(W0, H, B, soft) for _ in range(4))
    off.set_loss_mining(0.5)                                           # allocates the scratch ...
    off.set_loss_mining(1.0)                                           # ... and switches it off again
    ls_never = never.train_step(frames, labels, lr, **kw).cpu().numpy()
    ls_off = off.train_step(frames, labels, lr, **kw).cpu().numpy()
    assert np.array_equal(ls_never, ls_off) and _same_state(never, off)
    with pytest.raises(RuntimeError, match="no mined step"):
        off.mining_result()
    mined.set_loss_mining(0.25)
    ls_m = mined.train_step(frames, labels, lr, **kw).cpu().numpy()
    res = mined.mining_result()
    map_m = mined.mined_labels(B).cpu().numpy()
    print("mined step (%s): loss %.6f over %g kept of %d valid (rank %d, threshold %.6f); unmined loss %.6f"
          % ("soft" if soft else "hard", ls_m[0] / ls_m[1], ls_m[1], res["valid"], res["rank"], res["threshold"], ls_never[0] / ls_never[1]))
    assert res["kept"] >= res["rank"] == mining_rank(0.25, res["valid"]) and res["valid"] > 4
    assert int((map_m != 255).sum()) == res["kept"] and np.array_equal(map_m[map_m != 255], labels[map_m != 255])
    if not soft:
        assert ls_m[1] == res["kept"] and res["valid"] == int(np.isin(labels, CI).sum())
        assert ls_m[0] / ls_m[1] > ls_never[0] / ls_never[1]           # the plain mean over the hardest pixels
    ls_t = twin.train_step(frames, map_m, lr, **kw).cpu().numpy()
    assert np.array_equal(ls_m, ls_t) and _same_state(mined, twin)
    # refusals: in words, the student keeping what it had, nothing launched
    before = mined.get_variables()
    for bad in (0.0, -0.25, 1.5, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="top_k"):
            mined.set_loss_mining(bad)
    assert mined.loss_top_k == 0.25
    with pytest.raises(RuntimeError, match="all-reduce"):
        mined.train_step(frames, labels, lr, allreduce=lambda t: None, **kw)
    after = mined.get_variables()
    assert all(np.array_equal(before[k], after[k]) for k in before) and mined.adam_step == 1
    for e in (never, off, mined, twin):
        e.close()


def test_student_entry_refusals(W0):
    """ams_student_set_loss_mining: a frozen student, a scratch that is NULL, misaligned or too small are refused in words and the student keeps
    what it had; top_k = 1 with NULL scratch is accepted and switches mining off."""
    H, B = 64, 2
    frozen = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=False)
    with pytest.raises(RuntimeError, match="frozen"):
        frozen.set_loss_mining(0.25)
    frozen.close()
    eng = _engine(W0, H, B, False)
    lib, need = eng.lib, eng.lib.ams_k_loss_mining_scratch(B, H, 2 * H)
    scr = torch.zeros(need + 16, dtype=torch.uint8, device=DEV)
    for ptr, size in ((0, need), (scr.data_ptr() + 8, need), (scr.data_ptr(), need - 1)):
        assert lib.ams_student_set_loss_mining(eng._h, 0.25, C.c_void_p(ptr), size) == -1
        assert b"scratch" in lib.ams_last_error()
    frames, labels = synth.SyntheticVideo(H, B, CI, seed=5).clip()
    plain = eng.train_step(frames, labels, 1e-3).cpu().numpy()         # still unmined: the count is every valid pixel
    assert plain[1] == int(np.isin(labels, CI).sum())
    hip.check(lib.ams_student_set_loss_mining(eng._h, 0.25, C.c_void_p(scr.data_ptr()), need))
    hip.check(lib.ams_student_set_loss_mining(eng._h, 1.0, None, 0))
    assert eng.train_step(frames, labels, 1e-3).cpu().numpy()[1] == plain[1]
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# SemanticNetwork on a DeviceReplayMemory, the scheduler
# ---------------------------------------------------------------------------------------------------------
H, BATCH, ITERS, SLOTS, SEED, GRID = 64, 2, 3, 4, 3, (9, 17)


def test_semantic_network_mined_phase_equals_hand_made_steps(W0):
    """SemanticNetwork(soft_teacher=True, loss_top_k=0.25, loss_top_k_warmup=2) for three iterations on a replay memory, against three engine steps
    at the fractions 1.0, 0.625 and 0.25 on the same draws: every variable and last_losses equal bit for bit, last_mining is the last step's block."""
    assert [mining_fraction(0.25, 2, it) for it in range(ITERS)] == [1.0, 0.625, 0.25]
    mem, frames, labels, logits = LR.memory(np.random.default_rng(12), H, SLOTS, GRID)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=BATCH, lr=1e-3,
                          initial_variables=W0, soft_teacher=True, loss_top_k=0.25, loss_top_k_warmup=2)
    LR.seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    assert len(net.last_losses) == ITERS and all(np.isfinite(net.last_losses))
    LR.seed(SEED)
    desc = draw_samples(len(mem), (H, 2 * H), [H, 2 * H], [1], BATCH, ITERS, flip=False)
    eng = StudentEngine(net.class_indices_graph.tolist(), H, 2 * H, max_batch=BATCH, trainable=True)
    eng.load_variables(W0)
    eng.set_soft_teacher(True)
    want = []
    for it, frac in enumerate((1.0, 0.625, 0.25)):
        picks = desc[it][:, 0]
        eng.set_loss_mining(frac)
        ls = eng.train_step(frames[picks], labels[picks], 1e-3, teacher_logits=logits[picks]).cpu().numpy()
        want.append(float(ls[0] / ls[1]))
    assert [float(x) for x in net.last_losses] == want
    assert net.last_mining == eng.mining_result() and net.last_mining["rank"] == mining_rank(0.25, net.last_mining["valid"])
    a, b = net.get_vars(), eng.get_variables()
    assert all(np.array_equal(a[k], b[k]) for k in b), [k for k in b if not np.array_equal(a[k], b[k])][:5]
    assert torch.equal(net.engine.adam_m, eng.adam_m) and torch.equal(net.engine.adam_v, eng.adam_v)
    assert net.engine.loss_top_k == 1.0                                # a phase leaves the engine unmined
    net.close_model()
    eng.close()


def test_scheduler_writes_one_mining_row_per_training_event(tmp_path):
    """python -m ams_amd.run --device_memory --loss_top_k 0.25 on the seeded 8-second clip (height 32): <results>_mining.npy holds one finite row
    (threshold, kept, valid) per training event with kept >= mining_rank(0.25, valid), and the other files have the names of a run without it."""
    from ams_amd import run as R
    out = {}
    for tag, extra in (("plain", []), ("mined", ["--loss_top_k", "0.25"])):
        out[tag] = str(tmp_path / tag) + "/"
        os.makedirs(out[tag])
        LR.seed(1)
        summary = R.main(["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", out[tag],
                          "--gpu", "0", "--mode", "simple", "--height", "32", "--batch_size", "2", "--iter", "1", "--send_period", "2",
                          "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--device_memory"] + extra)
        assert summary["frames"] == 16
    names = {tag: sorted(os.path.basename(p) for p in glob.glob(o + "*")) for tag, o in out.items()}
    assert not any(n.endswith("_mining.npy") for n in names["plain"])
    assert [n for n in names["mined"] if not n.endswith("_mining.npy")] == names["plain"]
    hits = glob.glob(out["mined"] + "*_mining.npy")
    assert len(hits) == 1
    rows = np.load(hits[0])
    events = np.load(glob.glob(out["mined"] + "*_train_ms.npy")[0])
    assert rows.shape == (len(events), 3) and len(events) >= 2 and np.isfinite(rows).all()
    assert all(kept >= mining_rank(0.25, valid) >= 1 and valid >= kept for _thr, kept, valid in rows)
