"""What the tests of the fine-tune loss share (test_gpu_soft_teacher, test_gpu_kd_loss, test_gpu_weighted_loss, test_kd_cpu, test_weighted_loss_cpu):
the kernel cases' material, the objective

    pixel = alpha T^2 sum_k softmax(t / T)_k (logsumexp(z / T) - z_k / T) + (1 - alpha) (logsumexp(z) - z_y)
    w = cw_y (max_k softmax(t / T)_k)^gamma,    loss = sum_valid w pixel / sum_valid w

written out in torch (any dtype) and restated in f32 NumPy for the weight alone, one ctypes call of whichever kernel-level entry a test is about,
the oracle's gradients under the objective, and the replay memory of the SemanticNetwork tests."""
import ctypes as C
import random
import re
from pathlib import Path

import numpy as np
import torch

from ams_amd import hip

DEV = "cuda:0"
CI = [0, 1, 2, 10, 11, 13]
CW6 = [1.0, 1.0, 1.0, 4.0, 4.0, 2.0]
Q = 1048576.0


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)


def teacher_logits(labels, rng, nc=19, th=None, tw=None, sharp=3.0):
    """Synthetic cached teacher logits: noise + a bump on the class of the label map (what a teacher whose argmax gave those labels looks like),
    optionally sampled down to th x tw."""
    B, H, W = labels.shape
    t = rng.standard_normal((B, H, W, nc)).astype(np.float32)
    ok = labels < nc
    bi, yi, xi = np.nonzero(ok)
    t[bi, yi, xi, labels[ok]] += sharp
    if th is not None:
        ys = np.round(np.linspace(0, H - 1, th)).astype(int)
        xs = np.round(np.linspace(0, W - 1, tw)).astype(int)
        t = np.ascontiguousarray(t[:, ys][:, :, xs])
    return t


def material(h, w, H, W, NC, th, tw, seed, B=2):
    """Student logits ~ 2 N(0, 1), labels with 10 % ignored, teacher logits = noise + a bump of 3."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, h, w, NC)) * 2).astype(np.float32)
    teacher = rng.integers(0, NC, (B, H, W)).astype(np.uint8)
    teacher[rng.random((B, H, W)) < 0.1] = 255
    tl = teacher_logits(np.where(teacher < NC, teacher, 0).astype(np.int64), rng, nc=NC, th=th if (th, tw) != (H, W) else None, tw=tw)
    assert tl.shape == (B, th, tw, NC)
    return logits, teacher, tl


def targets(teacher, cls):
    """(valid, index in the subset or 0) per label."""
    lut = np.full(256, -1)
    lut[cls] = np.arange(len(cls))
    return lut[teacher] >= 0, np.where(lut[teacher] >= 0, lut[teacher], 0).astype(np.int64)


def pixel_weights(t, y, cw, T, gamma):
    """w = cw_y c^gamma per pixel; t [..., K] or None (gamma = 0 then), y int64 [...], cw tensor [K]."""
    w = cw[y]
    if gamma:
        w = w * torch.softmax(t.detach() / T, -1).max(-1).values ** gamma
    return w


def objective(z, t, y, valid, T=1.0, alpha=1.0, cw=None, gamma=0.0):
    """(loss, sum of the weights): z [..., K], t [..., K] (no gradient) or None for the hard form (alpha = 0, gamma = 0), y int64 [...], valid
    bool [...], cw tensor [K] or None = ones."""
    hard = torch.logsumexp(z, -1) - torch.gather(z, -1, y.unsqueeze(-1)).squeeze(-1)
    pixel = (1 - alpha) * hard
    if alpha:
        p = torch.softmax(t.detach() / T, -1)
        pixel = pixel + alpha * T * T * (p * (torch.logsumexp(z / T, -1, keepdim=True) - z / T)).sum(-1)
    if cw is None:
        cw = torch.ones(z.shape[-1], dtype=z.dtype)
    w = torch.where(valid, pixel_weights(t, y, cw, T, gamma), torch.zeros((), dtype=z.dtype))
    return (w * pixel).sum() / w.sum(), w.sum()


def quantised(w):
    return np.rint(np.asarray(w, dtype=np.float64) * Q) / Q


def weights_f32(t, y, cw, T, gamma):
    """The weight as an f32 program forms it: c^gamma = exp(-gamma log sum_k exp((t_k - max) / T)), every step rounded to f32."""
    t = np.asarray(t, dtype=np.float32)
    w = np.asarray(cw, dtype=np.float32)[y]
    if gamma:
        e = np.exp((t - t.max(-1, keepdims=True)) * np.float32(1.0 / T), dtype=np.float32)
        w = w * np.exp(-np.float32(gamma) * np.log(e.sum(-1, dtype=np.float32), dtype=np.float32), dtype=np.float32)
    return w.astype(np.float32)


def loss_call(lib, entry, logits, teacher, tl, cls, NC, H, W, T=1.0, alpha=1.0, cw=None, gamma=0.0, layout=hip.TLOGITS_FULL):
    """One call of ams_k_ce_loss_grad ("hard"), _soft, _kd or _weighted on host arrays or device tensors: (loss pair, dlogits) as NumPy.  Each
    entry is given what its prototype takes and nothing else; tl None = NULL teacher logits."""
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
    out = (P(loss), P(dl), P(scr), n, stream())
    if entry == "hard":
        hip.check(lib.ams_k_ce_loss_grad(P(ld), B, h, w, NC, ci, K, H, W, P(td), *out))
    elif entry == "soft":
        hip.check(lib.ams_k_ce_loss_grad_soft(P(ld), B, h, w, NC, ci, K, H, W, P(td), P(tld), th, tw, *out))
    elif entry == "kd":
        hip.check(lib.ams_k_ce_loss_grad_kd(P(ld), B, h, w, NC, NC, ci, K, H, W, P(td), P(tld), th, tw, layout, *out, C.c_float(T), C.c_float(alpha)))
    else:
        assert entry == "weighted", entry
        cwp = (C.c_float * K)(*[float(v) for v in cw]) if cw is not None else None
        hip.check(lib.ams_k_ce_loss_grad_weighted(P(ld), B, h, w, NC, NC, ci, K, H, W, P(td), P(tld), th, tw, layout, *out, C.c_float(T), C.c_float(alpha),
                                                  cwp, C.c_float(gamma)))
    return loss.cpu().numpy(), dl.cpu().numpy()


def oracle_gradients(o, frames, labels, tl, T, alpha, cw=None, gamma=0.0):
    """(loss, sum of the weights, gradients) of the objective on the oracle's own network (StudentOracle.logits_full in training mode), by autograd."""
    from oracle.student_torch import resize_bilinear_align_corners
    params, leaves = dict(o.vars), {}
    for v in o.spec.trainable:
        leaves[v.name] = params[v.name] = o.vars[v.name].clone().requires_grad_(True)
    z = o.reduced_logits(o.logits_full(frames, "train", params))
    y, weight = o.label_targets(labels)
    t = torch.as_tensor(tl).to(o.dtype)
    if t.shape[1:3] != z.shape[1:3]:
        t = resize_bilinear_align_corners(t, z.shape[1], z.shape[2])
    loss, sum_w = objective(z, o.reduced_logits(t), y, weight > 0, T, alpha, None if cw is None else torch.as_tensor(np.asarray(cw)).to(o.dtype), gamma)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return float(loss.detach()), float(sum_w.detach()), dict(zip(leaves, grads))


def seed(value):
    np.random.seed(value)
    random.seed(value)


def memory(rng, H, slots, grid):
    """A DeviceReplayMemory of `slots` random H x 2H frames with blocky labels and teacher logits on `grid` (noise + a bump of 3 on the label's class):
    (memory, frames, labels, logits), the last three stacked."""
    from ams_amd.replay import DeviceReplayMemory
    src = (H, 2 * H)
    frames = [rng.integers(0, 256, src + (3,), dtype=np.uint8) for _ in range(slots)]
    labels = [np.repeat(np.repeat(rng.integers(0, 19, (H // 8, 2 * H // 8), dtype=np.uint8), 8, axis=0), 8, axis=1) for _ in range(slots)]
    ys = np.rint(np.linspace(0, src[0] - 1, grid[0])).astype(np.int64)
    xs = np.rint(np.linspace(0, src[1] - 1, grid[1])).astype(np.int64)
    logits = []
    for l in labels:
        t = rng.standard_normal(grid + (19,)).astype(np.float32)
        cls = l[ys][:, xs][..., None].astype(np.int64)
        np.put_along_axis(t, cls, np.take_along_axis(t, cls, 2) + 3.0, axis=2)
        logits.append(t)
    mem = DeviceReplayMemory(slots, src[0], src[1], DEV, logits_shape=grid + (19,))
    for f, l, t in zip(frames, labels, logits):
        mem.append(f, l, t)
    return mem, np.stack(frames), np.stack(labels), np.stack(logits)


C_TYPES = {"float": C.c_float, "int32_t": C.c_int32, "size_t": C.c_size_t, "int": C.c_int}


def header_prototype(name):
    """(restype, argtypes) of a function of include/ams_hip.h as the binding spells them: the class list is int32 *, a weight table float *, any
    other pointer void *."""
    text = re.sub(r"/\*.*?\*/", "", (Path(__file__).resolve().parent.parent / "include" / "ams_hip.h").read_text(), flags=re.S)
    ret, args = re.search(r"\b(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text).groups()
    out = []
    for a in args.split(","):
        a = a.strip()
        flat = a.replace(" ", "")
        if flat.startswith("constint32_t*"):
            out.append(C.POINTER(C.c_int32))
        elif flat.startswith("constfloat*class_weights_host"):
            out.append(C.POINTER(C.c_float))
        elif "*" in a:
            out.append(C.c_void_p)
        else:
            out.append(C_TYPES[a.split()[-2]])
    return C_TYPES[ret], out
