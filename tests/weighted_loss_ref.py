"""What tests/test_weighted_loss_cpu.py and tests/test_gpu_weighted_loss.py share: the kernel cases' material and the weighted objective

    w = cw_y (max_k softmax(t / T)_k)^gamma,    loss = sum_valid w pixel / sum_valid w

written out in torch (any dtype) and restated in f32 NumPy for the weight alone."""
import numpy as np
import torch

CI = [0, 1, 2, 10, 11, 13]
CW6 = [1.0, 1.0, 1.0, 4.0, 4.0, 2.0]
Q = 1048576.0


def teacher_logits(labels, rng, nc=19, th=None, tw=None, sharp=3.0):
    """tests/test_gpu_kd_loss.py's: noise + a bump of 3 on the class of the label map, optionally sampled down to th x tw."""
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


def pixel_weights(t, y, cw, T, gamma):
    """w = cw_y c^gamma per pixel; t [..., K] or None (gamma = 0 then), y int64 [...], cw tensor [K]."""
    w = cw[y]
    if gamma:
        w = w * torch.softmax(t.detach() / T, -1).max(-1).values ** gamma
    return w


def weighted_objective(z, t, y, valid, T, alpha, cw, gamma):
    """(loss, sum of the weights): z [..., K], t [..., K] or None for the hard form (alpha = 0, gamma = 0), valid bool [...]."""
    hard = torch.logsumexp(z, -1) - torch.gather(z, -1, y.unsqueeze(-1)).squeeze(-1)
    pixel = (1 - alpha) * hard
    if alpha:
        p = torch.softmax(t.detach() / T, -1)
        pixel = pixel + alpha * T * T * (p * (torch.logsumexp(z / T, -1, keepdim=True) - z / T)).sum(-1)
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
