"""NumPy restatement of ``ams_teacher_labels_from_logits`` (include/ams_hip.h): label(Y, X) = argmax_c U(Y, X, c), where U is the
align-corners upsample of the cached teacher logits by the soft loss kernel's arithmetic, float32 operations one at a time (f32 scale, f32
product, f32 weights, bilerp's operation order, the cached sample itself on a grid point), and the argmax is tf.argmax's (the first maximum).
``src_taps`` / ``upsample`` are the only restatement of Stage U: the CPU and the GPU tests of the derived labels and the GPU tests of the
low-resolution logits gather share them; nothing here touches a device."""
import numpy as np


def src_taps(n_out, n_in):
    """src_tap of head_common.hpp for every position of an axis of n_out points over n_in cached ones: lo, hi, weight (f32)"""
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    assert scale.dtype == np.float32
    src = np.arange(n_out, dtype=np.float32) * scale
    fl = np.floor(src)
    t = src - fl
    assert src.dtype == np.float32 and t.dtype == np.float32
    lo = fl.astype(np.int64)
    return lo, np.minimum(lo + 1, n_in - 1), t


def upsample(t, Hs, Ws):
    """Stage U: ``t`` f32 [lh, lw, C] -> f32 [Hs, Ws, C]."""
    t = np.asarray(t, dtype=np.float32)
    ylo, yhi, ty = src_taps(Hs, t.shape[0])
    xlo, xhi, tx = src_taps(Ws, t.shape[1])
    tl, tr, bl, br = t[ylo][:, xlo], t[ylo][:, xhi], t[yhi][:, xlo], t[yhi][:, xhi]
    tx, ty = tx[None, :, None], ty[:, None, None]
    d = tr - tl
    d *= tx
    top = tl + d
    d = br - bl
    d *= tx
    bot = bl + d
    bot -= top
    bot *= ty
    v = top + bot
    assert v.dtype == np.float32
    return np.where((ty == 0) & (tx == 0), tl, v)                  # a grid point is the cached sample itself


def grid_points(Hs, Ws, lh, lw):
    """bool [Hs, Ws]: the positions of U that are cached samples (both weights zero), and the cached sample each position starts from."""
    ylo, _, ty = src_taps(Hs, lh)
    xlo, _, tx = src_taps(Ws, lw)
    return (ty == 0)[:, None] & (tx == 0)[None, :], ylo, xlo


def labels_from_logits(t, Hs, Ws):
    """uint8 [Hs, Ws]: the first maximum over every class of U (np.argmax returns the first of equal values; -0.0 == +0.0)."""
    t = np.asarray(t, dtype=np.float32)
    assert t.ndim == 3 and 1 <= t.shape[2] <= 255 and np.isfinite(t).all()
    return np.argmax(upsample(t, Hs, Ws), axis=-1).astype(np.uint8)
