"""Logit regimes the head's read-out and loss kernels make promises for and the 2 N(0, 1) material of the other suites never reaches: exact
ties, saturated softmaxes, non-finite values.  Pure NumPy, no device: tests/test_logit_regimes_cpu.py asserts on the f32 restatement of the
interpolation (ams_amd.confidence.interpolate_selected) that every regime is what it says at every shape the GPU tests
(test_gpu_head_regimes.py, test_gpu_loss_regimes.py) run, and those hold the kernels to the rule below.

Every generator returns (logits f32 [B,h,w,NC], teacher u8 [B,H,W], teacher_logits f32 [B,th,tw,NC]) for a class subset `cls`,
deterministic from `seed`; `nonfinite` adds what its tests need.

The rule (include/ams_hip.h, ams_k_upsample_argmax): the label of a pixel is a strict `>` scan from class 0 in subset order over the K
interpolated values, `first_maximum`.  Ties and -0.0 / +0.0 take the lower index; a NaN wins only in class 0."""
import numpy as np

from ams_amd.confidence import _taps, interpolate_selected

F32 = np.float32
MARGINS = (40.0, 90.0, 200.0)
NONFINITE_GRID = (5, 9)
# (cell row, cell column, position in the subset, value) of the four cells `nonfinite` spoils in frame 0
NONFINITE_CELLS = ((1, 1, 2, np.nan), (1, 5, 0, np.nan), (3, 2, 1, np.inf), (3, 6, 3, -np.inf))


def first_maximum(z):
    """[..., K] -> int64 [...]: arg = 0; for k in 1 .. K - 1: if z[k] > z[arg]: arg = k.  np.argmax on finite input; on NaN the kernels'
    rule and not NumPy's (there a NaN wins wherever it stands)."""
    z = np.asarray(z)
    arg = np.zeros(z.shape[:-1], dtype=np.int64)
    best = z[..., 0].copy()
    for k in range(1, z.shape[-1]):
        m = z[..., k] > best
        arg[m] = k
        best = np.where(m, z[..., k], best)
    return arg


def last_maximum(z):
    """the highest index that holds the maximum (finite input): the other end of a tie"""
    z = np.asarray(z)
    K = z.shape[-1]
    return K - 1 - np.argmax(z[..., ::-1], axis=-1)


def tied(z):
    """bool [...]: the maximum is held by more than one class, exactly"""
    z = np.asarray(z)
    return (z == z.max(-1, keepdims=True)).sum(-1) > 1


def stripes(w):
    """the cell columns' stripe (0, 1, 2): thirds of the grid, the left ones wider"""
    return np.minimum(np.arange(w) * 3 // w, 2)


def _ignore(rng, teacher, share=0.1):
    teacher[rng.random(teacher.shape) < share] = 255
    return teacher


def _tied_grid(rng, B, h, w, NC, cls, bump):
    """Noise N(0, 1) with tied channels.  s = subset order; the cell columns fall into three stripes.
    Even frames: s1 is a bitwise copy of s0 and s3, s4 are copies of s2 in EVERY cell, so each group ties at every pixel whatever the taps and
    weights; a bump on (s0, s1) in stripe 0, on (s2, s3, s4) in stripe 1 and on (s2, s3) in stripe 2 decides which group is the maximum: two
    pairs and a triple.  Odd frames: stripe 0 is a plateau (all K channels equal, cell by cell); in stripes 1 and 2 the pair (s1, s4) is
    (-0.0, +0.0) and (+0.0, -0.0) over K - 2 channels below -bump (the lerp returns +0.0 for either: the tie is exact and at 0)."""
    K = len(cls)
    assert K >= 6, "the tie layout needs six classes"
    s = list(cls)
    z = rng.standard_normal((B, h, w, NC)).astype(F32)
    st = stripes(w)
    bump = F32(bump)
    for b in range(B):
        if b % 2 == 0:
            z[b, :, :, s[1]] = z[b, :, :, s[0]]
            z[b, :, :, s[3]] = z[b, :, :, s[2]]
            z[b, :, :, s[4]] = z[b, :, :, s[2]]
            for group, cols in (((0, 1), st == 0), ((2, 3, 4), st == 1), ((2, 3), st == 2)):
                for g in group:
                    z[b, :, cols, s[g]] = z[b, :, cols, s[g]] + bump
        else:
            plateau = st == 0
            for k in range(1, K):
                z[b, :, plateau, s[k]] = z[b, :, plateau, s[0]]
            for r, (za, zb) in ((1, (-0.0, 0.0)), (2, (0.0, -0.0))):
                cols = st == r
                for k in range(K):
                    z[b, :, cols, s[k]] = -bump - np.abs(z[b, :, cols, s[k]])
                z[b, :, cols, s[1]] = F32(za)
                z[b, :, cols, s[4]] = F32(zb)
    return z


def ties(h, w, H, W, NC, cls, th, tw, seed, B=2):
    """Exact ties of the maximum (for `>` against `>=` and for the order in which a read-out visits the classes): two pairs, a triple, a
    plateau of all K classes (label 0, ssum == K, p == 1.f / K, loss log K) and a -0.0 / +0.0 pair in both orders (_tied_grid has the
    layout; bump 6).  The teacher's class is the lower index of the tied group in 45 % of the pixels, the higher in 45 %, any class in
    the rest; 10 % are ignored.  The teacher logits carry the same ties with a bump of 60: under conf_gamma max_k p_k is 1/2, 1/3, 1/K
    with psum an exact integer in f32."""
    rng = np.random.default_rng(seed)
    logits = _tied_grid(rng, B, h, w, NC, cls, 6.0)
    z = interpolate_selected(logits, cls, H, W)
    lo, hi = first_maximum(z), last_maximum(z)
    u = rng.random((B, H, W))
    ids = np.asarray(cls)
    teacher = np.where(u < 0.45, ids[lo], np.where(u < 0.9, ids[hi], rng.integers(0, NC, (B, H, W)))).astype(np.uint8)
    teacher = _ignore(rng, teacher)
    tl = _tied_grid(rng, B, th, tw, NC, cls, 60.0)
    return logits, teacher, tl


def quantised(h, w, NC, cls, seed, B=2):
    """For the identity resize alone (H, W = h, w; the teacher logits on the same grid): every logit a multiple of 0.5 in [-4, 4], so ties
    fall at random between random classes and the values compared are the cached samples themselves."""
    rng = np.random.default_rng(seed)
    logits = (rng.integers(-8, 9, (B, h, w, NC)) * 0.5).astype(F32)
    teacher = _ignore(rng, rng.integers(0, NC, (B, h, w)).astype(np.uint8))
    tl = (rng.integers(-8, 9, (B, h, w, NC)) * 0.5).astype(F32)
    return logits, teacher, tl


def _saturated_grid(rng, winners, NC, cls, margins, contested=None):
    """N(0, 1) + per cell a margin out of `margins` on the cell's winner (winners: subset positions [B, gh, gw]).  contested (bool
    [B, gh, gw] or None): in those cells a second class, one per frame and never cls[0] in an odd frame, stands 0.5, 1, 2 or 3 below the
    winner."""
    B, gh, gw = winners.shape
    K = len(cls)
    ids = np.asarray(cls)
    z = rng.standard_normal((B, gh, gw, NC)).astype(F32)
    margin = rng.choice(np.asarray(margins, dtype=F32), (B, gh, gw))
    bi, yi, xi = np.indices((B, gh, gw))
    z[bi, yi, xi, ids[winners]] += margin
    for b in range(B if contested is not None else 0):
        i, j = np.nonzero(contested[b])
        first = winners[b, i, j]
        assert (first == first[0]).all(), "a contested region has one winner"
        second = int(rng.choice([k for k in range(b % 2, K) if k != first[0]]))
        z[b, i, j, ids[second]] = z[b, i, j, ids[first]] - rng.choice(np.asarray([0.5, 1.0, 2.0, 3.0], dtype=F32), i.size)
    return z


def saturated(h, w, H, W, NC, cls, th, tw, seed, B=2):
    """A confident student, what fine-tuning produces: per cell a winner with a margin of 40, 90 or 200 over N(0, 1).  Winners are constant
    over blocks of 3 x 3 cells, so the interior has p == 1.0f exactly, every other softmax entry underflowing (below 2^-149 in f64 at 200),
    and they change between blocks, so the borders run through crossings.  The top left block of every frame is contested
    (_saturated_grid): the mid-range confidences, which the crossings alone supply to under 5 % of the pixels and at the identity resize
    to none.  The teacher agrees with the student's label in one half of the frame, the upper in even frames and the lower in odd ones (loss
    about 0: whole cells see nothing but correct, saturated pixels), and names another subset class in the other half (loss about the
    margin); 10 % are ignored.  In odd frames cls[0] wins nowhere: a class slot beyond K, which repeats
    cls[0]'s logit, lies far below the maximum.  The teacher logits are saturated the same way with a bump of 60; 30 % of their winners
    are drawn anew."""
    rng = np.random.default_rng(seed)
    K = len(cls)
    ids = np.asarray(cls)
    gh, gw = -(-h // 3), -(-w // 3)
    blocks = np.stack([rng.integers(b % 2, K, (gh, gw)) for b in range(B)])
    winners = np.repeat(np.repeat(blocks, 3, axis=1), 3, axis=2)[:, :h, :w]
    contested = np.zeros((B, h, w), dtype=bool)
    contested[:, :3, :3] = True
    logits = _saturated_grid(rng, winners, NC, cls, MARGINS, contested)
    arg = first_maximum(interpolate_selected(logits, cls, H, W))
    other = (arg + rng.integers(1, K, arg.shape)) % K
    upper = (np.arange(H) < H / 2)[None, :, None]
    agree = np.where((np.arange(B) % 2 == 0)[:, None, None], upper, ~upper)
    teacher = _ignore(rng, ids[np.where(agree, arg, other)].astype(np.uint8))
    ys = np.rint(np.linspace(0, h - 1, th)).astype(np.int64)
    xs = np.rint(np.linspace(0, w - 1, tw)).astype(np.int64)
    tw_ = winners[:, ys][:, :, xs]
    tw_ = np.where(rng.random(tw_.shape) < 0.3, rng.integers(0, K, tw_.shape), tw_)
    tl = _saturated_grid(rng, tw_, NC, cls, (60.0,))
    return logits, teacher, tl


def nonfinite(H, W, NC, cls, th, tw, seed, B=2):
    """Divergence as data, on the 5 x 9 grid: 2 N(0, 1) material (noise + a bump of 3 for the teacher logits, which stay finite) with, in
    frame 0 alone, a quiet NaN in channel cls[2] of cell (1, 1) — it never wins —, a NaN in cls[0] of cell (1, 5) — it keeps label 0 —, +inf
    in cls[1] of cell (3, 2) and -inf in cls[3] of cell (3, 6).  The pixels with a tap on one of the four cells (a tap of weight 0 counts:
    0 * inf is a NaN) form four disjoint sets.  Returns (logits, teacher, teacher_logits, affected, replaced): affected bool [B,H,W], those
    pixels; replaced, the logits with the four cells set to 0 in every channel."""
    h, w = NONFINITE_GRID
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((B, h, w, NC)) * 2).astype(F32)
    teacher = _ignore(rng, rng.integers(0, NC, (B, H, W)).astype(np.uint8))
    tl = rng.standard_normal((B, th, tw, NC)).astype(F32)
    ys = np.rint(np.linspace(0, H - 1, th)).astype(np.int64)
    xs = np.rint(np.linspace(0, W - 1, tw)).astype(np.int64)
    lab = np.where(teacher < NC, teacher, 0)[:, ys][:, :, xs].astype(np.int64)
    np.put_along_axis(tl, lab[..., None], np.take_along_axis(tl, lab[..., None], -1) + F32(3), axis=-1)
    replaced = logits.copy()
    affected = np.zeros((B, H, W), dtype=bool)
    for i, j, k, v in NONFINITE_CELLS:
        logits[0, i, j, cls[k]] = v
        replaced[0, i, j, :] = 0
        affected[0] |= footprint(h, w, H, W, i, j)
    return logits, teacher, tl, affected, replaced


def footprint(h, w, H, W, i, j):
    """bool [H, W]: the pixels with a tap, of whatever weight, on cell (i, j)"""
    y0, y1, _ = _taps(h, H)
    x0, x1, _ = _taps(w, W)
    return ((y0 == i) | (y1 == i))[:, None] & ((x0 == j) | (x1 == j))[None, :]


def cells_of(h, w, H, W, pixels):
    """bool [B, h, w]: the cells with a tap from one of `pixels` (bool [B, H, W]): where a pixel's gradient can land"""
    y0, y1, _ = _taps(h, H)
    x0, x1, _ = _taps(w, W)
    out = np.zeros((pixels.shape[0], h, w), dtype=bool)
    b, y, x = np.nonzero(pixels)
    for ys in (y0, y1):
        for xs in (x0, x1):
            out[b, ys[y], xs[x]] = True
    return out


# ---------------------------------------------------------------------------------------------------- the cases of the GPU suites
SUB6 = [0, 1, 2, 10, 11, 13]              # KMAX = 8: the register forms
SUB19 = list(range(19))                   # per pixel in the read-outs, KMAX = 20 in the loss
SUB21 = list(range(21))                   # KMAX = 32 (the kd mix form alone)
# (h, w, H, W): the smallest that reach both code forms; the identity; a second column strip that is mostly dead
HEAD_SHAPES = [(5, 9, 32, 64), (5, 9, 5, 9), (3, 5, 7, 300)]
IDENTITY = (5, 9, 5, 9)
LOSS_SHAPE = (5, 9, 32, 64)
LOSS_GRIDS = [(32, 64), (9, 17)]          # the teacher logits at the label size and on a smaller grid


def cases():
    """every (regime, (h, w, H, W), NC, cls, (th, tw)) a GPU test runs"""
    out = []
    for cls in (SUB6, SUB19):
        for shape in HEAD_SHAPES:
            for regime in ("ties", "saturated") + (("quantised", "nonfinite") if shape == IDENTITY else ()):
                out.append((regime, shape, 19, cls, shape[2:]))
        for grid in LOSS_GRIDS:
            for regime in ("ties", "saturated", "nonfinite"):
                if (regime, LOSS_SHAPE, 19, cls, grid) not in out:
                    out.append((regime, LOSS_SHAPE, 19, cls, grid))
    for regime in ("ties", "saturated"):
        out.append((regime, LOSS_SHAPE, 21, SUB21, LOSS_GRIDS[1]))
    return out


_MATERIAL = {}


def material(regime, shape, NC, cls, grid):
    """The case's arrays, generated once and shared (nothing writes to them): the generator's tuple."""
    key = (regime, tuple(shape), NC, tuple(cls), tuple(grid))
    if key not in _MATERIAL:
        h, w, H, W = shape
        seed = 1000 * h * w + H + W + len(cls) + grid[0]
        if regime == "ties":
            m = ties(h, w, H, W, NC, cls, grid[0], grid[1], seed)
        elif regime == "saturated":
            m = saturated(h, w, H, W, NC, cls, grid[0], grid[1], seed)
        elif regime == "quantised":
            assert (h, w) == (H, W) == tuple(grid)
            m = quantised(h, w, NC, cls, seed)
        else:
            assert regime == "nonfinite" and (h, w) == NONFINITE_GRID
            m = nonfinite(H, W, NC, cls, grid[0], grid[1], seed)
        for a in m:
            a.setflags(write=False)
        _MATERIAL[key] = m
    return _MATERIAL[key]
