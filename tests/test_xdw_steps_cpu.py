"""The steps of the streaming expand + depthwise kernels (ams_amd/csrc/xdw_steps.hpp) through ams_k_expand_dw_steps: host arithmetic, no GPU.

The entry walks the launchers' own geometry with the rule the kernels' step loops use, so what is checked here is what is launched: the counts
of DESIGN.md 5 (2026-10-21) for the timed layers, and — against a restatement of the raster walk in Python — that no step is skipped that a
stored result needs, whatever the geometry."""
import ctypes as C
from collections import Counter

import pytest

from ams_amd import hip


def steps(B, H, W, Cin, Cexp, rate, f16, presplit):
    """-> header (STEP, Wp, SH, T, items, executed, E compute, E zero, D active, both), per item (T_item, ...), per item the T step codes"""
    lib = hip.lib()
    head = (C.c_int32 * 10)()
    hip.check(lib.ams_k_expand_dw_steps(B, H, W, Cin, Cexp, rate, f16, presplit, head, 10))
    T, items = head[3], head[4]
    n = 10 + (5 + T) * items
    out = (C.c_int32 * n)()
    hip.check(lib.ams_k_expand_dw_steps(B, H, W, Cin, Cexp, rate, f16, presplit, out, n))
    out = list(out)
    assert out[:10] == list(head)
    per_item = [tuple(out[10 + 5 * i:15 + 5 * i]) for i in range(items)]
    codes = [tuple(out[10 + 5 * items + T * i:10 + 5 * items + T * (i + 1)]) for i in range(items)]
    return out[:10], per_item, codes


# (T_item, E compute, E zero, D active, E compute and D active) of an item -> how many items of the launch
TABLES = [
    # weight-register kernel, 33x65, rate 2, 160 -> 960: STEP 32, Wp 35, SH 17, T 21; sub-images of 17 and of 16 rows
    ((16, 33, 65, 160, 960, 2, 1, 2), (32, 35, 17, 21, 64), {(21, 19, 2, 19, 18): 32, (20, 18, 2, 18, 17): 32}),
    ((32, 33, 65, 160, 960, 2, 1, 2), (32, 35, 17, 21, 128), {(21, 19, 2, 19, 18): 64, (20, 18, 2, 18, 17): 64}),
    # LDS-weight kernel, 33x65, rate 1, STEP 64, Wp 67.  16 frames, 64 -> 384: four row segments of 9, 9, 9 and 6 rows, T 12: 10, 10, 10 and
    # 7 active D-steps; the last segment ends after 9 steps (3 of the 12 have no work for either role)
    ((16, 33, 65, 64, 384, 1, 1, 1), (64, 67, 9, 12, 64), {(12, 11, 1, 10, 10): 16, (12, 12, 0, 10, 10): 32, (9, 8, 1, 7, 6): 16}),
    # 16 frames, 96 -> 576: three segments of 11 rows, T 14, 12 active D-steps in each
    ((16, 33, 65, 96, 576, 1, 1, 1), (64, 67, 11, 14, 48), {(14, 13, 1, 12, 12): 16, (14, 14, 0, 12, 12): 16, (14, 13, 1, 12, 11): 16}),
    # 32 frames: two segments of 17 and 16 rows, T 20, 18 and 17 active D-steps
    ((32, 33, 65, 64, 384, 1, 1, 1), (64, 67, 17, 20, 64), {(20, 19, 1, 18, 18): 32, (19, 18, 1, 17, 16): 32}),
    ((32, 33, 65, 96, 576, 1, 1, 1), (64, 67, 17, 20, 64), {(20, 19, 1, 18, 18): 32, (19, 18, 1, 17, 16): 32}),
]


@pytest.mark.parametrize("args,geom,items", TABLES)
def test_step_counts_of_the_timed_layers(args, geom, items, knobs):
    knobs(AMS_XDS_FORCE=None, AMS_XWR_FORCE=None)
    head, per_item, codes = steps(*args)
    assert tuple(head[:5]) == geom
    assert Counter(per_item) == Counter(items)
    assert head[5:] == [sum(p[k] for p in per_item) for k in range(5)]
    for p, c in zip(per_item, codes):
        assert p[0] == sum(1 for v in c if v & 8)


def check_item(Wp, STEP, SH, R, Hs, Ws, i0, j0, sbase, cb, codes):
    """One item walked as the kernels walk it, with the ring slots as they stand when the item begins (sbase: slot of the E-waves' position 0,
    cb: slot of the first tap of the D-waves' first centre, both carried from the items before).  E-step t writes positions
    [t STEP, (t + 1) STEP); D-step t follows it, beside E-step t + 1, and takes the centres [t STEP - Wp - 1, (t + 1) STEP - Wp - 1)."""
    live = i0 < Hs and j0 < Ws
    rows = min(SH, Hs - i0) if live else 0
    cols = min(Wp - 2, Ws - j0)

    def inside(p):
        row, col = divmod(p, Wp)
        return live and 0 <= i0 - 1 + row < Hs and 0 <= j0 - 1 + col < Ws and row < SH + 2

    def is_read(p):                      # by a stored centre
        row, col = divmod(p, Wp)
        return rows > 0 and row <= rows + 1 and col <= cols + 1

    T_item = sum(1 for c in codes if c & 8)
    assert all(c & 8 for c in codes[:T_item]) and not any(c & 15 for c in codes[T_item:]), "executed steps are a prefix; no work behind them"
    if T_item:                           # both roles end at the same step: the last stored centre's D-step, whose last tap that E-step writes
        assert codes[T_item - 1] & 4 and codes[T_item - 1] & 3
    with_inside = [p // STEP for p in range((SH + 2) * Wp) if inside(p)]
    ring = {}
    prev_reads = set()
    n_inside = n_stored = 0
    for t in range(T_item):
        cls, act = codes[t] & 3, bool(codes[t] & 4)
        ins = [inside(p) for p in range(t * STEP, (t + 1) * STEP)]
        assert not any(ins) or cls == 2, "an E-step that holds a position of the feature map computes"
        assert (cls == 2) == (bool(with_inside) and with_inside[0] <= t <= with_inside[-1]), "and so do exactly the steps between two such"
        assert (cls != 0) == any(is_read(p) for p in range(t * STEP, (t + 1) * STEP)), "zero: no position inside, but one that is read"
        n_inside += sum(ins)
        if cls:
            for k in range(STEP):
                slot = (sbase + k) % R
                assert slot not in prev_reads, "E-step t + 1 overwrites what D-step t reads beside it"
                ring[slot] = (t * STEP + k, ins[k])
        reads = set()
        stored_here = 0
        c0 = t * STEP - Wp - 1
        for k in range(max(0, -c0), STEP):
            row, col = divmod(c0 + k, Wp)
            if 1 <= row <= rows and 1 <= col <= cols:
                stored_here += 1
                for di in range(3):
                    for dj in range(3):
                        pos = c0 + k + (di - 1) * Wp + dj - 1
                        slot = (cb + k + di * Wp + dj) % R
                        assert ring.get(slot) == (pos, inside(pos)), "a stored centre reads a slot that holds its tap: the value or the padding's 0"
                        reads.add(slot)
        assert act == (stored_here > 0), "a D-step is active exactly when it holds a stored centre"
        n_stored += stored_here
        prev_reads = reads
        sbase = (sbase + STEP) % R
        cb = (cb + STEP) % R
    assert n_stored == rows * cols, "every stored centre lies in an executed, active D-step"
    assert n_inside == sum(inside(p) for p in range((SH + 2) * Wp)), "every position inside the feature map lies in an E compute step"
    return sbase, cb


SIZES = [(h, w) for h in range(1, 13) for w in range(1, 13)] + [(17, 33), (33, 65)]
# (presplit, f16, Cin, Cexp, knob, its value for (nsy, nsx), STEP): the LDS-weight kernel with 4 and 8 E-waves (the bf16-part entry: the fp16
# form runs with 4 + 4 waves only), the weight-register kernel with one and two row groups; one block per chunk / channel group
KERNELS = [(0, 0, 64, 96, "AMS_XDS_FORCE", "2,%d,%d,4,4,1", 64), (0, 0, 64, 96, "AMS_XDS_FORCE", "2,%d,%d,8,4,1", 128),
           (2, 1, 64, 96, "AMS_XWR_FORCE", "4,%d,%d,1,1", 16), (2, 1, 64, 96, "AMS_XWR_FORCE", "4,%d,%d,1,2", 32)]


@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: "%s-step%d" % (k[4][4:7].lower(), k[6]))
@pytest.mark.parametrize("rate", [1, 2])
def test_no_needed_step_is_skipped(kernel, rate, knobs):
    """Exhaustive over H, W in 1 .. 12 plus 17x33 and 33x65, 1 .. 4 forced row segments and 1 .. 3 forced column strips: the items of one block
    in its order, the ring slots carried from item to item (items of different T_item follow each other: the smaller sub-images, the short
    last segments, the segments past the end of a sub-image, which have no step at all)."""
    presplit, f16, Cin, Cexp, knob, force, STEP = kernel
    seen = {}
    for H, W in SIZES:
        for nsy in range(1, 5):
            for nsx in range(1, 4):
                knobs(**{"AMS_XDS_FORCE": None, "AMS_XWR_FORCE": None, knob: force % (nsy, nsx)})
                head, per_item, codes = steps(1, H, W, Cin, Cexp, rate, f16, presplit)
                assert head[0] == STEP
                Wp, SH, T, items = head[1:5]
                SW = Wp - 2
                nsx_real = -(-(-(-W // rate)) // SW)                 # ceil(ceil(W / rate) / SW): the launchers recompute the strips from the strip width
                assert items == rate * rate * nsy * nsx_real and T == -(-(SH + 2) * Wp // STEP)
                R = (2 * Wp + 2 + 2 * STEP + STEP - 1) // STEP * STEP
                sbase, cb = 0, (2 * R - 2 * Wp - 2) % R
                for item in range(items):
                    segx, u = item % nsx_real, item // nsx_real
                    segy, sub = u % nsy, u // nsy
                    sy, sx = sub // rate, sub % rate
                    Hs, Ws = (H - sy + rate - 1) // rate, (W - sx + rate - 1) // rate
                    key = (Wp, SH, R, Hs, Ws, segy * SH, segx * SW, sbase, cb, codes[item])
                    if key not in seen:
                        seen[key] = check_item(Wp, STEP, SH, R, Hs, Ws, segy * SH, segx * SW, sbase, cb, codes[item])
                    sbase, cb = seen[key]
                    assert per_item[item][0] == sum(1 for c in codes[item] if c & 8)
                    assert (cb - sbase) % R == (-2 * Wp - 2) % R, "the D-waves' slot stays 2 Wp + 2 behind the E-waves' from item to item"
