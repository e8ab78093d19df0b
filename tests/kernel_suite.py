"""What the kernel-level GPU suites (tests/test_gpu_kernels.py, tests/test_gpu_entry_corners.py) share: the guarded buffers of tests/guarded.py
behind short names, `run` / `refused` after every call, the error measure, the guard sizes, and the scratch formulas of include/ams_hip.h that have
no *_scratch() entry.  The two fixtures are imported by name into each suite (pytest finds a fixture in the module that imports it).

Buffers: every result is a view inside a larger buffer pre-filled with the NaN pattern 0x7FC12345 — after the call both guards must hold the
pattern bit for bit and no element of the result may; every operand lies between guards of the same pattern; every scratch region and panel set
has exactly the size the entry states and is poisoned, never zeroed.  Guards: GEMM results 256 rows x N (the tallest row tile a launcher picks),
image results eight image rows, everything else 4096 elements."""
import ctypes as C

import numpy as np
import pytest
import torch

import guarded as G
from ams_amd import hip

E_INVALID, E_HIP = -1, -2          # AMS_E_INVALID, AMS_E_HIP


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip.lib()


@pytest.fixture(autouse=True)
def _guarded_buffers():
    """Every buffer of a test lives until the test ends (kernels run asynchronously); a result nobody checked is an error of the test."""
    G.reset()
    yield
    left = G.pending()
    G.reset()
    assert not left, "results handed out and never checked: %s" % [tuple(t.shape) for t in left]


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def lib_error():
    msg = hip.lib().ams_last_error()
    return msg.decode() if msg else "?"


def out(shape, dtype=torch.float32, guard=G.GUARD):
    """a result inside poisoned guards (tests/guarded.py); `guard` elements on either side, at least 4096"""
    return G.out(shape, dtype, guard)


def gemm_guard(N):
    """a GEMM result's guard: the tallest row tile a launcher here picks (256 rows: pw_pick_tile and the AMS_PWX_FORCE forms top out at 8 waves x
    32 rows) times N"""
    return max(G.GUARD, 256 * N)


def image_guard(W, Cn):
    """an image result's guard: eight image rows"""
    return max(G.GUARD, 8 * W * Cn)


def frames(case, small, B):
    """the frame counts a case runs with: the shapes of the parent suite keep their B; the small maps added beside them (the list `small`) run
    with ONE frame — 1x1 is then one work item in all, with nothing behind the operand and the result but guard — and with two, for the
    kernels whose work items run across frame boundaries (the streaming and weight-register kernels, the walking depthwise forms, the
    depthwise weight gradient) and at no cost for the others.  Between two frame counts the buffers of the first, all checked, are let go
    (every check looks at the guards of every live buffer)."""
    for b in ((1, 2) if case in small else (B,)):
        yield b
        left = G.pending()
        G.reset()
        assert not left, "results handed out and never checked: %s" % [tuple(t.shape) for t in left]


def dev(a, dtype=torch.float32):
    """the operand on the device, its surroundings poisoned"""
    return G.inp(a, dtype)


def PD(a, dtype=torch.float32):
    return P(dev(a, dtype))


def scratch(n, dtype=torch.float32):
    """exactly n poisoned elements of scratch between guards"""
    return G.scratch(int(n), dtype)


def run(rc, what="the call", untouched=None):
    """the entry succeeded; nothing outside its buffers was written, every element of its results was"""
    if rc == E_HIP:
        pytest.exit("%s: a HIP call failed (%s); the device may be in a failed state, nothing more runs on it" % (what, lib_error()), returncode=3)
    hip.check(rc)
    try:
        G.check(what, untouched)
    except RuntimeError as e:                  # a fault of the kernel surfaces at the synchronisation
        pytest.exit("%s: %s; nothing more runs on this device" % (what, e), returncode=3)


def refused(rc, what):
    """AMS_E_INVALID in front of the first launch: no result element and no guard was touched"""
    assert rc == E_INVALID, "%s: expected a refusal, got %d" % (what, rc)
    G.check(what, untouched=[(t, True) for t in G.pending()])


def rel_err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def cdiv(a, b):
    return -(-a // b)


def wgrad_f32_scratch(M, K, N):
    """floats the exact-f32 weight gradient needs (include/ams_hip.h): splits * K * N with splits = min(ceil(1024 / tiles), ceil(M / 256)),
    tiles = ceil(K / 64) * ceil(N / 64)"""
    return max(min(cdiv(1024, cdiv(K, 64) * cdiv(N, 64)), cdiv(M, 256)), 1) * K * N


def wgrad_x6_scratch(M, K, N):
    """floats the three-part weight gradient needs (include/ams_hip.h): splits * K * N with splits = min(ceil(512 / tiles), ceil(M / 256), 32),
    tiles = ceil(K / (16 kt)) * ceil(N / (16 nw)), kt = 8 above 64 input channels and 4 up to there, nw = the 16-column groups of a block"""
    kt, n16 = (8 if K > 64 else 4), cdiv(N, 16)
    if n16 <= 10:
        nw = 4 if n16 <= 4 else 5 if n16 <= 5 else 6 if n16 <= 6 else 8 if n16 <= 8 else 10
    else:
        nw = 10 if n16 % 10 == 0 else 8 if n16 % 8 == 0 else 6 if n16 % 6 == 0 else 8
    return max(min(cdiv(512, cdiv(K, 16 * kt) * cdiv(N, 16 * nw)), cdiv(M, 256), 32), 1) * K * N


def dw_wgrad_scratch(B, Ho, Wo, Cn):
    """floats ams_k_depthwise3x3_wgrad needs (include/ams_hip.h): one 9 x C partial per block; items = B * ceil(Ho / 4) * Wo (4 output rows x 1
    column each), blocks = min(ceil(items / (2 * slots)), max(items * 2 // 9, 1), 1024) with slots = max(256 // (C / 4), 1)"""
    items = B * ((Ho + 3) // 4) * Wo
    slots = max(256 // (Cn // 4), 1)
    return min(-(-items // (2 * slots)), max(items * 2 // 9, 1), 1024) * 9 * Cn


def f16_parts(a):
    """(hi, lo) of the two-fp16-part split as the kernels form it: hi = f16(x), lo = f16((x - hi) * 2^11), both round-to-nearest-even"""
    a = np.asarray(a, dtype=np.float32)
    hi = a.astype(np.float16)
    lo = ((a - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi, lo


def h2i_pack(a):
    """[M, C] f32 -> the H2I bytes as a uint16 array [M, C / 8, 2, 8] (per 8 channels: 8 hi, then 8 lo)"""
    hi, lo = f16_parts(a)
    M, C_ = a.shape
    return np.stack([hi.reshape(M, C_ // 8, 8), lo.reshape(M, C_ // 8, 8)], axis=2).view(np.uint16)
