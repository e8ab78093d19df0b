"""The streaming expand + depthwise kernels skip the steps that are only padding (ams_amd/csrc/xdw_steps.hpp): at the smallest shapes where that
logic can go wrong the result is still, bit for bit, the GEMM followed by the depthwise kernel.  No tolerance anywhere in this file.

Every buffer is guarded, poisoned and exactly sized (tests/guarded.py through the helpers of test_gpu_kernels.py): a step that is skipped
although a stored centre needs it leaves poison (a NaN) or stale values in the ring and shows in the comparison; a result element that is not
written shows in the buffer check."""
import numpy as np
import pytest
import torch

from ams_amd import hip
from test_gpu_kernels import P, _guarded_buffers, dev, gemm_guard, h2i_pack, image_guard, lib, out, run, scratch, stream  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# (AMS_XDS_FORCE: 16-channel tiles, row segments, column strips, E-waves, D-waves, blocks per chunk; AMS_XWR_FORCE: E-waves, row segments,
# column strips, blocks per channel group, row groups per E-wave and step), 0 = automatic.  Both step sizes of either kernel (LDS-weight: 4 and
# 8 E-waves; weight-register: 4 E-waves with 1 and 2 row groups, and 8 E-waves) with the automatic segments, with ONE block per chunk /
# channel group — it walks every item, items of different T_item back to back, the ring slots carried from one to the next — and with three
# row segments and two column strips: a short last segment, and segments past the end of the smaller sub-images (items that are not live).
PLANS = [("2,0,0,4,4,0", "4,0,0,0,1"), ("2,0,0,8,4,0", "4,0,0,0,2"), ("4,0,0,4,4,0", "8,0,0,0,1"),
         ("2,0,0,4,4,1", "4,0,0,1,1"), ("2,0,0,8,4,1", "4,0,0,1,2"), ("4,0,0,4,4,1", "8,0,0,1,1"),
         ("2,3,2,4,4,0", "4,3,2,0,1"), ("2,3,2,8,4,0", "4,3,2,0,2"), ("4,3,2,4,4,0", "8,3,2,0,1"),
         ("2,3,2,4,4,1", "4,3,2,1,1"), ("2,3,2,8,4,1", "4,3,2,1,2"), ("4,3,2,4,4,1", "8,3,2,1,1")]

CASES = [
    # 3x3 and 4x5 under rate 2, one frame and three: four sub-images of different rows and columns (at 3x3 one is 1x1: nearly every step
    # is zero or idle)
    (1, 3, 3, 64, 96, 2, PLANS), (3, 3, 3, 64, 96, 2, PLANS), (1, 4, 5, 64, 96, 2, PLANS), (3, 4, 5, 64, 96, 2, PLANS),
    # 7x6, both rates, three frames: with three row segments the last one is short (rate 1: 3 + 3 + 1 rows)
    (3, 7, 6, 64, 96, 1, PLANS), (3, 7, 6, 64, 96, 2, PLANS),
    # 64 -> 160: the weight-register kernel's last channel group is short (its `active` branch beside the step classes)
    (3, 4, 5, 64, 160, 2, PLANS), (3, 7, 6, 64, 160, 1, PLANS),
    # the timed layer's channel counts at a small frame, the automatic plan
    (2, 9, 17, 160, 960, 2, [(None, None)]),
]


@pytest.mark.parametrize("B,H,W,Cin,Cexp,rate,plans", CASES, ids=lambda v: "plans%d" % len(v) if isinstance(v, list) else str(v))
def test_skipped_padding_steps_change_no_bit(lib, B, H, W, Cin, Cexp, rate, plans, knobs):
    knobs(AMS_XDS_FORCE=None, AMS_XWR_FORCE=None)
    rng = np.random.default_rng(1000 * H + 10 * W + Cexp + rate + B)
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    we = (rng.standard_normal((Cin, Cexp)) / np.sqrt(Cin)).astype(np.float32)
    wd = (rng.standard_normal((3, 3, Cexp, 1)) * 0.4).astype(np.float32)
    se, sd = rng.uniform(0.5, 1.5, Cexp).astype(np.float32), rng.uniform(0.5, 1.5, Cexp).astype(np.float32)
    he, hd = rng.standard_normal(Cexp).astype(np.float32), rng.standard_normal(Cexp).astype(np.float32)
    xd, wed, sed, hed, wdd, sdd, hdd = (dev(a) for a in (x, we, se, he, wd, sd, hd))
    M, Kp = B * H * W, (Cin + 31) // 32 * 32

    def unfused(gemm, planes):
        """the pair of kernels the fused ones replace, once per case"""
        ebuf = out((M, Cexp), guard=gemm_guard(Cexp))
        pan = scratch(planes * Cexp * Kp, torch.int16)
        run(gemm(pan, ebuf), "the GEMM of the unfused pair")
        y = out((B, H, W, Cexp), guard=image_guard(W, Cexp))
        run(lib.ams_k_depthwise3x3(P(ebuf), B, H, W, Cexp, P(wdd), 1, rate, P(sdd), P(hdd), hip.ACT_RELU6, P(y), stream()))
        return y.cpu().numpy()

    want_f16 = unfused(lambda pan, e: lib.ams_k_pointwise_split_f16(P(xd), M, Cin, P(wed), Cexp, P(sed), P(hed), hip.ACT_RELU6, None, P(e), P(pan),
                                                                    pan.numel(), None, None, stream()), 2)
    want_bf16 = unfused(lambda pan, e: lib.ams_k_pointwise_split3(P(xd), M, Cin, P(wed), Cexp, P(sed), P(hed), hip.ACT_RELU6, None, P(e), P(pan),
                                                                  pan.numel(), stream()), 3)
    packed = h2i_pack(want_f16.reshape(M, Cexp))
    for xds, xwr in plans:
        knobs(AMS_XDS_FORCE=xds, AMS_XWR_FORCE=xwr)
        eight = xds is not None and xds.split(",")[3] == "8"          # the fp16 form of the LDS-weight kernel runs with 4 + 4 waves only
        for pre in (0, 1, 2):
            what = "%s | %s presplit %d" % (xds, xwr, pre)
            # the bf16-part entry: both forms of the LDS-weight kernel's operand, and the weight-register kernel on three parts
            n = 3 * Cexp * Cin + (3 * M * Cin if pre else 0)
            y = out((B, H, W, Cexp), guard=image_guard(W, Cexp))
            run(lib.ams_k_expand_dw_stream(P(xd), B, H, W, Cin, P(wed), P(sed), P(hed), Cexp, P(wdd), rate, P(sdd), P(hdd), P(y),
                                           P(scratch(n, torch.int16)), n, 3, pre, stream()), "expand_dw_stream " + what)
            assert np.array_equal(y.cpu().numpy(), want_bf16), what
            if eight and pre != 2:
                continue
            n = 2 * Cexp * Cin + (2 * M * Cin if pre else 0)
            for y_h2i in (0, 1):                                      # both output formats
                y = out((B, H, W, Cexp), guard=image_guard(W, Cexp))
                run(lib.ams_k_expand_dw_stream_f16(P(xd), B, H, W, Cin, P(wed), P(sed), P(hed), Cexp, P(wdd), rate, P(sdd), P(hdd), P(y),
                                                   P(scratch(n, torch.int16)), n, pre, y_h2i, stream()), "expand_dw_stream_f16 " + what)
                got = y.cpu().numpy()
                if y_h2i:
                    assert np.array_equal(got.view(np.uint16).reshape(M, Cexp // 8, 2, 8), packed), what
                else:
                    assert np.array_equal(got, want_f16), what
