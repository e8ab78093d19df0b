"""The frozen head as one chained kernel (ams_amd/csrc/k_head_chain.hip, AMS_OPT_FUSE_HEAD bit 0) and the f32 stores bit 1 of the option
drops (PwArgs::y_skip_f32: a project result whose only reader takes the part planes) against the plan without either, on the same engine.

Per output element the chained kernel forms the products, joins the two accumulators and applies the epilogues exactly as the three
launches it replaces, so every comparison here is one of bits: np.array_equal on the 19 low-resolution logit columns, torch.equal on the
label maps.  Nothing is compared against an oracle: the unfused plan has its own tests.

Geometries.  64 x 128 frames give a 5 x 9 low-resolution grid, 45 rows per image: no row count below is a multiple of the wave's 16 rows
or the block's 64, and every 16-row tile beyond the first image straddles two images (the per-image bias is per row).  Below 256 rows
(B = 1, 2, 3, 5) the head's GEMMs run exact f32 and the plan must decline the chain; B = 6 and 7 (270 and 315 rows) are the smallest
batches at which the chain itself runs on such rows: 5 blocks, the last with 14 / 59 live rows.  Two parts: 12 and 13 frames split 6 + 6
and 7 + 6, so each part stream runs the chain on 270 / 315 ragged rows (and, with AMS_OPT_STREAM_MIN_ROWS = 0, the dropped stores);
the profiler forces one stream, so that the chain and the skip run at a part's batch size is asserted on one-stream calls of 6 and 7.
512 x 1024 at B = 2 is 4290 rows: 68 blocks, and the stride-16 blocks stream on part planes there.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine

pytestmark = pytest.mark.gpu

CI = [0, 1, 2, 10, 11, 13]
SMALL_H, SMALL_B = 64, 13


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


def make_engine(W, H, max_batch, stream_min_rows=None):
    eng = StudentEngine(CI, H, 2 * H, max_batch=max_batch, trainable=False)
    if stream_min_rows is not None:
        hip.check(eng.lib.ams_student_set_option(eng._h, hip.OPT_STREAM_MIN_ROWS, stream_min_rows))
    eng.load_variables(W)
    eng.freeze()
    return eng


@pytest.fixture(scope="module")
def small(W0):
    eng = make_engine(W0, SMALL_H, SMALL_B)
    frames, _ = synth.SyntheticVideo(SMALL_H, SMALL_B, CI, seed=5).clip()
    yield eng, frames
    eng.close()


def run(eng, frames):
    lab = eng.predict(frames).clone()
    h, w = eng.lowres
    return lab, eng.logits_lowres.view(-1, h, w, 32)[:len(frames), :, :, :19].cpu().numpy().copy()


def profile(eng, frames):
    """(kernel, layer, algorithmic bytes) of every launch of one profiled frozen call (the profiler runs the call on one stream)"""
    hip.check(eng.lib.ams_student_profile(eng._h, 1))
    try:
        eng.predict(frames)
        need = C.c_size_t()
        hip.check(eng.lib.ams_student_profile_read(eng._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 16)
        hip.check(eng.lib.ams_student_profile_read(eng._h, buf, len(buf), C.byref(need)))
    finally:
        hip.check(eng.lib.ams_student_profile(eng._h, 0))
    rows = [line.split("\t") for line in buf.value.decode().splitlines()]
    return [(f[0], int(f[1]), float(f[3])) for f in rows]


def kernels(eng, frames):
    return [r[0] for r in profile(eng, frames)]


def skipped_stores(eng, frames):
    """layers whose project GEMM reports 4 M N bytes less with bit 1 of the option than without: the f32 stores really dropped"""
    h, w = eng.lowres
    M = len(frames) * h * w
    eng.set_fuse_head(0)
    base = profile(eng, frames)
    eng.set_fuse_head(2)
    skip = profile(eng, frames)
    assert [r[:2] for r in base] == [r[:2] for r in skip]               # same launches, same order
    out = []
    for (name, layer, b0), (_, _, b1) in zip(base, skip):
        if b0 != b1:
            cout = S.build_spec().layers[layer - 1].cout
            assert S.build_spec().layers[layer - 1].idx == layer and b0 - b1 == 4.0 * M * cout, (name, layer, b0, b1)
            out.append(layer)
    return out


def both_plans(eng, frames, what):
    eng.set_fuse_head(False)
    lab0, low0 = run(eng, frames)
    eng.set_fuse_head(True)
    lab1, low1 = run(eng, frames)
    assert np.isfinite(low0).all(), what
    assert np.array_equal(low1, low0), "%s: %d of %d low-resolution logits differ, max |diff| %g" % (
        what, int((low1 != low0).sum()), low0.size, float(np.abs(low1 - low0).max()))
    assert torch.equal(lab1, lab0), what


@pytest.mark.parametrize("B", [1, 2, 3, 5, 6, 7])
def test_ragged_rows_and_tiles_across_images(small, B):
    """45 rows per image, one stream"""
    eng, frames = small
    eng.set_dual_stream(0)
    try:
        both_plans(eng, frames[:B], "B %d, one stream" % B)
    finally:
        eng.set_dual_stream(1, parts=2)
        eng.set_fuse_head(True)


@pytest.mark.parametrize("B", [1, 2, 3, 5, 12, 13])
def test_two_parts(small, B):
    """two parts on two streams (from 2 frames on): up to 5 frames no part reaches 256 rows and the plan declines on both; 6 + 6 and
    7 + 6 frames are 270 / 315 rows a part: the chain runs
    on the caller's stream and on the part stream; asserted at those batch sizes by test_plan_takes_the_chain_from_256_rows_on)"""
    eng, frames = small
    eng.set_dual_stream(2, parts=2)
    try:
        both_plans(eng, frames[:B], "B %d, two parts" % B)
    finally:
        eng.set_dual_stream(1, parts=2)
        eng.set_fuse_head(True)


def test_plan_takes_the_chain_from_256_rows_on(small):
    """the chain replaces the three GEMMs where they would run the fp16 product (>= 256 rows) and nowhere else"""
    eng, frames = small
    eng.set_dual_stream(0)
    try:
        eng.set_fuse_head(True)
        assert kernels(eng, frames[:6]).count("head_chain_kernel") == 1      # ... and 6 and 7 frames are what a part of test_two_parts holds
        assert kernels(eng, frames[:7]).count("head_chain_kernel") == 1
        eng.set_fuse_head(1)                                                # bit 0 alone
        assert kernels(eng, frames[:6]).count("head_chain_kernel") == 1
        eng.set_fuse_head(2)                                                # bit 1 alone: no chain
        assert "head_chain_kernel" not in kernels(eng, frames[:6])
        eng.set_fuse_head(True)
        assert "head_chain_kernel" not in kernels(eng, frames[:5])          # 225 rows: exact-f32 GEMMs, three launches
        eng.set_fuse_head(False)
        assert "head_chain_kernel" not in kernels(eng, frames[:6])
    finally:
        eng.set_dual_stream(1, parts=2)
        eng.set_fuse_head(True)


def test_full_size_geometry(W0):
    """512 x 1024, B = 2: 4290 rows in 68 blocks (the last with 2 live rows); the stride-16 blocks stream, so the dropped stores run too"""
    eng = make_engine(W0, 512, 2)
    try:
        frames, _ = synth.SyntheticVideo(512, 2, CI, seed=5).clip()
        assert kernels(eng, frames).count("head_chain_kernel") == 1
        assert len(skipped_stores(eng, frames)) == 3                        # the outputs feeding 64 -> 96, 96 -> 160 and 160 -> 320
        both_plans(eng, frames, "512 x 1024, B 2")
    finally:
        eng.close()


def test_range_fallback_declines_the_chain(W0):
    """aspp0's weights beyond fp16's range (x 2^20, its BN compensating: the same function): the freeze moves the layer to three bf16 parts and
    the head keeps its three launches, with the bits of the plan that never chains"""
    k = 20
    W = dict(W0)
    f = np.float32(2.0 ** k)
    W["aspp0/weights:0"] = W["aspp0/weights:0"] * f
    W["aspp0/BatchNorm/moving_mean:0"] = W["aspp0/BatchNorm/moving_mean:0"] * f
    W["aspp0/BatchNorm/gamma:0"] = W["aspp0/BatchNorm/gamma:0"] * np.float32(2.0 ** -k)
    assert np.abs(W["aspp0/weights:0"]).max() > 65504
    eng = make_engine(W, SMALL_H, SMALL_B)
    try:
        frames, _ = synth.SyntheticVideo(SMALL_H, SMALL_B, CI, seed=5).clip()
        eng.set_dual_stream(0)
        eng.set_fuse_head(True)
        assert "head_chain_kernel" not in kernels(eng, frames)
        both_plans(eng, frames, "aspp0 x 2^%d" % k)
    finally:
        eng.close()


def test_dropped_f32_stores(W0):
    """64 x 128 with AMS_OPT_STREAM_MIN_ROWS = 0: the stride-16 blocks stream at any row count, and from 256 rows on their project GEMMs
    hand part planes over — without the f32 copy where the next block adds no residual.  One stream at 6 and 7 frames: the three stores
    are really dropped (the launches' algorithmic bytes say so) and the logits are those of the plan that stores everything; at 3 frames
    (135 rows) no planes are handed over and nothing is dropped.  Then 12 and 13 frames as two parts of 6 / 7: the skip on both streams."""
    eng = make_engine(W0, SMALL_H, SMALL_B, stream_min_rows=0)
    try:
        frames, _ = synth.SyntheticVideo(SMALL_H, SMALL_B, CI, seed=9).clip()
        eng.set_dual_stream(0)
        assert skipped_stores(eng, frames[:3]) == []
        for B in (6, 7):
            assert len(skipped_stores(eng, frames[:B])) == 3
            both_plans(eng, frames[:B], "stream_min_rows 0, B %d, one stream" % B)
        eng.set_dual_stream(2, parts=2)
        for B in (12, 13):
            both_plans(eng, frames[:B], "stream_min_rows 0, B %d, two parts" % B)
    finally:
        eng.close()
