"""The first block of the frozen path at the kernel level (k_first_block.hip through ams_k_first_block, the tile-per-wave form of k_block.hip
through ams_k_first_block_tiles) against the f64 reference of tests/first_block_ref.py: every product form, both frame types, both pixel scales,
at the smallest sizes that reach each path of the launcher and of the kernels' border code (first_block_ref.SIZES), and one batch in which the
walking kernels' blocks really take several tiles.  Reference, cases, measure and bars: first_block_ref.py; that they catch small defects:
tests/test_first_block_cpu.py.

Frames lie inside a larger device buffer whose surroundings hold 255 (a read outside the batch shows as a wrong value), the result inside a
larger buffer of NaN (nothing outside may change, no NaN may remain inside).

Measured on an MI355X (worst case and channel of each form): L = 8.5e-7, bars 3.4e-6 (exact-f32 forms) and 6.8e-6 (split forms); form 0 and the
tile-per-wave form 1.07e-6, form 1 1.03e-6, form 2 8.3e-7, each at 1 x 1 or 2 x 3 and at most 4.7e-7 from 9 x 7 up; the walking batch 3.1e-7 on 648 + 384
blocks for 1936 + 768 tiles ("First block: what holds it").
"""
import ctypes as C

import numpy as np
import pytest
import torch

import first_block_ref as R
from ams_amd import hip, spec as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 4096                                     # elements in front of and behind the frames / the result
SIZES = list(R.SIZES)
WNAMES = ("w_stem", "sc_s", "sh_s", "w_dw", "sc_d", "sh_d", "w_proj", "sc_p", "sh_p")
FORM_BAR = {0: "f32", 1: "split", 2: "split", "tiles": "f32"}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return hip.lib()


@pytest.fixture(scope="module")
def wd():
    """The weights on the device, in the entries' argument order."""
    w = R.weights()
    return [torch.tensor(w[n]).to(DEV).contiguous() for n in WNAMES]


@pytest.fixture(scope="module")
def bars():
    L, at = R.f32_level()
    b = R.bars()
    print("\nfirst block: f32 CPU level L = %.3g at %s -> bars: exact-f32 forms %.3g, split forms %.3g" % (L, at, b["f32"], b["split"]))
    assert b["split"] <= R.BAR_CAP
    return b


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def device_frames(arr, as_f32=False):
    """-> (the whole buffer, kept alive by the caller; the frames inside it)."""
    src = torch.tensor(np.asarray(arr)).reshape(-1)
    if as_f32:
        src = src.to(torch.float32)
    buf = torch.full((GUARD + src.numel() + GUARD,), 255, dtype=src.dtype, device=DEV)
    buf[GUARD:GUARD + src.numel()] = src.to(DEV)
    return buf, buf[GUARD:GUARD + src.numel()]


class Runner:
    def __init__(self, lib, wd, Bn, H, W, ps):
        self.lib, self.wd, self.Bn, self.H, self.W, self.ps = lib, wd, Bn, H, W, ps
        self.Ho, self.Wo = R.out_size(H, W)
        self.n = Bn * self.Ho * self.Wo * 16
        self.panels = torch.zeros(3072, dtype=torch.int16, device=DEV)
        assert lib.ams_k_first_block_scratch(1) == lib.ams_k_first_block_scratch(2) == 3072

    def _out(self):
        buf = torch.full((GUARD + self.n + GUARD,), float("nan"), device=DEV)
        return buf, buf[GUARD:GUARD + self.n]

    def _checked(self, buf, what):
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + self.n:]).all()), "%s wrote outside its result" % what
        y = buf[GUARD:GUARD + self.n]
        assert not bool(torch.isnan(y).any()), "%s left %d elements unwritten (or NaN)" % (what, int(torch.isnan(y).sum()))
        return y.view(self.Bn, self.Ho, self.Wo, 16)

    def _head(self, fr):
        dtype = hip.DT_U8 if fr.dtype == torch.uint8 else hip.DT_F32
        return (P(fr), dtype, self.Bn, self.H, self.W, C.c_float(self.ps)) + tuple(P(t) for t in self.wd)

    def form(self, fr, form):
        buf, y = self._out()
        plan = hip.FirstBlockPlan()
        self.panels.zero_()
        hip.check(self.lib.ams_k_first_block(*self._head(fr), P(y), form, P(self.panels), self.panels.numel(), C.byref(plan), stream()))
        return self._checked(buf, "form %d" % form), plan

    def tiles(self, fr):
        buf, y = self._out()
        hip.check(self.lib.ams_k_first_block_tiles(*self._head(fr), P(y), stream()))
        return self._checked(buf, "the tile-per-wave form")

    def three_kernels(self, fr):
        lib, (w_stem, sc_s, sh_s, w_dw, sc_d, sh_d, w_proj, sc_p, sh_p) = self.lib, self.wd
        dtype = hip.DT_U8 if fr.dtype == torch.uint8 else hip.DT_F32
        M = self.Bn * self.Ho * self.Wo
        # 16 rows or fewer go to the GEMM's small-M kernel (the pool branch's: another summation order).  The claim is about the MFMA GEMM the
        # engine runs on this layer, so the GEMM gets zero rows up to 32 and its first M rows are compared
        Mg = max(M, 32)
        s = torch.full((M, 32), float("nan"), device=DEV)
        d = torch.zeros((Mg, 32), device=DEV)
        d[:M] = float("nan")
        buf = torch.full((GUARD + Mg * 16 + GUARD,), float("nan"), device=DEV)
        y = buf[GUARD:]
        hip.check(lib.ams_k_stem_conv(P(fr), dtype, self.Bn, self.H, self.W, P(w_stem), 32, P(sc_s), P(sh_s), hip.ACT_RELU6, C.c_float(self.ps), P(s), stream()))
        hip.check(lib.ams_k_depthwise3x3(P(s), self.Bn, self.Ho, self.Wo, 32, P(w_dw), 1, 1, P(sc_d), P(sh_d), hip.ACT_RELU6, P(d), stream()))
        hip.check(lib.ams_k_pointwise(P(d), Mg, 32, P(w_proj), 16, 0, None, 1, P(sc_p), P(sh_p), hip.ACT_NONE, None, P(y), stream()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + Mg * 16:]).all()), "the GEMM wrote outside its result"
        y = y[:self.n]
        assert not bool(torch.isnan(y).any()), "the three kernels left elements unwritten (or NaN)"
        return y.view(self.Bn, self.Ho, self.Wo, 16)


def worst_at(a, b):
    """'(frame, row, column, channel)' of the largest difference: a border bug names its pixel."""
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    at = np.unravel_index(int(d.argmax()), d.shape)
    return "max abs diff %g at (b, y, x, c) = %s of %s, %d elements differ" % (d.max(), tuple(int(i) for i in at), d.shape, int((d > 0).sum()))


def held(y, ref, bar, what):
    got = y.cpu().numpy()
    e = R.measure(got, ref)
    print("first_block_error %s: %.3g (bar %.3g)" % (what, e, bar))
    assert e <= bar, "%s: worst channel %.3g above its bar %.3g; %s; per channel %s" % (what, e, bar, worst_at(got, ref), R.channel_errors(got, ref))
    return e


def assert_same_bits(a, b, what):
    assert same_bits(a, b), "%s: %s" % (what, worst_at(a.cpu().numpy(), b.cpu().numpy()))


@pytest.mark.parametrize("H,W", SIZES)
def test_every_form_against_f64(lib, wd, bars, knobs, H, W):
    """Forms 0, 1, 2 and the tile-per-wave entry, uint8 frames, f32 frames holding the same integers (the same bits as uint8, in every form) and
    f32 frames with fractions, at both pixel scales; form 2 on uint8 frames with AMS_FB_WALK unset and 0."""
    knobs(AMS_FB_WALK=None)
    for ps in R.PIXEL_SCALES:
        run = Runner(lib, wd, R.B, H, W, ps)
        tag = "%dx%d ps=1/%g" % (H, W, round(1.0 / ps, 1))
        ref = R.reference(R.B, H, W, "bytes", ps)
        keep_u8, fr_u8 = device_frames(R.frames(R.B, H, W, "bytes"))
        keep_fi, fr_fi = device_frames(R.frames(R.B, H, W, "bytes"), as_f32=True)
        for form in (0, 1, 2):
            y_u8, _ = run.form(fr_u8, form)
            y_fi, _ = run.form(fr_fi, form)
            held(y_u8, ref, bars[FORM_BAR[form]], "form=%d frames=uint8 %s" % (form, tag))
            held(y_fi, ref, bars[FORM_BAR[form]], "form=%d frames=f32-integers %s" % (form, tag))
            assert_same_bits(y_u8, y_fi, "form %d, %s: f32 frames holding integers against uint8 frames" % (form, tag))
        for name, fr in (("uint8", fr_u8), ("f32-integers", fr_fi)):
            held(run.tiles(fr), ref, bars["f32"], "form=tiles frames=%s %s" % (name, tag))
        knobs(AMS_FB_WALK=0)
        y_one, plan = run.form(fr_u8, 2)
        knobs(AMS_FB_WALK=None)
        assert plan.interior_tiles == 0
        held(y_one, ref, bars["split"], "form=2 frames=uint8 AMS_FB_WALK=0 %s" % tag)
        ref = R.reference(R.B, H, W, "fractions", ps)
        keep_ff, fr_ff = device_frames(R.frames(R.B, H, W, "fractions"))
        for form in (0, 1, 2):
            held(run.form(fr_ff, form)[0], ref, bars[FORM_BAR[form]], "form=%d frames=f32-fractions %s" % (form, tag))
        held(run.tiles(fr_ff), ref, bars["f32"], "form=tiles frames=f32-fractions %s" % tag)


@pytest.mark.parametrize("H,W", SIZES)
def test_exact_form_is_the_three_kernels_bit_for_bit(lib, wd, H, W):
    """k_first_block.hip's header: "arithmetic per element is the same as in the three separate kernels".  Form 0 and the tile-per-wave entry give
    the bits of ams_k_stem_conv -> ams_k_depthwise3x3 -> ams_k_pointwise."""
    for ps in R.PIXEL_SCALES:
        run = Runner(lib, wd, R.B, H, W, ps)
        for kind, as_f32 in (("bytes", False), ("bytes", True), ("fractions", False)):
            keep, fr = device_frames(R.frames(R.B, H, W, kind), as_f32)
            want = run.three_kernels(fr)
            y0, _ = run.form(fr, 0)
            yt = run.tiles(fr)
            what = "%s%s at %d x %d, pixel scale %g" % (kind, " as f32" if as_f32 else "", H, W, ps)
            assert_same_bits(y0, want, "form 0, %s" % what)
            assert_same_bits(yt, want, "tile-per-wave form, %s" % what)


@pytest.mark.parametrize("H,W", SIZES)
def test_walk_knob_changes_no_bit_and_the_plan_says_what_ran(lib, wd, knobs, H, W):
    """Form 2 on uint8 frames: AMS_FB_WALK unset, 0 (one tile per block), 1, 2, 5 (at most n tiles per walking block) and -2 (the border tiles on
    the one-tile kernel) give the same bits.  The interior launch runs exactly when the plan has a tile to walk (first_block_ref.planned_interior_tiles:
    from 34 x 68 and 36 x 66 on; at 34 x 66 the one tile with all its taps would have the kernel load bytes behind the frame)."""
    interior = len(R.planned_interior_tiles(H, W))
    for ps in R.PIXEL_SCALES:
        run = Runner(lib, wd, R.B, H, W, ps)
        keep, fr = device_frames(R.frames(R.B, H, W, "bytes"))
        first = None
        for walk in (None, 0, 1, 2, 5, -2):
            knobs(AMS_FB_WALK=walk)
            y, plan = run.form(fr, 2)
            ran = plan.interior_tiles > 0
            assert ran == (bool(interior) and walk != 0), "AMS_FB_WALK=%s at %d x %d: interior launch %s" % (walk, H, W, "ran" if ran else "did not run")
            if ran:
                assert plan.interior_tiles == R.B * interior and plan.interior_tiles + plan.border_tiles == R.B * plan.tiles_y * plan.tiles_x
                assert plan.border_walks == (0 if walk == -2 else 1)
            if first is None:
                first = y
            else:
                assert_same_bits(y, first, "AMS_FB_WALK=%s against unset at %d x %d, pixel scale %g" % (walk, H, W, ps))


def test_blocks_that_really_walk(lib, wd, bars, knobs):
    """B = 16 at 200 x 400 (3.8 MB of frames): 121 interior and 48 border tiles per frame, more than the device holds blocks of either walking
    kernel, so blocks take a second and third tile (prefetch, buffer swap, hand-over across a frame boundary).  The plan has to say so: this test
    fails, it does not skip, on a launch in which no block walks."""
    Bn, H, W = R.WALK_CASE
    knobs(AMS_FB_WALK=None)
    run = Runner(lib, wd, Bn, H, W, S.PIXEL_SCALE)
    keep, fr = device_frames(R.frames(Bn, H, W, "bytes"))
    y, plan = run.form(fr, 2)
    print("\nfirst_block_walk_plan: interior %d tiles on %d blocks, border %d tiles on %d blocks (walking border kernel: %d)"
          % (plan.interior_tiles, plan.interior_grid, plan.border_tiles, plan.border_grid, plan.border_walks))
    assert (plan.interior_tiles, plan.border_tiles, plan.border_walks) == (Bn * 121, Bn * 48, 1)
    assert plan.interior_grid < plan.interior_tiles, "no block of the interior launch took a second tile: %d tiles on %d blocks" % (plan.interior_tiles, plan.interior_grid)
    assert plan.border_grid < plan.border_tiles, "no block of the border launch took a second tile: %d tiles on %d blocks" % (plan.border_tiles, plan.border_grid)
    held(y, R.reference(Bn, H, W, "bytes", S.PIXEL_SCALE), bars["split"], "form=2 frames=uint8 walking %dx%dx%d" % (Bn, H, W))
    for walk in (0, 1):
        knobs(AMS_FB_WALK=walk)
        y2, plan2 = run.form(fr, 2)
        assert plan2.interior_grid == (0 if walk == 0 else plan2.interior_tiles)
        assert_same_bits(y2, y, "AMS_FB_WALK=%d against unset" % walk)
