"""Range of the default product form (AMS_MATMUL_SPLIT_F16) on every layer that has fp16 panels and on the plans that ship.

A layer scaled by a power of two 2^k with its BN compensating (weights x 2^k, moving_mean x 2^k, gamma x 2^-k: the fold gives fscale 2^-k and the
same fshift, exactly) computes the same function: nothing is rounded differently.  logits/semantic has no BN: its weights and biases scale
and the logits come out x 2^k.  So ONE f64 oracle forward of the unscaled weights per geometry is the reference of every scaled case.

  a. f32 and bf16-part products scale exactly: in every mode but SPLIT_F16 a scaled network gives the same bits.
  b. a layer with a weight beyond 65504 leaves the fp16 form (three bf16 parts) and the network stays at the f32 level; at 256 x 512 with
     AMS_OPT_STREAM_MIN_ROWS = 0 the stride-16 blocks hand their input over as ready-made parts, and the hand-over must follow the consumer.
  c. a layer whose weights all lie far below 1 (fp16 parts subnormal, tests/test_f16_split_cpu.py) leaves the fp16 form too.
  d. the boundaries of the check; e. re-freezing moves layers on and off the fp16 form without leftovers.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ams_amd import hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine

pytestmark = pytest.mark.gpu

CI = [0, 1, 2, 10, 11, 13]
SPEC = S.build_spec()
LOGITS = "logits/semantic"
BIG, SMALL = 20, -24                       # 2^20: weights ~ 1e5 > 65504; 2^-24: weights ~ 4e-8, every fp16 part subnormal


def _scopes_with_f16_panels():
    """the layers that hold fp16 panels (engine_plan.hip: whf_mem): the stem, every expand and project, aspp0, concat_projection, logits"""
    out = []
    for l in SPEC.layers:
        if l.scope == "MobilenetV2/Conv" or l.scope.endswith("/expand") or l.scope.endswith("/project") or \
                l.scope in ("aspp0", "concat_projection", LOGITS):
            out.append(l.scope)
    return out


F16_SCOPES = _scopes_with_f16_panels()
IDX = {l.scope: l.idx for l in SPEC.layers}


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)


def scaled(W, ks):
    """W with each scope of ``ks`` scaled by 2^k and its BN compensating (the same function, exactly); logits x 2^k for logits/semantic"""
    W = dict(W)
    for scope, k in ks.items():
        f = np.float32(2.0 ** k)
        wn = [n for n in (scope + "/weights:0", scope + "/depthwise_weights:0") if n in W][0]
        W[wn] = W[wn] * f
        if scope == LOGITS:
            W[scope + "/biases:0"] = W[scope + "/biases:0"] * f
        else:
            W[scope + "/BatchNorm/moving_mean:0"] = W[scope + "/BatchNorm/moving_mean:0"] * f
            W[scope + "/BatchNorm/gamma:0"] = W[scope + "/BatchNorm/gamma:0"] * np.float32(2.0 ** -k)
    return W


class Geometry:
    """frames and the f64 oracle of the unscaled weights at one size (computed once)"""

    def __init__(self, W0, H, B, seed=3):
        from oracle.student_torch import StudentOracle
        self.H, self.B = H, B
        self.frames, _ = synth.SyntheticVideo(H, B, CI, seed=seed).clip()
        o = StudentOracle(W0, CI, dtype=torch.float64)
        self.taps = {}
        with torch.no_grad():
            fr = self.frames.astype(np.float32)
            self.low = o.forward_lowres(fr, "frozen", taps=self.taps).numpy()
            self.full = o.reduced_logits(o.logits_full(fr, "frozen")).numpy()
        self.proj = self.taps["concat_projection"].numpy()      # the logits layer's input, for oracles that change only that layer
        self.bar = None


def engine(geo, W, mode=hip.MATMUL_SPLIT_F16, stream_min_rows=None, max_batch=None):
    eng = StudentEngine(CI, geo.H, 2 * geo.H, max_batch=max_batch or geo.B, trainable=False)
    if stream_min_rows is not None:
        hip.check(eng.lib.ams_student_set_option(eng._h, hip.OPT_STREAM_MIN_ROWS, stream_min_rows))
    eng.set_matmul_mode(mode)
    eng.load_variables(W)
    eng.freeze()
    return eng


def refreeze(eng, W):
    eng.load_variables(W)
    eng.freeze()
    n = C.c_int32()
    hip.check(eng.lib.ams_student_f16_fallback_layers(eng._h, C.byref(n)))
    return n.value


def run(eng, frames):
    """label maps and low-res logits (19 classes) of one frozen call"""
    B = len(frames)
    lab = eng.predict(frames).cpu().numpy()
    h, w = eng.lowres
    return lab, eng.logits_lowres.view(-1, h, w, 32)[:B, :, :, :19].cpu().numpy().copy()


def check_labels(got, oracle_logits_sel, tol):
    """the rule of test_gpu_network.py: labels equal the oracle's argmax wherever its top-2 margin exceeds ``tol``"""
    want = np.argmax(oracle_logits_sel, axis=-1)
    srt = np.sort(oracle_logits_sel, axis=-1)
    margin = srt[..., -1] - srt[..., -2]
    bad = got != want
    assert not np.any(bad & (margin > tol)), "label mismatch on a pixel with margin %g" % margin[bad].max()


def check_against_oracle(geo, lab, low, bar, what):
    assert np.isfinite(low).all(), what + ": non-finite logits"
    err = rel(low, geo.low)
    print("%s: low-res logits vs the f64 oracle %.3e (bar %.1e)" % (what, err, bar))
    assert err < bar, "%s: low-res logits rel err %g against f64 (bar %g)" % (what, err, bar)
    check_labels(lab, geo.full, tol=2e-3 * np.abs(geo.low).max())
    return err


# ---- the profile hook: which kernel computed which layer --------------------------------------------------------------------------------
def profile(eng, frames):
    hip.check(eng.lib.ams_student_profile(eng._h, 1))
    try:
        eng.predict(frames)
        need = C.c_size_t(0)
        hip.check(eng.lib.ams_student_profile_read(eng._h, None, 0, C.byref(need)))
        buf = C.create_string_buffer(need.value + 16)
        hip.check(eng.lib.ams_student_profile_read(eng._h, buf, len(buf), C.byref(need)))
    finally:
        hip.check(eng.lib.ams_student_profile(eng._h, 0))
    rows = []
    for line in buf.value.decode().splitlines():
        name, layer = line.split("\t")[:2]
        rows.append((name, int(layer)))
    return rows


def _targs(name):
    base, _, rest = name.partition("<")
    return base, [a.strip() for a in rest.rstrip(">").split(",")] if rest else []


def runs_f16(name):
    """the launch multiplies on fp16 parts"""
    base, a = _targs(name)
    if base.startswith("pw_gemm_f16"):
        return True
    pos = {"xdw_stream_kernel": 8, "xdw_wreg_kernel": 5, "block_kernel": 7, "first_block_kernel": 2}.get(base)
    return pos is not None and len(a) > pos and a[pos] == "true"


def takes_parts(name):
    """a stride-16 expand+depthwise launch that reads its operand as pre-split parts (the project GEMM before it wrote them)"""
    base, a = _targs(name)
    return base == "xdw_wreg_kernel" or (base == "xdw_stream_kernel" and a[5] == "true")


def covering(rows, scope):
    """the launches that compute the products of layer ``scope`` (a fused kernel is profiled under its last layer)"""
    i = IDX[scope]
    out = [n for n, l in rows if l == i and not n.startswith(("dw3x3", "col_reduce", "upsample", "global_mean", "pw_small"))]
    if scope == "MobilenetV2/Conv" or scope == "MobilenetV2/expanded_conv/project":
        out += [n for n, l in rows if l == 3 and n.startswith("first_block")]
    if scope.endswith("/expand"):
        out += [n for n, l in rows if l == i + 1 and n.startswith(("xdw_", "expand_dw"))]
        out += [n for n, l in rows if l == i + 2 and n.startswith("block_kernel")]
    if scope.endswith("/project"):
        out += [n for n, l in rows if l == i and n.startswith("block_kernel")]
    return out


# blocks 8-16: the project GEMM before each runs at stride 16 (block 7 takes the output of a stride-2 block)
STRIDE16_EXPANDS = ["MobilenetV2/expanded_conv_%d/expand" % b for b in range(8, 17)]


def check_path(rows, fallen):
    """the plan ran the hand-over the test means to cover: stride-16 blocks on pre-split parts; the fallen-back layers on no fp16 product;
    a neighbour of each still on fp16"""
    for scope in fallen:
        cov = covering(rows, scope)
        assert cov, "no launch found for %s" % scope
        assert not any(runs_f16(n) for n in cov), "%s fell back but ran %s" % (scope, cov)
    pre = [s for s in STRIDE16_EXPANDS if any(takes_parts(n) for n in covering(rows, s))]
    fallen_idx = {IDX[s] for s in fallen}
    # every stride-16 block whose expand layer and the project before it kept the fp16 form streamed on parts
    for s in STRIDE16_EXPANDS:
        if IDX[s] not in fallen_idx and IDX[s] - 1 not in fallen_idx:
            assert s in pre, "%s did not stream on pre-split parts: %s" % (s, covering(rows, s))
    for scope in fallen:
        i = F16_SCOPES.index(scope)
        near = [t for t in F16_SCOPES[max(0, i - 3):i + 4] if t not in fallen and not set(covering(rows, t)) & set(covering(rows, scope))]
        assert any(runs_f16(n) for t in near for n in covering(rows, t)), "no neighbour of %s on the fp16 form" % scope


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(SPEC, seed=0)


@pytest.fixture(scope="module")
def g64(W0):
    return Geometry(W0, 64, 2)


@pytest.fixture(scope="module")
def g256(W0):
    """the streaming geometry: 256 x 512, stride-16 GEMMs of 1024 rows write parts (AMS_OPT_STREAM_MIN_ROWS = 0)"""
    geo = Geometry(W0, 256, 2)
    geo.eng = engine(geo, W0, stream_min_rows=0)
    geo.lab0, geo.low0 = run(geo.eng, geo.frames)
    err = check_against_oracle(geo, geo.lab0, geo.low0, 1e-4, "256x512 in range")
    geo.bar = 2 * err                    # a fallen-back layer runs three bf16 parts: the same f32 level as the fp16 form
    assert geo.bar <= 2e-4
    rows = profile(geo.eng, geo.frames)
    check_path(rows, [])
    yield geo
    geo.eng.close()


@pytest.fixture(scope="module")
def g512(W0):
    geo = Geometry(W0, 512, 2, seed=1)
    geo.bar = 5e-5                       # the in-range default plan's bar against f64 (test_gpu_fullsize.py)
    geo.eng = engine(geo, W0)
    yield geo
    geo.eng.close()


def test_power_of_two_scaling_keeps_the_function_in_f64(W0, g64):
    """the premise: the f64 oracle of a scaled weight set is the oracle of W0"""
    from oracle.student_torch import StudentOracle
    ks = {l.scope: (13 if j % 2 else -11) for j, l in enumerate(l for l in SPEC.layers)}
    o = StudentOracle(scaled(W0, ks), CI, dtype=torch.float64)
    with torch.no_grad():
        low = o.forward_lowres(g64.frames.astype(np.float32), "frozen").numpy()
    assert rel(low * 2.0 ** -ks[LOGITS], g64.low) < 1e-12


@pytest.mark.parametrize("H,stream_min_rows", [(64, None), (256, 0), (512, None)])
@pytest.mark.parametrize("mode", [hip.MATMUL_F32, hip.MATMUL_SPLIT_BF16_X6, hip.MATMUL_SPLIT_BF16, hip.MATMUL_BF16])
def test_power_of_two_scaling_is_bit_exact(W0, H, stream_min_rows, mode):
    """every BN layer and the logits layer at once, k alternating +13 / -11: the same label maps and the same logits (x 2^-k) bit for bit"""
    B = 2
    frames, _ = synth.SyntheticVideo(H, B, CI, seed=3).clip()
    ks = {l.scope: (13 if j % 2 else -11) for j, l in enumerate(SPEC.layers)}
    eng = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=False)
    if stream_min_rows is not None:
        hip.check(eng.lib.ams_student_set_option(eng._h, hip.OPT_STREAM_MIN_ROWS, stream_min_rows))
    eng.set_matmul_mode(mode)
    try:
        assert refreeze(eng, W0) == 0
        lab0, low0 = run(eng, frames)
        refreeze(eng, scaled(W0, ks))
        lab1, low1 = run(eng, frames)
    finally:
        eng.close()
    assert np.array_equal(lab1, lab0)
    assert np.array_equal(low1 * np.float32(2.0 ** -ks[LOGITS]), low0)


@pytest.mark.parametrize("scope", F16_SCOPES)
def test_each_layer_beyond_fp16_range_falls_back(g256, W0, scope):
    """256 x 512, SPLIT_F16: one layer x 2^20 (weights ~ 1e5) leaves the fp16 form; the network stays at the f32 level and the plan
    still hands parts over between the stride-16 blocks — in the consumer's format"""
    W = scaled(W0, {scope: BIG})
    assert refreeze(g256.eng, W) == 1
    lab, low = run(g256.eng, g256.frames)
    if scope == LOGITS:
        low = low * np.float32(2.0 ** -BIG)
    check_against_oracle(g256, lab, low, g256.bar, scope + " x 2^20")
    check_path(profile(g256.eng, g256.frames), [scope])


@pytest.mark.parametrize("scopes", [["MobilenetV2/expanded_conv_9/expand", "MobilenetV2/expanded_conv_9/project"],
                                    ["MobilenetV2/expanded_conv_14/expand", "MobilenetV2/expanded_conv_14/project"],
                                    ["MobilenetV2/expanded_conv_10/project", "MobilenetV2/expanded_conv_11/expand"],
                                    ["MobilenetV2/expanded_conv_13/project", "MobilenetV2/expanded_conv_14/expand"]])
def test_neighbouring_layers_beyond_fp16_range_fall_back(g256, W0, scopes):
    W = scaled(W0, {s: BIG for s in scopes})
    assert refreeze(g256.eng, W) == len(scopes)
    lab, low = run(g256.eng, g256.frames)
    check_against_oracle(g256, lab, low, g256.bar, " + ".join(scopes) + " x 2^20")
    check_path(profile(g256.eng, g256.frames), scopes)


@pytest.mark.parametrize("scope", ["MobilenetV2/expanded_conv_2/expand",          # whole-block kernel
                                   "MobilenetV2/expanded_conv_7/expand",          # streamed (Cin 64)
                                   "MobilenetV2/expanded_conv_16/expand",         # weight-register kernel (Cin 160)
                                   "MobilenetV2/expanded_conv_10/project",        # feeds a streamed block
                                   "concat_projection", LOGITS])
def test_each_layer_below_fp16_normal_range_falls_back(g256, W0, scope):
    """one layer x 2^-24 (weights ~ 4e-8: hi = 0, lo subnormal) leaves the fp16 form: the network stays at the f32 level"""
    W = scaled(W0, {scope: SMALL})
    assert refreeze(g256.eng, W) == 1
    lab, low = run(g256.eng, g256.frames)
    if scope == LOGITS:
        low = low * np.float32(2.0 ** -SMALL)
    check_against_oracle(g256, lab, low, g256.bar, scope + " x 2^-24")
    check_path(profile(g256.eng, g256.frames), [scope])


@pytest.mark.parametrize("scope", ["MobilenetV2/Conv", "MobilenetV2/expanded_conv_2/expand", "MobilenetV2/expanded_conv_7/expand",
                                   "MobilenetV2/expanded_conv_13/project", "MobilenetV2/expanded_conv_15/expand", "aspp0"])
def test_layer_beyond_fp16_range_full_size(g512, W0, scope):
    """512 x 1024, two frames, default options: a fallen-back layer keeps the in-range plan's bar against f64"""
    assert refreeze(g512.eng, scaled(W0, {scope: BIG})) == 1
    lab, low = run(g512.eng, g512.frames)
    check_against_oracle(g512, lab, low, g512.bar, "512x1024 " + scope + " x 2^20")


def test_layer_beyond_fp16_range_full_size_late_subbatches(g512, W0):
    """512 x 1024, four frames in late sub-batches of two (each offsets into the part planes); frames a b b a, so a sub-batch that read
    the other's parts would give the wrong frame"""
    scope = "MobilenetV2/expanded_conv_15/expand"
    fr = np.concatenate([g512.frames, g512.frames[::-1]])
    eng = engine(g512, scaled(W0, {scope: BIG}), max_batch=4)
    try:
        eng.set_dual_stream(0)
        eng.set_late_subbatch(2)
        n = C.c_int32()
        hip.check(eng.lib.ams_student_f16_fallback_layers(eng._h, C.byref(n)))
        assert n.value == 1
        lab, low = run(eng, fr)
        rows = profile(eng, fr)
    finally:
        eng.close()
    assert sum(1 for n_, l in rows if l == IDX["aspp0"] and n_.startswith("pw_gemm")) == 2          # the late section ran twice
    want = np.concatenate([g512.low, g512.low[::-1]])
    full = np.concatenate([g512.full, g512.full[::-1]])
    assert np.isfinite(low).all()
    err = rel(low, want)
    print("512x1024 B=4 late sub-batches, %s x 2^20: %.3e" % (scope, err))
    assert err < g512.bar
    check_labels(lab, full, tol=2e-3 * np.abs(want).max())


def test_fp16_range_check_boundaries(W0, g64):
    """logits/semantic (no later fp16 operand sees its values): one weight set to the edge of the range, against the f64 oracle of that
    weight set (the logits layer's input is the same: a product in f64)"""
    name = LOGITS + "/weights:0"
    eng = engine(g64, W0)
    try:
        def case(value, fallbacks, compare=True, scale=None):
            W = dict(W0)
            w = np.array(W0[name], copy=True)
            if scale is not None:
                w = (w * np.float32(scale / np.abs(w).max())).astype(np.float32)
                np.clip(w, -scale, scale, out=w)
            flat = w.reshape(-1)
            j = int(np.argmax(np.abs(flat)))
            flat[j] = np.float32(value)
            W[name] = w
            assert refreeze(eng, W) == fallbacks, (value, scale)
            if not compare:
                return
            lab, low = run(eng, g64.frames)
            want = np.einsum("bhwc,ck->bhwk", g64.proj, w.reshape(w.shape[-2], w.shape[-1]).astype(np.float64)) + W[LOGITS + "/biases:0"]
            assert np.isfinite(low).all()
            err = rel(low, want)
            print("64x128 logits weight %r: %.3e" % (value, err))
            assert err < 2e-4
        case(65504.0, 0)
        case(65520.0, 1)
        case(-65520.0, 1)
        case(np.nan, 1, compare=False)
        case(np.inf, 1, compare=False)
        # the small side: the largest |w| exactly 2^-10 keeps the fp16 form, one f32 step below it does not
        case(2.0 ** -10, 0, scale=2.0 ** -10)
        case(-(2.0 ** -10), 0, scale=2.0 ** -10)
        case(np.nextafter(np.float32(2.0 ** -10), np.float32(0)), 1, scale=float(np.nextafter(np.float32(2.0 ** -10), np.float32(0))))
        assert refreeze(eng, W0) == 0
    finally:
        eng.close()


def test_refreeze_moves_layers_on_and_off_the_fp16_form(g256, W0):
    """at the streaming geometry, one engine frozen in range, beyond it, below it and in range again gives in each state the bits of a
    fresh engine frozen in that state"""
    states = [(W0, 0), (scaled(W0, {"MobilenetV2/expanded_conv_14/expand": BIG, "aspp0": BIG}), 2),
              (scaled(W0, {"MobilenetV2/expanded_conv_8/expand": SMALL}), 1), (W0, 0)]
    eng = engine(g256, W0, stream_min_rows=0)
    try:
        for W, nfb in states:
            assert refreeze(eng, W) == nfb
            lab, low = run(eng, g256.frames)
            fresh = engine(g256, W, stream_min_rows=0)
            try:
                lab_f, low_f = run(fresh, g256.frames)
            finally:
                fresh.close()
            assert np.array_equal(lab, lab_f) and np.array_equal(low, low_f)
    finally:
        eng.close()
