"""The corners of the domains the GEMM, depthwise / stem and recompute entries accept (include/ams_hip.h), each against plain NumPy / torch f64
of the same operation: the smallest and largest channel counts, the fewest rows and columns, every instantiation a launcher can pick.
tests/test_gpu_kernels.py runs the shapes of the network and the edges of the tiles; tests/test_train_entry_refusals_cpu.py holds what lies
outside the domains.  Every case here lies inside: no refused argument reaches the GPU.

Buffers as in tests/test_gpu_kernels.py (tests/kernel_suite.py, tests/guarded.py): results inside poisoned guards, operands between guards,
scratch and panels of exactly the stated size and poisoned, `run()` after every call.

Bars: the ones each family has in tests/test_gpu_kernels.py, under the same measure (rel_err: the largest error over the largest |reference|):
2e-5 the f32 GEMM, the sums and the partial rows; 5e-5 the two-part bf16 GEMM; 2e-5 the three-part one (all 24 significand bits: the f32 GEMM's
bar); 3e-5 the weight gradients; 2e-6 the fp16 form; 1e-5 the depthwise tensors and the stem; bit for bit what is bit for bit there.
rel_err divides by the largest |reference value|, which a result of a handful of elements can have near zero by chance: every case draws its
operands (N(0, 1)-scaled as there) from the first seed, counted up from one fixed by its shape, at which each f64 reference ALONE reaches 0.25
(first_seed: nothing of the GPU result enters), and asserts that (scaled) in front of its first GPU call.  The one exception is
ams_k_pointwise_wgrad_split, whose results have 4096 elements and more and whose operands are scaled as in its existing test (dy by 1e-3)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded as G
from ams_amd import hip, spec as S
from kernel_suite import (P, PD, _guarded_buffers, dev, dw_wgrad_scratch, f16_parts, frames, gemm_guard, h2i_pack, image_guard, lib, out,  # noqa: F401
                          rel_err, run, scratch, stream, wgrad_f32_scratch, wgrad_x6_scratch)
from test_gpu_kernels import recompute_block_kernels

pytestmark = pytest.mark.gpu

FLOOR = 0.25
f32, f64 = np.float32, np.float64


def first_seed(base, make):
    """make(rng) -> (operands, {name: f64 reference}): those of the first seed from `base` on at which every reference reaches FLOOR"""
    for seed in range(base, base + 256):
        ops, want = make(np.random.default_rng(seed))
        if all(np.abs(w).max() >= FLOOR for w in want.values()):
            return ops, want
    raise AssertionError("no seed in %d .. %d at which every f64 reference reaches %g" % (base, base + 255, FLOOR))


def scaled(want):
    """in front of the first GPU call: no reference is near zero throughout"""
    for name, w in want.items():
        assert np.abs(w).max() >= FLOOR, "%s: the largest |reference| is %g" % (name, np.abs(w).max())


# ------------------------------------------------------------------------------------------------ pointwise
def gemm_case(M, K, N, base, x_like_act=False, f16_edges=False):
    def make(rng):
        x = (np.clip(rng.standard_normal((M, K)) * 2 + 1, 0, 6) if x_like_act else rng.standard_normal((M, K))).astype(f32)
        if f16_edges:
            x[0, :8] = [0.0, 6.0, 1e-7, 3e-5, 6.1e-5, 1.0, 0.333333, 5.9999995]          # fp16 subnormal / boundary values of hi and lo
        w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(f32)
        scale = rng.uniform(0.5, 1.5, N).astype(f32)
        shift = rng.standard_normal(N).astype(f32)
        res = rng.standard_normal((M, N)).astype(f32)
        prod = x.astype(f64) @ w.astype(f64)
        return (x, w, scale, shift, res), dict(plain=prod, relu6_res=np.clip(prod * scale + shift, 0, 6) + res, affine=prod * scale + shift,
                                               affine_res=prod * scale + shift + res)
    return first_seed(base, make)


@pytest.mark.parametrize("trans", [0, 1], ids=["w_kn", "w_nk"])
@pytest.mark.parametrize("K,N", [(4, 1), (4, 3), (12, 5), (8, 16), (4, 19)])
@pytest.mark.parametrize("M", [1, 17, 65])
def test_pointwise_at_its_smallest_k_and_n(lib, M, K, N, trans):
    """ams_k_pointwise accepts K % 4 == 0 and any N >= 1: one, two and three 4-wide k groups of a single 16-wide chunk (the other lanes of the chunk
    load nothing), one column, odd column counts, a full vector tile; one row (pw_small_m_kernel), 17 and 65 (the tiled kernel: a short block, a
    second block of one row); both weight orientations; with the whole epilogue and without."""
    (x, w, scale, shift, res), want = gemm_case(M, K, N, 1000 * M + 10 * K + N)
    scaled(want)
    xd, wd = dev(x), dev(np.ascontiguousarray(w.T) if trans else w)
    y = out((M, N), guard=gemm_guard(N))
    run(lib.ams_k_pointwise(P(xd), M, K, P(wd), N, trans, None, 1, PD(scale), PD(shift), hip.ACT_RELU6, PD(res), P(y), stream()), "pointwise")
    assert rel_err(y.cpu().numpy(), want["relu6_res"]) < 2e-5
    y = out((M, N), guard=gemm_guard(N))
    run(lib.ams_k_pointwise(P(xd), M, K, P(wd), N, trans, None, 1, None, None, hip.ACT_NONE, None, P(y), stream()), "pointwise, plain")
    assert rel_err(y.cpu().numpy(), want["plain"]) < 2e-5


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("K,N", [(8, 1), (8, 3), (16, 5), (24, 16), (24, 19)])
@pytest.mark.parametrize("M", [17, 65, 257])
def test_pointwise_split_below_one_stage(lib, parts, M, K, N):
    """ams_k_pointwise_split / _split3 accept K % 8 == 0: K = 8, 16, 24 are one stage of Kp = 32 of which 24, 16, 8 columns are the split kernel's
    zero padding (the operand loads beyond K repeat the row's last 8 values against them); N from one column on.  Panels: exactly 2 or 3 planes
    of N * 32, poisoned."""
    (x, w, scale, shift, res), want = gemm_case(M, K, N, 1000 * M + 10 * K + N + parts)
    scaled(want)
    entry, bar = (lib.ams_k_pointwise_split, 5e-5) if parts == 2 else (lib.ams_k_pointwise_split3, 2e-5)
    xd, wd = dev(x), dev(w)
    panels = scratch(parts * N * 32, torch.int16)
    y = out((M, N), guard=gemm_guard(N))
    run(entry(P(xd), M, K, P(wd), N, PD(scale), PD(shift), hip.ACT_RELU6, PD(res), P(y), P(panels), panels.numel(), stream()), "pointwise_split%d" % parts)
    assert rel_err(y.cpu().numpy(), want["relu6_res"]) < bar
    panels = scratch(parts * N * 32, torch.int16)
    y = out((M, N), guard=gemm_guard(N))
    run(entry(P(xd), M, K, P(wd), N, None, None, hip.ACT_NONE, None, P(y), P(panels), panels.numel(), stream()), "pointwise_split%d, plain" % parts)
    assert rel_err(y.cpu().numpy(), want["plain"]) < bar


@pytest.mark.parametrize("M,K,N", [(m, k, n) for m in (1, 17, 65) for (k, n) in ((32, 1), (32, 3), (40, 5))] + [(17, 32, 16), (65, 40, 24)])
def test_pointwise_split_f16_at_its_fewest_columns(lib, M, K, N):
    """ams_k_pointwise_split_f16 accepts K >= 32, K % 8 == 0 and any N >= 1: one, three and five columns (scalar epilogue) at the smallest K and at
    Kp = 64 with 24 pad columns; N = 16 and 24 (vector epilogue) keep the part planes beside them.  As in test_pointwise_split_f16: f64 to 2e-6,
    the operand packed first gives the same bits (and the packed operand is the host's), the part planes are the host's split of the result."""
    res = (M + N) % 2 == 1
    (x, w, scale, shift, r), want = gemm_case(M, K, N, 1000 * M + 10 * K + N, x_like_act=res, f16_edges=True)
    scaled(want)
    ref = want["affine_res"] if res else want["affine"]
    Kp = (K + 31) // 32 * 32
    vec = N % 4 == 0
    xd, wd, sd, hd, rd = dev(x), dev(w), dev(scale), dev(shift), dev(r) if res else None
    y = out((M, N), guard=gemm_guard(N))
    parts = out((2, M, N), torch.int16, guard=gemm_guard(N)) if vec else None
    panels = scratch(2 * N * Kp, torch.int16)
    run(lib.ams_k_pointwise_split_f16(P(xd), M, K, P(wd), N, P(sd), P(hd), hip.ACT_NONE, P(rd), P(y), P(panels), panels.numel(), None, P(parts),
                                      stream()), "pointwise_split_f16")
    got = y.cpu().numpy()
    assert rel_err(got, ref) < 2e-6
    if vec:
        hi, lo = f16_parts(got)
        pp = parts.cpu().numpy().view(np.uint16)
        assert np.array_equal(pp[0], hi.view(np.uint16)) and np.array_equal(pp[1], lo.view(np.uint16))
    xh = out((M, K), guard=gemm_guard(K))
    y2 = out((M, N), guard=gemm_guard(N))
    panels = scratch(2 * N * Kp, torch.int16)
    run(lib.ams_k_pointwise_split_f16(P(xd), M, K, P(wd), N, P(sd), P(hd), hip.ACT_NONE, P(rd), P(y2), P(panels), panels.numel(), P(xh), None,
                                      stream()), "pointwise_split_f16 from fp16 pairs")
    assert np.array_equal(xh.cpu().numpy().view(np.uint16).reshape(M, K // 8, 2, 8), h2i_pack(x))
    assert torch.equal(y2, y)


@pytest.mark.parametrize("M,Cn", [(1, 8), (3, 8), (65, 24)])
def test_pack_h2i(lib, M, Cn):
    """ams_k_pack_h2i on its own: one thread per 8 channels — one thread in all, three, and 195 (a second block of 256 would start at 257);
    bit for bit the host's packing, fp16 subnormal and boundary values of hi and lo included."""
    rng = np.random.default_rng(M + Cn)
    x = (rng.standard_normal((M, Cn)) * 2).astype(f32)
    x[0, :8] = [0.0, 6.0, 1e-7, 3e-5, 6.1e-5, 1.0, 0.333333, 5.9999995]
    o = out((M, Cn))
    run(lib.ams_k_pack_h2i(PD(x), M, Cn, P(o), stream()), "pack_h2i")
    assert np.array_equal(o.cpu().numpy().view(np.uint16).reshape(M, Cn // 8, 2, 8), h2i_pack(x))


# launch_pointwise_wgrad picks pw_wgrad_f32<VA, VB>: V = 1 up to 16 channels, at most 2 up to 32, else the widest of 4 / 2 / 1 that divides the
# count — one shape per instantiation
WGRAD_FORMS = {"<4, 4>": (40, 48), "<4, 2>": (40, 24), "<4, 1>": (40, 5), "<2, 4>": (24, 48), "<2, 2>": (24, 24), "<2, 1>": (24, 5),
               "<1, 4>": (5, 48), "<1, 2>": (5, 24), "<1, 1>": (5, 7)}
WGRAD_CASES = [pytest.param(m, k, n, id="%s-K%d-N%d-M%d" % (form, k, n, m)) for form, (k, n) in WGRAD_FORMS.items() for m in (1, 3, 260)] + \
              [pytest.param(65, k, n, id="<1, 1>-K%d-N%d-M65" % (k, n)) for (k, n) in ((1, 1), (2, 3), (3, 2), (5, 7))]


@pytest.mark.parametrize("M,K,N", WGRAD_CASES)
def test_pointwise_wgrad_in_every_instantiation(lib, M, K, N):
    """All nine <VA, VB> forms of the exact-f32 weight gradient, each at one row (every pixel slot but one is the clamped last row, selected to
    zero), three, and 260 (two row splits, of 132 and of 128 rows); and channel counts below 16 that are odd or tiny, down to one channel on
    either side.  Scratch: exactly the entry's own floats, poisoned; a second run gives the same bits."""
    def make(rng):
        x = rng.standard_normal((M, K)).astype(f32)
        dy = rng.standard_normal((M, N)).astype(f32)
        return (x, dy), dict(dw=x.astype(f64).T @ dy.astype(f64))
    (x, dy), want = first_seed(M * 3 + K + N, make)
    scaled(want)
    n_scr = wgrad_f32_scratch(M, K, N)
    xd, dyd = dev(x), dev(dy)
    scr = scratch(n_scr)
    dw = out((K, N))
    run(lib.ams_k_pointwise_wgrad(P(xd), P(dyd), M, K, N, P(dw), P(scr), n_scr, stream()), "pointwise_wgrad")
    assert rel_err(dw.cpu().numpy(), want["dw"]) < 3e-5
    dw2 = out((K, N))
    scr = scratch(n_scr)
    run(lib.ams_k_pointwise_wgrad(P(xd), P(dyd), M, K, N, P(dw2), P(scr), n_scr, stream()), "pointwise_wgrad again")
    assert torch.equal(dw, dw2)


@pytest.mark.parametrize("M,K,N", [(1024, 4, 1024), (1024, 1024, 4), (1024, 8, 512)])
def test_pointwise_wgrad_split_at_its_smallest_corners(lib, M, K, N):
    """The smallest M, and the smallest K and N (one float4 of a 64-channel tile side; the rest is clamped and selected to zero) at which
    K * N >= 4096 still holds.  The rule of test_pointwise_wgrad_split: f64 to 3e-5, no worse than twice the exact-f32 kernel, same bits twice."""
    rng = np.random.default_rng(M + K + N)
    x = (rng.standard_normal((M, K)) * rng.uniform(0.1, 4.0, (1, K))).astype(f32)
    dy = (rng.standard_normal((M, N)) * 1e-3).astype(f32)
    want = x.astype(f64).T @ dy.astype(f64)
    n_scr, n_f32 = wgrad_x6_scratch(M, K, N), wgrad_f32_scratch(M, K, N)
    assert lib.ams_k_pointwise_wgrad_scratch(M, K, N) == max(n_scr, n_f32)
    xd, dyd = dev(x), dev(dy)
    scr = scratch(n_scr)
    dw = out((K, N))
    run(lib.ams_k_pointwise_wgrad_split(P(xd), P(dyd), M, K, N, P(dw), P(scr), n_scr, stream()), "pointwise_wgrad_split")
    got = dw.cpu().numpy()
    assert rel_err(got, want) < 3e-5
    exact = out((K, N))
    scr = scratch(n_f32)
    run(lib.ams_k_pointwise_wgrad(P(xd), P(dyd), M, K, N, P(exact), P(scr), n_f32, stream()), "pointwise_wgrad")
    assert rel_err(got, want) <= 2 * rel_err(exact.cpu().numpy(), want) + 1e-6
    dw2 = out((K, N))
    scr = scratch(n_scr)
    run(lib.ams_k_pointwise_wgrad_split(P(xd), P(dyd), M, K, N, P(dw2), P(scr), n_scr, stream()), "pointwise_wgrad_split again")
    assert torch.equal(dw, dw2)


# ------------------------------------------------------------------------------------------------ depthwise
# C = 4, 8, 12: CG = C / 4 = 1, 2, 3 channel groups — 256, 128 and 85 column slots of a tile (at 85 the weight gradient runs 255 threads and the
# walking forms fold column strips that wrap around three groups); C = 1024: one column slot, every thread another group.  Maps 1 x 1 (every
# tap but the centre is padding) and 5 x 7 (two row tiles of four, odd extents in every parity class); C = 1024 on 5 x 7 only.
DW_MAPS = [(H, W, Cn) for Cn in (4, 8, 12) for (H, W) in ((1, 1), (5, 7))] + [(5, 7, 1024)]


def conv_pads(H, W, stride, rate):
    Ho, pt, pb = S.same_pad(H, 3, stride, rate)
    Wo, pl, pr = S.same_pad(W, 3, stride, rate)
    return Ho, Wo, (pl, pr, pt, pb)


def nhwc(t):
    return t.detach().permute(0, 2, 3, 1).numpy()


def per_channel(v):
    return torch.as_tensor(v).double().view(1, -1, 1, 1)


@pytest.mark.parametrize("stride,rate", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("H,W,Cn", DW_MAPS)
def test_depthwise_at_the_ends_of_its_channel_range(lib, H, W, Cn, stride, rate):
    """ams_k_depthwise3x3, _dgrad and _wgrad as in test_depthwise_forward_and_backward (f64 autograd of the padded conv), one frame and two."""
    for B in frames(None, [None], None):
        Ho, Wo, pads = conv_pads(H, W, stride, rate)

        def make(rng):
            x = rng.standard_normal((B, H, W, Cn)).astype(f32)
            w = (rng.standard_normal((3, 3, Cn, 1)) * 0.4).astype(f32)
            scale = rng.uniform(0.5, 1.5, Cn).astype(f32)
            shift = rng.standard_normal(Cn).astype(f32)
            dy = rng.standard_normal((B, Ho, Wo, Cn)).astype(f32)
            xt = torch.as_tensor(x).double().permute(0, 3, 1, 2).requires_grad_(True)
            wt = torch.as_tensor(w).double().permute(2, 3, 0, 1).requires_grad_(True)
            raw = F.conv2d(F.pad(xt, pads), wt, stride=stride, dilation=rate, groups=Cn)
            y = torch.clamp(raw * per_channel(scale) + per_channel(shift), 0, 6)
            raw.backward(torch.as_tensor(dy).double().permute(0, 3, 1, 2))
            return (x, w, scale, shift, dy), dict(y=nhwc(y), raw=nhwc(raw), dx=nhwc(xt.grad), dw=wt.grad.permute(2, 3, 0, 1).numpy())
        (x, w, scale, shift, dy), want = first_seed(H * W + Cn + 100 * B, make)
        scaled(want)
        xd, wd, dyd = dev(x), dev(w), dev(dy)
        y = out((B, Ho, Wo, Cn), guard=image_guard(Wo, Cn))
        run(lib.ams_k_depthwise3x3(P(xd), B, H, W, Cn, P(wd), stride, rate, PD(scale), PD(shift), hip.ACT_RELU6, P(y), stream()), "depthwise3x3")
        assert rel_err(y.cpu().numpy(), want["y"]) < 1e-5
        y = out((B, Ho, Wo, Cn), guard=image_guard(Wo, Cn))
        run(lib.ams_k_depthwise3x3(P(xd), B, H, W, Cn, P(wd), stride, rate, None, None, hip.ACT_NONE, P(y), stream()), "depthwise3x3, raw")
        assert rel_err(y.cpu().numpy(), want["raw"]) < 1e-5
        dx = out((B, H, W, Cn), guard=image_guard(W, Cn))
        run(lib.ams_k_depthwise3x3_dgrad(P(dyd), B, H, W, Cn, P(wd), stride, rate, P(dx), stream()), "depthwise3x3_dgrad")
        assert rel_err(dx.cpu().numpy(), want["dx"]) < 1e-5
        n_scr = dw_wgrad_scratch(B, Ho, Wo, Cn)
        scr = scratch(n_scr)
        dw = out((3, 3, Cn, 1))
        run(lib.ams_k_depthwise3x3_wgrad(P(xd), P(dyd), B, H, W, Cn, stride, rate, P(dw), P(scr), n_scr, stream()), "depthwise3x3_wgrad")
        assert rel_err(dw.cpu().numpy(), want["dw"]) < 2e-5


@pytest.mark.parametrize("rate", [1, 2])
@pytest.mark.parametrize("H,W,Cn", DW_MAPS)
def test_depthwise_fine_tune_forms_at_the_ends_of_their_channel_range(lib, H, W, Cn, rate):
    """The four one-kernel forms with the asserts of test_depthwise_fine_tune_kernels and test_depthwise_backward_with_folded_apply: tensors and
    the sums folded from the partial rows against f64; the reported rows free of poison; the tile form's z_d bit for bit the walking form's; the
    folded apply's gradient bit for bit that of the separate pass (dz_d formed in the pass's own f32 arithmetic) followed by the walking form.
    One frame and two."""
    for B in frames(None, [None], None):
        _, _, pads = conv_pads(H, W, 1, rate)

        def make(rng):
            o = dict(ze=rng.standard_normal((B, H, W, Cn)).astype(f32) * 2.0, w=(rng.standard_normal((3, 3, Cn, 1)) * 0.4).astype(f32),
                     scale=rng.uniform(0.5, 1.5, Cn).astype(f32), shift=rng.standard_normal(Cn).astype(f32),
                     center=(rng.standard_normal(Cn) * 0.1).astype(f32), mean=(rng.standard_normal(Cn) * 0.2).astype(f32),
                     rstd=rng.uniform(0.5, 2.0, Cn).astype(f32), dy_d=rng.standard_normal((B, H, W, Cn)).astype(f32),
                     z_d=rng.standard_normal((B, H, W, Cn)).astype(f32), cA=rng.uniform(0.5, 1.5, Cn).astype(f32),
                     cB=(rng.standard_normal(Cn) * 0.3).astype(f32), cC=(rng.standard_normal(Cn) * 0.3).astype(f32))
            o["dz32"] = ((o["cA"] * o["dy_d"] + o["cB"]) + o["cC"] * o["z_d"]).astype(f32)            # the apply pass's own f32 arithmetic
            dz64 = o["cA"].astype(f64) * o["dy_d"] + o["cB"] + o["cC"].astype(f64) * o["z_d"]
            y = torch.as_tensor(o["ze"]).double().permute(0, 3, 1, 2) * per_channel(o["scale"]) + per_channel(o["shift"])
            mask = nhwc(((y > 0) & (y < 6)).double())
            xhat = (o["ze"].astype(f64) - o["mean"]) * o["rstd"]
            want = {}
            for name, dz in (("walk", o["dz32"].astype(f64)), ("apply", dz64)):       # each backward form against the gradient IT is given
                a_e = torch.clamp(y, 0, 6).detach().requires_grad_(True)
                wt = torch.as_tensor(o["w"]).double().permute(2, 3, 0, 1).requires_grad_(True)
                zd = F.conv2d(F.pad(a_e, pads), wt, dilation=rate, groups=Cn)
                zd.backward(torch.as_tensor(dz).permute(0, 3, 1, 2))
                dy = nhwc(a_e.grad) * mask
                want.update({name + "/dy": dy, name + "/sum": dy.sum(axis=(0, 1, 2)), name + "/sum_xhat": (dy * xhat).sum(axis=(0, 1, 2)),
                             name + "/taps": wt.grad.permute(2, 3, 0, 1).numpy()[..., 0]})
            d = nhwc(zd) - o["center"].astype(f64)
            want.update(zd=nhwc(zd), s1=d.sum(axis=(0, 1, 2)), s2=(d * d).sum(axis=(0, 1, 2)))
            return o, want
        o, want = first_seed(H * W + Cn + rate + 100 * B, make)
        scaled(want)
        d = {k: dev(v) for k, v in o.items()}
        rows = C.c_int32(0)
        size, guard = (B, H, W, Cn), image_guard(W, Cn)

        def forward(entry, n_scr, what):
            scr = scratch(n_scr)
            zd = out(size, guard=guard)
            run(entry(P(d["ze"]), B, H, W, Cn, P(d["w"]), rate, P(d["scale"]), P(d["shift"]), hip.ACT_RELU6, P(d["center"]), P(zd), P(scr), n_scr,
                      C.byref(rows), stream()), what)
            G.no_poison(scr, scr[: rows.value * 2 * Cn], what + "'s partial rows")
            assert rel_err(zd.cpu().numpy(), want["zd"]) < 1e-5, what
            part = scr[: rows.value * 2 * Cn].cpu().numpy().astype(f64).reshape(rows.value, 2, Cn).sum(axis=0)
            assert rel_err(part[0], want["s1"]) < 2e-5 and rel_err(part[1], want["s2"]) < 2e-5, what
            return zd

        def backward(call, n_scr, name, what):
            scr = scratch(n_scr)
            dyo = out(size, guard=guard)
            run(call(dyo, scr, n_scr), what)
            G.no_poison(scr, scr[: rows.value * 11 * Cn], what + "'s partial rows")
            assert rel_err(dyo.cpu().numpy(), want[name + "/dy"]) < 1e-5, what
            part = scr[: rows.value * 11 * Cn].cpu().numpy().astype(f64).reshape(rows.value, 11, Cn).sum(axis=0)
            assert rel_err(part[0], want[name + "/sum"]) < 2e-5 and rel_err(part[1], want[name + "/sum_xhat"]) < 2e-5, what
            assert rel_err(part[2:].reshape(3, 3, Cn), want[name + "/taps"]) < 2e-5, what
            return dyo

        zd_walk = forward(lib.ams_k_depthwise3x3_fwd_bn, lib.ams_k_depthwise3x3_fwd_bn_scratch(B, H, W, Cn, rate), "depthwise3x3_fwd_bn")
        zd_tile = forward(lib.ams_k_depthwise3x3_fwd_bn_tiles, lib.ams_k_depthwise3x3_fwd_bn_tiles_scratch(B, H, W, Cn, rate), "depthwise3x3_fwd_bn_tiles")
        assert torch.equal(zd_tile, zd_walk), "tile-form forward differs from dw3x3_fwd_bn_kernel by %g" % (zd_tile - zd_walk).abs().max().item()
        tail = (P(d["ze"]), P(d["scale"]), P(d["shift"]), hip.ACT_RELU6, P(d["mean"]), P(d["rstd"]))
        dy_walk = backward(lambda dyo, scr, n: lib.ams_k_depthwise3x3_dgrad_bn(P(d["dz32"]), B, H, W, Cn, P(d["w"]), rate, *tail, P(dyo), P(scr), n,
                                                                             C.byref(rows), stream()),
                           lib.ams_k_depthwise3x3_dgrad_bn_scratch(B, H, W, Cn), "walk", "depthwise3x3_dgrad_bn")
        dy_apply = backward(lambda dyo, scr, n: lib.ams_k_depthwise3x3_dgrad_bn_apply(P(d["dy_d"]), P(d["z_d"]), P(d["cA"]), P(d["cB"]), P(d["cC"]), B, H, W,
                                                                                    Cn, P(d["w"]), rate, *tail, P(dyo), P(scr), n, C.byref(rows), stream()),
                            lib.ams_k_depthwise3x3_dgrad_bn_apply_scratch(B, H, W, Cn, rate), "apply", "depthwise3x3_dgrad_bn_apply")
        assert torch.equal(dy_apply, dy_walk), "folded apply differs from the separate pass by %g" % (dy_apply - dy_walk).abs().max().item()


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("H,W,dtype", [(9, 7, np.uint8), (32, 64, np.uint8), (9, 7, np.float32)], ids=["u8-9x7", "u8-32x64", "f32-9x7"])
@pytest.mark.parametrize("cout", [8, 16, 24, 32, 64, 256])
def test_stem_conv_at_every_width(lib, cout, H, W, dtype):
    """ams_k_stem_conv accepts cout % 8 == 0 up to 256; the engine hands it the spec's cout.  Every width but 32 runs stem_conv_kernel (thread =
    pixel x 8 output channels, the weights [27][cout] in dynamic LDS): one group of 8, two, three, eight, and the 32 groups of the largest; 32
    itself (stem_mfma_kernel) on the same frames holds the same reference formula as test_stem_conv.  With BN + ReLU6 and raw (training mode)."""
    B = 2
    Ho, pt, pb = S.same_pad(H + 1, 3, 2, 1)
    Wo, pl, pr = S.same_pad(W + 1, 3, 2, 1)

    def make(rng):
        fr = rng.integers(0, 256, (B, H, W, 3)).astype(dtype)
        if dtype == np.float32:
            fr = fr + rng.random((B, H, W, 3)).astype(f32) * 0.5
        w = (rng.standard_normal((3, 3, 3, cout)) * 0.3).astype(f32)
        scale = rng.uniform(0.5, 1.5, cout).astype(f32)
        shift = rng.standard_normal(cout).astype(f32)
        x = torch.as_tensor(fr.astype(f32)).permute(0, 3, 1, 2)
        x = F.pad(x, (0, 1, 0, 1), value=127.5) * np.float32(S.PIXEL_SCALE) - 1.0
        raw = F.conv2d(F.pad(x.double(), (pl, pr, pt, pb)), torch.as_tensor(w).double().permute(3, 2, 0, 1), stride=2)
        return (fr, w, scale, shift), dict(raw=nhwc(raw), y=nhwc(torch.clamp(raw * per_channel(scale) + per_channel(shift), 0, 6)))
    (fr, w, scale, shift), want = first_seed(H + cout, make)
    scaled(want)
    fd = dev(fr, torch.uint8 if dtype == np.uint8 else torch.float32)     # uint8 frames lie in 255, float frames in NaN
    code = hip.DT_U8 if dtype == np.uint8 else hip.DT_F32
    wd = dev(w)
    y = out((B, Ho, Wo, cout), guard=image_guard(Wo, cout))
    run(lib.ams_k_stem_conv(P(fd), code, B, H, W, P(wd), cout, PD(scale), PD(shift), hip.ACT_RELU6, S.PIXEL_SCALE, P(y), stream()), "stem_conv")
    assert rel_err(y.cpu().numpy(), want["y"]) < 1e-5
    y = out((B, Ho, Wo, cout), guard=image_guard(Wo, cout))
    run(lib.ams_k_stem_conv(P(fd), code, B, H, W, P(wd), cout, None, None, hip.ACT_NONE, S.PIXEL_SCALE, P(y), stream()), "stem_conv, raw")
    assert rel_err(y.cpu().numpy(), want["raw"]) < 1e-5


# ------------------------------------------------------------------------------------------------ recompute
@pytest.mark.parametrize("H,W,stride", [(5, 17, 1), (17, 16, 2)])
@pytest.mark.parametrize("Cin,Cexp", [(20, 80), (28, 176), (32, 32), (8, 192), (32, 64)])
def test_recompute_block_kernels_at_the_corners_of_their_channels(lib, H, W, Cin, Cexp, stride):
    """The four ams_k_xdw_* entries (and ams_k_xdw_dwe on their sums) with the f64 autograd reference and the asserts of
    test_recompute_block_kernels: Cin = 20 and 28 (a second k chunk of 4 and of 12 channels), Cexp = 80 and 176 (5 and 11 waves: odd counts), 64,
    the smallest and the largest of either range against the other's largest and smallest.  5 x 17: a stride-1 tile row of four and one more
    row, one tile column and one more column; 17 x 16 at stride 2: an odd and an even extent (pad 1 and 0 in front)."""
    recompute_block_kernels(lib, 2, H, W, Cin, Cexp, stride)


def test_expand_weight_gradient_of_the_stem(lib):
    """ams_k_xdw_dwe as engine_backward calls it for the stem: Cin = 27 taps in rows of KP = 32, Cexp = 32; the five pad rows of G1, of XX (and its
    pad columns) and of g0 are zero, as the stem pass leaves them.  dW = cA G1 + g0^T cB + cC (XX W) = x^T (cA dy + cB + cC z) without a pass over
    the pixels; bar: the 5e-5 of test_recompute_block_kernels' expand weight gradient."""
    Cin, Cexp, KP, M = 27, 32, 32, 300

    def make(rng):
        p = rng.standard_normal((M, Cin))
        dy = rng.standard_normal((M, Cexp))
        w = (rng.standard_normal((Cin, Cexp)) / np.sqrt(Cin)).astype(f32)
        cA, cB, cC = (rng.standard_normal(Cexp).astype(f32) for _ in range(3))
        G1 = np.zeros((KP, Cexp), f32); G1[:Cin] = p.T @ dy
        XX = np.zeros((KP, KP), f32); XX[:Cin, :Cin] = p.T @ p
        g0 = np.zeros(KP, f32); g0[:Cin] = p.sum(axis=0)
        dz = cA.astype(f64) * dy + cB.astype(f64) + cC.astype(f64) * (p @ w.astype(f64))       # over the pixels, in f64
        return (G1, np.concatenate([XX.reshape(-1), g0]), w, cA, cB, cC), dict(dw=p.T @ dz)
    (G1, xx_g0, w, cA, cB, cC), want = first_seed(27, make)
    scaled(want)
    dwe = out((Cin, Cexp))
    run(lib.ams_k_xdw_dwe(PD(G1), PD(xx_g0), Cin, Cexp, PD(w), PD(cA), PD(cB), PD(cC), P(dwe), stream()), "xdw_dwe for the stem")
    assert rel_err(dwe.cpu().numpy(), want["dw"]) < 5e-5


@pytest.mark.parametrize("Cexp", [32, 40])
@pytest.mark.parametrize("M", [1, 3, 5, 1027])
@pytest.mark.parametrize("Cin", [4, 5, 17, 20, 28])
def test_expand_statistics_at_the_corners_of_cin(lib, Cin, M, Cexp):
    """ams_k_xx_gram and ams_k_expand_stats accept any Cin in 4 .. 32: the smallest, an odd one, one channel into the second 16-wide chunk, 20 and
    28; one row (a variance of zero), three (less than one 4-pixel group), five, 1027 (five blocks, a last group of three rows).  x has channel
    means several sigma from zero; the bars of test_expand_statistics_from_gram_matrix."""
    eps, omd = 1e-3, 0.1

    def make(rng):
        o = dict(x=(rng.standard_normal((M, Cin)) * rng.uniform(0.2, 2.0, Cin) + rng.standard_normal(Cin) * 3.0).astype(f32),
                 w=(rng.standard_normal((Cin, Cexp)) / np.sqrt(Cin)).astype(f32), gamma=rng.uniform(0.5, 1.5, Cexp).astype(f32),
                 beta=(rng.standard_normal(Cexp) * 0.1).astype(f32), center=(rng.standard_normal(Cexp) * 0.1).astype(f32),
                 mm0=(rng.standard_normal(Cexp) * 0.1).astype(f32), mv0=rng.uniform(0.5, 1.5, Cexp).astype(f32))
        z = o["x"].astype(f64) @ o["w"].astype(f64)
        mean, var = z.mean(axis=0), z.var(axis=0)
        rstd = 1.0 / np.sqrt(var + eps)
        d = z - o["center"].astype(f64)
        return o, dict(mean=mean, rstd=rstd, scale=o["gamma"] * rstd, shift=o["beta"] - mean * o["gamma"] * rstd,
                       mm=o["mm0"] - (o["mm0"] - mean) * omd, mv=o["mv0"] - (o["mv0"] - var * (M / max(M - 1, 1))) * omd,
                       s1=d.sum(axis=0), s2=(d * d).sum(axis=0))
    o, want = first_seed(M + Cin + Cexp, make)
    scaled(want)
    KP = (Cin + 15) // 16 * 16
    n_scr = int(lib.ams_k_xx_gram_scratch(M, Cin))
    scr = scratch(n_scr, torch.float64)
    xx64 = out(KP * KP + KP, torch.float64)
    xx32 = out(KP * KP + KP)
    run(lib.ams_k_xx_gram(PD(o["x"]), M, Cin, P(scr), n_scr, P(xx64), P(xx32), stream()), "xx_gram")
    x64 = o["x"].astype(f64)
    XX = np.zeros((KP, KP)); XX[:Cin, :Cin] = x64.T @ x64
    g0 = np.zeros(KP); g0[:Cin] = x64.sum(axis=0)
    got = xx64.cpu().numpy()
    assert np.abs(got[:KP * KP].reshape(KP, KP) - XX).max() <= 1e-12 * np.abs(XX).max()
    assert np.abs(got[KP * KP:] - g0).max() <= 1e-12 * max(np.abs(g0).max(), 1.0)
    assert np.allclose(xx32.cpu().numpy(), got.astype(f32), rtol=1e-6, atol=0)
    scale, shift, smean, srstd = (out(Cexp) for _ in range(4))
    mm, mv = dev(o["mm0"]), dev(o["mv0"])
    sums = out(2 * Cexp, torch.float64)
    run(lib.ams_k_expand_stats(P(xx64), Cin, PD(o["w"]), Cexp, float(M), PD(o["center"]), PD(o["gamma"]), PD(o["beta"]), eps, omd, P(mm), P(mv), P(scale),
                               P(shift), P(smean), P(srstd), P(sums), stream()), "expand_stats")
    assert rel_err(smean.cpu().numpy(), want["mean"]) < 1e-6 and rel_err(srstd.cpu().numpy(), want["rstd"]) < 1e-6
    assert rel_err(scale.cpu().numpy(), want["scale"]) < 1e-6 and rel_err(shift.cpu().numpy(), want["shift"]) < 2e-6
    assert rel_err(mm.cpu().numpy(), want["mm"]) < 1e-6 and rel_err(mv.cpu().numpy(), want["mv"]) < 1e-6
    s = sums.cpu().numpy()
    assert rel_err(s[:Cexp], want["s1"]) < 1e-9 and rel_err(s[Cexp:], want["s2"]) < 1e-9
