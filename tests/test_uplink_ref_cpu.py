"""tests/uplink_ref.py, the NumPy statement of the uplink frame codec AUC1, held to the mathematics it restates and to its own format:

  a. the integer transform against the f64 orthonormal DCT, the colour conversion against the f64 JFIF equations and the decoder against the
     same steps in real numbers, each inside the bound the oracle's docstring derives from the rounding steps (the measured figure is printed);
  b. the division the kernels replace by a multiplication is exact over every numerator they can meet;
  c. header and table arithmetic, the sizes, the worst block;
  d. every listed malformed payload is refused, with the status the device must give;
  e. the rate rule: the largest quality that fits, whatever the order of the sizes; fits = False below the smallest payload.
"""
import numpy as np
import pytest

import uplink_ref as U

SHAPE = (48, 80)


@pytest.fixture(scope="module")
def contents():
    return U.frames(*SHAPE)


def test_integer_transform_is_within_its_bound_of_the_f64_dct():
    rng = np.random.RandomState(1)
    blocks = [rng.randint(-128, 128, (20000, 8, 8))]
    for v in range(8):
        for u in range(8):
            s = np.where(np.outer(U.C8[v], U.C8[u]) >= 0, 127, -128)          # the pattern that drives coefficient (v, u) furthest
            blocks += [s[None], (-1 - s)[None]]
    blocks += [np.full((1, 8, 8), -128), np.full((1, 8, 8), 127)]
    x = np.concatenate(blocks).astype(np.int64)
    assert len(x) == 20130
    c = U.fdct(x)
    exact = np.einsum("vi,nij,uj->nvu", U.C8, x.astype(np.float64), U.C8)
    err = np.abs(c - exact).max()
    print("forward transform: |c - f64| <= %.4f (bound %.4f), |c| <= %d" % (err, U.FWD_BOUND, np.abs(c).max()))
    assert err <= U.FWD_BOUND < 1.0
    assert np.abs(c).max() <= 1024 + U.FWD_BOUND                                # what the kernels' 12-bit numerators rest on
    back = U.idct(c)
    assert np.abs(back - (x + 128)).max() <= 2                                   # two rounded passes each way


def test_the_reciprocal_division_of_the_kernels_is_exact():
    n = np.arange(4096, dtype=np.uint64)[:, None]
    d = np.arange(1, 256, dtype=np.uint64)[None, :]
    m = ((1 << 20) + d - 1) // d
    assert (n * m).max() < 1 << 32                                               # the product stays in 32 bits
    assert np.array_equal((n * m) >> 20, n // d)


def test_colour_conversion_is_within_its_bound_of_the_f64_equations():
    rng = np.random.RandomState(2)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    rgb = np.concatenate([corners, rng.randint(0, 256, (400000, 3))]).astype(np.uint8)[None]
    planes = U.rgb_to_ycc(rgb)
    f = rgb.astype(np.float64)
    exact = {"Y": 0.299 * f[..., 0] + 0.587 * f[..., 1] + 0.114 * f[..., 2],
             "Cb": -0.168736 * f[..., 0] - 0.331264 * f[..., 1] + 0.5 * f[..., 2] + 128,
             "Cr": 0.5 * f[..., 0] - 0.418688 * f[..., 1] - 0.081312 * f[..., 2] + 128}
    for p, name in zip(planes, ("Y", "Cb", "Cr")):
        err = np.abs(p - np.clip(exact[name], 0, 255)).max()
        print("%s: %.4f (bound %.4f)" % (name, err, U.COLOUR_BOUNDS[name]))
        assert err <= U.COLOUR_BOUNDS[name] < 0.51
    q = rng.randint(0, 256, (64, 64)).astype(np.int64)
    assert np.abs(U.subsample(q) - q.reshape(32, 2, 32, 2).mean((1, 3))).max() <= 0.5
    # back: integer planes through the integer and the real equations
    ycc = np.concatenate([np.array([[y, cb, cr] for y in (0, 255) for cb in (0, 255) for cr in (0, 255)]), rng.randint(0, 256, (100000, 3))])
    y, cb, cr = (ycc[None, :, i] for i in range(3))              # chroma planes [1, n]; every 2 x 2 of the Y plane holds one y
    rep = lambda p: np.repeat(np.repeat(p, 2, 0), 2, 1)
    got = U.ycc_to_rgb(rep(y), cb, cr).astype(np.float64)
    yf, cbf, crf = rep(y).astype(np.float64), rep(cb) - 128.0, rep(cr) - 128.0
    want = np.clip(np.stack([yf + 1.402 * crf, yf - 0.344136 * cbf - 0.714136 * crf, yf + 1.772 * cbf], -1), 0, 255)
    for i, name in enumerate("RGB"):
        err = np.abs(got[..., i] - want[..., i]).max()
        print("%s: %.4f (bound %.4f)" % (name, err, U._INV_C[name]))
        assert err <= U._INV_C[name] < 0.51


@pytest.mark.parametrize("name,q", [("clip", 10), ("clip", 60), ("clip", 100), ("noise", 100), ("primaries", 75), ("checker", 90), ("constant", 50)])
def test_decoder_is_within_its_bound_of_the_f64_decode(contents, name, q):
    H, W = SHAPE
    payload = U.encode(contents[name], q)
    got_q, planes, status = U.parse(payload, H, W)
    assert (got_q, status) == (q, U.OK)
    want = [U.quantise(c, q, i > 0) for i, c in enumerate(U.transform(contents[name]))]
    assert all(np.array_equal(a, b) for a, b in zip(planes, want))               # the entropy code is lossless
    cmax = max(int(np.abs(U.dequantise(lv, q, i > 0)).max()) for i, lv in enumerate(planes))
    got = U.reconstruct(planes, q, H, W).astype(np.float64)
    assert np.array_equal(got, U.decode(payload, H, W))
    exact = U.reconstruct_f64(planes, q, H, W)
    bounds = U.decode_bounds(cmax)
    for i, ch in enumerate("RGB"):
        err = np.abs(got[..., i] - exact[..., i]).max()
        print("%s q=%d %s: %.3f (bound %.3f at cmax %d)" % (name, q, ch, err, bounds[ch], cmax))
        assert err <= bounds[ch]


def test_decoder_bound_holds_at_the_clamp():
    """levels no encoder produces: every dequantised coefficient at or beyond +-2047"""
    H, W = 16, 32
    rng = np.random.RandomState(3)
    planes = [rng.choice([-2047, 2047, -300, 300, 0], (n, 64)) for n in U.plane_blocks(H, W)]
    got = U.reconstruct(planes, 50, H, W).astype(np.float64)
    exact = U.reconstruct_f64(planes, 50, H, W)
    bounds = U.decode_bounds(2047)
    for i, ch in enumerate("RGB"):
        assert np.abs(got[..., i] - exact[..., i]).max() <= bounds[ch]


def test_header_table_and_sizes(contents):
    H, W = SHAPE
    assert U.plane_blocks(H, W) == [60, 15, 15] and U.slice_counts(H, W) == [2, 1, 1]
    assert U.max_bytes(H, W) == 16 + 2 * 4 + 208 * 90 and U.BLOCK_MAX_BITS == 1664
    sizes = U.size_table(contents["clip"])
    for q in (1, 37, 100):
        p = U.encode(contents["clip"], q)
        assert p[:4] == b"AUC1" and U.header_size(p) == (H, W) and p[8] == q and p[9:12] == b"\0\0\0"
        assert int.from_bytes(p[12:16], "little") == len(p) == sizes[q - 1] <= U.max_bytes(H, W)
        lens = np.frombuffer(p[16:24], "<u2")
        assert 16 + 8 + int(lens.sum()) == len(p) and lens.min() >= 1
    # the worst block: the largest DC step and 63 levels of the largest magnitude, each behind a run of 0
    lv = np.zeros((2, 64), np.int64)
    lv[0, 0], lv[1, 0] = 2047, -2047
    lv[1, 1:] = np.where(np.arange(63) & 1, 2047, -2047)
    assert U.block_bits(lv)[1] == U.BLOCK_MAX_BITS
    vals, nbits = U._symbols(lv)
    assert int(nbits.sum()) == int(U.block_bits(lv).sum())


def test_every_malformed_payload_is_refused(contents):
    for H, W in ((16, 16), SHAPE):
        payload = U.encode(U.frames(H, W)["clip"], 50)
        assert U.parse(payload, H, W)[2] == U.OK
        cases = U.malformed(payload, H, W)
        assert {st for _, st in cases.values()} == {U.BAD_HEADER, U.BAD_TABLE, U.BAD_SLICE_END, U.BAD_POSITION, U.BAD_ZERO_LEVEL, U.BAD_LEVEL,
                                                    U.BAD_OVERRUN}
        for name, (bad, status) in cases.items():
            assert U.parse(bad, H, W)[2] == status, name
            with pytest.raises(U.Refused) as e:
                U.decode(bad, H, W)
            assert e.value.status == status, name


def test_several_malformed_slices_give_the_largest_status():
    H, W = SHAPE
    payload = bytearray(U.malformed(U.encode(U.frames(H, W)["clip"], 50), H, W)["zero_level"][0])
    assert U.parse(bytes(payload), H, W)[2] == U.BAD_ZERO_LEVEL
    payload[-1] |= 1                                             # the last slice's last padding bit (or a code's last bit) as well
    assert U.parse(bytes(payload), H, W)[2] >= U.BAD_ZERO_LEVEL


def test_rate_rule(contents):
    frame = contents["clip"]
    sizes = U.size_table(frame)
    assert np.array_equal(sizes, [len(U.encode(frame, q)) for q in range(1, 101)])
    for budget in (int(sizes[0]), int(sizes[40]), int(sizes[40]) + 1, int(sizes[99]), 10 ** 9):
        payload, q, fits, table = U.encode_to_budget(frame, budget)
        assert fits and len(payload) <= budget and np.array_equal(table, sizes)
        assert q == max(k for k in range(1, 101) if sizes[k - 1] <= budget) and payload == U.encode(frame, q)
    payload, q, fits, _ = U.encode_to_budget(frame, int(sizes[0]) - 1)
    assert (q, fits) == (1, False) and payload == U.encode(frame, 1)
    # defined over all 100 sizes, not by bisection: an order no frame need give
    odd = np.array([50] * 100)
    odd[[3, 70]] = 20
    assert U.choose_quality(odd, 30) == (71, True) and U.choose_quality(odd, 19) == (1, False) and U.choose_quality(odd, 50) == (100, True)
