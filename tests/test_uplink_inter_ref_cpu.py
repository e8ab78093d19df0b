"""The NumPy oracle of the predicted uplink frame AUP1 (tests/uplink_inter_ref.py) against itself and against plain statements of its rules:
what the device tests then hold the kernels to, byte for byte."""
import functools

import numpy as np
import pytest

import uplink_ref as U
import uplink_inter_ref as P

SHAPE = (48, 80)


@functools.lru_cache(maxsize=None)
def pairs():
    return P.pairs(*SHAPE)


@functools.lru_cache(maxsize=None)
def clip_frames(n=4):
    from ams_amd import synth
    video = synth.SyntheticVideo(SHAPE[0], 1, [0, 1, 2, 10, 11, 13], seed=3)
    return [np.ascontiguousarray(video.frame(t)[0][:SHAPE[0], :SHAPE[1]]) for t in range(n)]


def test_rank_is_the_tie_order():
    assert len(P.RANK) == 961 < 1024 and P.RANK[(0, 0)] == 0
    assert P.RANK[(-1, 0)] < P.RANK[(0, -1)] < P.RANK[(0, 1)] < P.RANK[(1, 0)] < P.RANK[(-2, 0)]
    assert (255 * 256 + max(0, 64, 128, 256, 512)) < 1 << 22     # cost << 10 | rank fits 32 bits for every bias of the grid


@pytest.mark.parametrize("name", ("clip", "unrelated", "shift", "extremes"))
def test_vectorised_search_equals_the_triple_loop(name):
    cur, ref = pairs()[name]
    cy, ry = P.planes_of(cur)[0], P.planes_of(ref)[0]
    for bias in (0, P.ZERO_BIAS):
        got = P.search(cy, ry, bias)
        assert np.array_equal(got, P.search_naive(cy, ry, bias))
        mw = SHAPE[1] // 16
        assert all(P.legal(*SHAPE, i // mw, i % mw, *v) for i, v in enumerate(got.tolist()))


@pytest.mark.parametrize("name", sorted(P.pairs(16, 16)))
@pytest.mark.parametrize("q", (1, 50, 100))
def test_decode_gives_the_encoders_reconstruction(name, q):
    cur, ref = pairs()[name]
    analysed = P.analyse(cur, ref)
    payload = P.encode(cur, ref, q, analysed)
    assert len(payload) == P.size_table(cur, ref, analysed)[q - 1] <= P.max_bytes(*SHAPE)
    back = P.decode(payload, ref)
    assert np.array_equal(back, P.encoder_reconstruction(cur, ref, q, analysed))
    rq, vectors, planes, status = P.parse(payload, *SHAPE)
    assert (rq, status) == (q, U.OK) and np.array_equal(vectors, analysed[0])
    assert all(np.array_equal(lv, U.quantise(c, q, i > 0)) for i, (lv, c) in enumerate(zip(planes, analysed[1])))


def test_chroma_averages_are_both_used():
    cur, ref = pairs()["odd"]
    v = P.analyse(cur, ref)[0]
    assert (v[:, 0] & 1).any() and (v[:, 1] & 1).any() and ((v[:, 0] & 1) & (v[:, 1] & 1)).any()
    one = P.analyse(cur, ref, vectors=np.array([[1, 0] if P.legal(*SHAPE, i // 5, i % 5, 1, 0) else [0, 0] for i in range(15)]))
    assert np.array_equal(P.decode(P.encode(cur, ref, 50, one), ref), P.encoder_reconstruction(cur, ref, 50, one))


def test_four_frame_chain_does_not_drift():
    frames = clip_frames()
    payloads, decoded = P.chain(frames, 50)
    assert [P.kind_of(p) for p in payloads] == [P.INTRA] + [P.INTER] * 3
    # the decoder's frame k is the encoder's own reconstruction of frame k against the decoder's frame k - 1: the loop is closed
    for k in range(1, 4):
        assert np.array_equal(decoded[k], P.encoder_reconstruction(frames[k], decoded[k - 1], 50))
    err = [np.abs(d.astype(np.int64) - f).mean() for d, f in zip(decoded, frames)]
    assert max(err[1:]) < 2 * err[0] + 1, err                    # the error of the last frame is of the first frame's order


@pytest.mark.parametrize("shape", [(16, 16), (16, 144), (48, 80), (128, 256)])
def test_a_repeated_frame_costs_header_and_table(shape):
    cur = P.pairs(*shape)["same"][0]
    analysed = P.analyse(cur, cur)
    n = P.slice_count(*shape)
    assert np.array_equal(P.size_table(cur, cur, analysed), np.full(100, 16 + 2 * n))
    for q in (1, 37, 100):
        payload = P.encode(cur, cur, q, analysed)
        assert len(payload) == 16 + 2 * n and P.zero_length_slices(payload, *shape) == (n, n)
        assert np.array_equal(P.decode(payload, cur), U.ycc_to_rgb(*P.planes_of(cur)))          # the reference through the colour legs


@pytest.mark.parametrize("shape", [(48, 80), (128, 256)])
def test_every_malformed_payload_is_refused_with_its_status(shape):
    cur, ref = P.pairs(*shape)["clip"]
    good = P.encode(cur, ref, 50)
    cases = P.malformed(good, *shape)
    for name in ("vector_dy_16", "vector_dx_-16", "window_top", "window_left", "window_right", "window_bottom", "zero_motion_long", "zero_levels_long",
                 "magic", "intra_magic", "table_sum", "position", "zero_level", "level", "overrun", "padding_bit"):
        assert name in cases
    for name, (bad, want) in cases.items():
        assert P.parse(bad, *shape)[3] == want, name
        with pytest.raises(U.Refused) as e:
            P.decode(bad, ref)
        assert e.value.status == want, name
    assert {P.BAD_VECTOR, P.BAD_ZERO_SLICE} == {9, 10} and U.NO_ROOM == 8


def test_each_decoder_refuses_the_other_kind():
    cur, ref = pairs()["clip"]
    assert P.parse(U.encode(cur, 50), *SHAPE)[3] == U.BAD_HEADER
    assert U.parse(P.encode(cur, ref, 50), *SHAPE)[2] == U.BAD_HEADER


def test_rate_rule_and_its_tie_breaks():
    up = np.arange(100, 200)
    # the larger quality wins
    assert P.choose(up, up + 5, 150) == (P.INTRA, 51, True) and P.choose(up + 5, up, 150) == (P.INTER, 51, True)
    # equal quality: the smaller payload
    a, b = up.copy(), up.copy()
    b[50] = 148
    assert P.choose(a, b, 150) == (P.INTER, 51, True) and P.choose(b, a, 150) == (P.INTRA, 51, True)
    # equal quality and size: intra
    assert P.choose(up, up, 150) == (P.INTRA, 51, True)
    # only one fits; neither fits
    assert P.choose(up + 100, up, 120) == (P.INTER, 21, True) and P.choose(up, up + 100, 120) == (P.INTRA, 21, True)
    assert P.choose(up, up, 99) == (P.INTRA, 1, False)
    cur, ref = pairs()["clip"]
    intra, inter = U.size_table(cur), P.size_table(cur, ref)
    for budget in (int(min(intra[0], inter[0])) - 1, int(inter[40]), int(intra[99])):
        payload, q, fits, kind = P.encode_to_budget(cur, budget, ref)
        assert (kind, q, fits) == P.choose(intra, inter, budget) and P.kind_of(payload) == kind and (not fits or len(payload) <= budget)
        assert P.encode_to_budget(cur, budget)[:3] == U.encode_to_budget(cur, budget)[:3]


def test_residual_coefficients_stay_within_2047():
    """ref 0 under cur 255 and the reverse, flat and as every +-255 sign pattern of one basis function; and the bound the header derives"""
    et = 0.5 + 255.0 * U.R1 / 1024.0
    bound = 0.5 + U.A1 * et / 8.0 + U.R1 * (8.0 * U.A1 * 255.0 + et) / 65536.0
    assert abs(U.A1 - 8 / np.sqrt(8)) < 1e-12 and 255 * U.A1 ** 2 + bound <= 2047, bound
    signs = np.sign(np.einsum("vi,uj->vuij", U.C8, U.C8)).reshape(64, 8, 8).astype(np.int64)
    signs[signs == 0] = 1
    worst = 0
    for s in (1, -1):
        c = U.fdct(s * 255 * signs)
        worst = max(worst, int(np.abs(c).max()))
        assert np.abs(c - np.einsum("vi,nij,uj->nvu", U.C8, s * 255.0 * signs, U.C8)).max() <= bound
    assert 2040 - bound <= worst <= 2040 + bound <= 2047
    cur, ref = pairs()["extremes"]
    for a, b in ((cur, ref), (ref, cur)):
        zero = np.zeros((P.macroblocks(*SHAPE), 2), np.int64)
        planes = P.analyse(a, b, vectors=zero)[1]
        assert max(int(np.abs(p).max()) for p in planes) <= 2047 and abs(int(np.abs(planes[0]).max()) - 2040) <= bound
        assert np.array_equal(P.decode(P.encode(a, b, 100, vectors=zero), b), P.encoder_reconstruction(a, b, 100, P.analyse(a, b, vectors=zero)))
