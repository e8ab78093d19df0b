"""What tests/test_gpu_first_block.py stands on, proved without a GPU:
(a) its f64 reference (tests/first_block_ref.py) is the oracle's own first three layers in frozen mode;
(b) its error measure and bars catch small defects: each mutation of the reference lies at least 10 x above the wider bar;
(c) the launch plan's interior rectangle is the set its definition names, tile by tile and loaded byte by loaded byte, at every case size — and the plan of the walking case
    on a 256-CU part gives every block more than one tile in both launches;
(d) what the two kernel-level entries refuse, in which order and in which words.  No row reaches a device call."""
import ctypes as C

import numpy as np
import pytest
import torch

import first_block_ref as R
from ams_amd import hip, spec as S

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, never dereferenced: the checks compare it against NULL
E_INVALID = -1


# ---------------------------------------------------------------------------------------------------------------- (a) the reference
@pytest.mark.parametrize("H,W", [(35, 67), (34, 66)])
def test_reference_is_the_oracles_first_three_layers(H, W):
    from ams_amd.weights import synthetic_weights
    from oracle.student_torch import StudentOracle
    sp = S.build_spec()
    W0 = synthetic_weights(sp, seed=3)
    fr = R.frames(2, H, W, "bytes")
    taps = {}
    StudentOracle(W0, [0, 1, 2, 10, 11, 13], dtype=torch.float64).forward_lowres(fr.astype(np.float64), "frozen", taps=taps)
    l1, l2, l3 = sp.layers[:3]
    assert (l1.kind, l2.kind, l3.kind) == ("conv", "dw", "conv") and (l1.act, l2.act, l3.act) == ("relu6", "relu6", "none")
    w = {}
    for l, (wn, sn, hn) in zip((l1, l2, l3), (("w_stem", "sc_s", "sh_s"), ("w_dw", "sc_d", "sh_d"), ("w_proj", "sc_p", "sh_p"))):
        g, b = (W0[l.scope + "/BatchNorm/%s:0" % n].astype(np.float64) for n in ("gamma", "beta"))
        m, v = (W0[l.scope + "/BatchNorm/%s:0" % n].astype(np.float64) for n in ("moving_mean", "moving_variance"))
        w[sn] = g / np.sqrt(v + S.BN_EPS_FROZEN)
        w[hn] = b - m * w[sn]
        w[wn] = W0[l.weight_name].astype(np.float64)
    w["w_proj"] = w["w_proj"].reshape(32, 16)
    got = R.first_block(fr, w, S.PIXEL_SCALE)
    want = taps[l3.scope].numpy()
    assert got.shape == want.shape == (2,) + R.out_size(H, W) + (16,)
    assert R.measure(got, want) < 1e-13


# ---------------------------------------------------------------------------------------------------------------- (b) the measure
def test_bars_come_from_the_f32_level_and_stay_under_the_cap():
    L, at = R.f32_level()
    bars = R.bars()
    print("first block: f32 CPU level L = %.3g at %s; bars f32 %.3g, split %.3g" % (L, at, bars["f32"], bars["split"]))
    assert 1e-7 < L < R.BAR_CAP / R.FACTOR_SPLIT, "f32 evaluation of the reference: L = %g" % L       # f32's own 6e-8 .. the cap
    assert bars["f32"] == R.FACTOR_F32 * L and bars["split"] == R.FACTOR_SPLIT * L


@pytest.mark.parametrize("mutation", R.MUTATIONS)
@pytest.mark.parametrize("H,W", [(34, 66), (35, 67), (51, 131)])
def test_measure_catches_small_defects(H, W, mutation):
    if mutation == "same_pad_other_side" and (H % 2 == 0 or W % 2 == 0):
        # an even frame size pads 1 / 1: there is no other side.  The two odd sizes carry this mutation
        H, W = H + 1, W + 1
    ps = 1.0 / 128.0 if mutation == "pad_value_128" else S.PIXEL_SCALE
    ref = R.reference(R.B, H, W, "bytes", ps)
    e = R.channel_errors(R.first_block(R.frames(R.B, H, W, "bytes"), R.weights(), ps, mutation=mutation), ref)
    print("%s at %d x %d: worst channel %.3g, smallest affected %.3g" % (mutation, H, W, e.max(), e[e > 0].min()))
    assert e.max() >= 10.0 * R.bars()["split"], (mutation, e.max())


def test_pad_value_is_invisible_at_the_default_pixel_scale():
    """Why the cases include 1/128: at 1/127.5 the 127.5 pad normalises to exactly 0, the value of the SAME padding outside the frame."""
    assert float(np.float32(127.5) * np.float32(S.PIXEL_SCALE)) - 1.0 == 0.0
    assert float(np.float32(127.5) * np.float32(1.0 / 128.0)) - 1.0 == -1.0 / 256.0


# ---------------------------------------------------------------------------------------------------------------- (c) the plan
MI355X = (C.c_int32 * 3)(3, 2, 256)     # the two walking kernels' launch bounds (3 and 2 blocks per CU) on 256 CUs


def _plan(Bn, H, W, form=2, dtype=hip.DT_U8, occupancy=MI355X):
    p = hip.FirstBlockPlan()
    hip.check(hip.lib().ams_k_first_block_plan(dtype, Bn, H, W, form, occupancy, C.byref(p)))
    return p


# the case sizes with a walked tile.  34 x 66, 35 x 67, 34 x 67 and 35 x 66 have one tile with all its taps, whose last window ends at the frame's
# last pixel: the kernel's 8-byte load of that window's third row would end behind the frame, so the tile goes to the border launch
WALKED = {(34, 68), (36, 66), (35, 68), (36, 67), (36, 68), (50, 98), (51, 131), R.WALK_CASE[1:]}


@pytest.mark.parametrize("H,W", list(R.SIZES) + [R.WALK_CASE[1:]])
def test_plan_interior_rectangle_is_its_definition(H, W):
    p = _plan(R.B, H, W)
    Ho, Wo = R.out_size(H, W)
    assert (p.out_h, p.out_w) == (Ho, Wo) and (p.tiles_y, p.tiles_x) == (-(-Ho // R.TH), -(-Wo // R.TW))
    assert (p.pad_top, p.pad_left) == (S.same_pad(H + 1, 3, 2, 1)[1], S.same_pad(W + 1, 3, 2, 1)[1])
    taps_ok, loads_ok = R.interior_tiles_by_definition(H, W)
    want = R.planned_interior_tiles(H, W)
    got = {(ty, tx) for ty in range(p.ity0, p.ity0 + p.niy) for tx in range(p.itx0, p.itx0 + p.nix)}
    assert got <= loads_ok, "the walking kernel would load bytes outside the frame at tiles %s" % sorted(got - loads_ok)
    assert got == want
    assert bool(taps_ok) == (H >= 34 and W >= 66), "34 x 66 is the smallest case whose middle tile has all its taps"
    assert bool(want) == ((H, W) in WALKED)
    per_frame = p.tiles_y * p.tiles_x
    if want:
        assert p.interior_tiles == R.B * len(want) and p.border_tiles == R.B * (per_frame - len(want)) and p.border_walks == 1
        assert 0 < p.interior_grid <= p.interior_tiles and 0 < p.border_grid <= p.border_tiles
    else:
        assert (p.interior_tiles, p.interior_grid, p.border_walks) == (0, 0, 0) and p.border_tiles == p.border_grid == R.B * per_frame


def test_plan_of_the_other_forms_and_dtypes_is_one_tile_per_block():
    for form, dtype in ((0, hip.DT_U8), (1, hip.DT_U8), (2, hip.DT_F32), (0, hip.DT_F32)):
        p = _plan(R.B, 51, 131, form, dtype)
        assert (p.interior_tiles, p.interior_grid, p.border_walks) == (0, 0, 0) and p.border_tiles == p.border_grid == R.B * p.tiles_y * p.tiles_x


def test_plan_of_the_walking_case_gives_every_block_more_than_one_tile():
    Bn, H, W = R.WALK_CASE
    p = _plan(Bn, H, W)
    assert (p.tiles_y, p.tiles_x, p.niy, p.nix) == (13, 13, 11, 11)
    assert p.interior_tiles == Bn * 121 and p.border_tiles == Bn * 48
    assert -(-p.interior_tiles // p.interior_grid) == 3 and -(-p.border_tiles // p.border_grid) == 2          # rounds
    assert 2 * p.interior_grid <= p.interior_tiles and p.border_grid < p.border_tiles
    assert p.interior_tiles % p.interior_grid, "a ragged last share"
    assert p.interior_tiles % 121 == 0 and p.interior_grid % 121, "shares cross frame boundaries"


def test_plan_follows_the_walk_knob(knobs):
    Bn, H, W = R.WALK_CASE
    knobs(AMS_FB_WALK=0)
    p = _plan(Bn, H, W)
    assert p.interior_tiles == 0 and p.border_grid == Bn * 169
    knobs(AMS_FB_WALK=1)
    p = _plan(Bn, H, W)
    assert p.interior_grid == p.interior_tiles == Bn * 121 and p.border_grid == p.border_tiles == Bn * 48 and p.border_walks == 1
    knobs(AMS_FB_WALK=-2)
    p = _plan(Bn, H, W)
    assert p.interior_tiles == Bn * 121 and p.border_grid == p.border_tiles == Bn * 48 and p.border_walks == 0


# ---------------------------------------------------------------------------------------------------------------- (d) the refusals
def _args(**over):
    a = dict(frames=NULL, dtype=hip.DT_U8, B=3, H=35, W=67, form=2, panels=UNREAD, panel_elems=3072, w=UNREAD, y=UNREAD)
    a.update(over)
    return a


def _call(entry, a):
    lib = hip.lib()
    head = (a["frames"], a["dtype"], a["B"], a["H"], a["W"], C.c_float(S.PIXEL_SCALE)) + (a["w"],) * 9 + (a["y"],)
    if entry == "first_block":
        return lib.ams_k_first_block(*head, a["form"], a["panels"], a["panel_elems"], None, NULL)
    assert entry == "first_block_tiles"
    return lib.ams_k_first_block_tiles(*head, NULL)


BOTH = ("first_block", "first_block_tiles")
FORMS = ("first_block",)
# a fault per refusable argument, in the order of refusal: name -> (entries that can be given it, overrides, the word in the message)
FAULTS = {
    "dtype": (BOTH, dict(dtype=hip.DT_I32), b"frames must be uint8 or float32"),
    "size": (BOTH, dict(H=0), b"no pixels"),
    "form": (FORMS, dict(form=3), b"unknown form 3"),
    "panels": (FORMS, dict(panel_elems=3071), b"panel scratch too small (need 3072)"),
}
RANK = list(FAULTS)
MORE = [("dtype", dict(dtype=hip.DT_F64), None), ("dtype", dict(dtype=-1), None), ("size", dict(B=0), None), ("size", dict(W=-5), None),
        ("form", dict(form=-1), b"unknown form -1"), ("panels", dict(panels=NULL), None), ("panels", dict(form=1, panel_elems=100), None)]
SINGLE = [(e, f, FAULTS[f][1], FAULTS[f][2]) for f in RANK for e in FAULTS[f][0]] + \
         [(e, f, o, word or FAULTS[f][2]) for f, o, word in MORE for e in FAULTS[f][0]]


def _id(v):
    if isinstance(v, bytes):
        return v.decode()
    return v if isinstance(v, str) else ",".join("%s=%s" % (k, "NULL" if v[k] is NULL else "ptr" if v[k] is UNREAD else v[k]) for k in v)


def _refused(entry, a, word):
    assert _call(entry, a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("entry,fault,over,word", SINGLE, ids=_id)
def test_each_fault_is_refused_in_words(entry, fault, over, word):
    _refused(entry, _args(**over), word)


@pytest.mark.parametrize("entry,first,later", [(e, f, g) for e in BOTH for i, f in enumerate(RANK) for g in RANK[i + 1:]
                                               if e in FAULTS[f][0] and e in FAULTS[g][0]])
def test_the_earlier_ranked_fault_wins(entry, first, later):
    msg = _refused(entry, _args(**dict(FAULTS[first][1], **FAULTS[later][1])), FAULTS[first][2])
    assert FAULTS[later][2] not in msg, msg


@pytest.mark.parametrize("entry", BOTH)
def test_a_call_without_fault_reaches_the_null_pointers(entry):
    """frames is NULL in every row above, so a row whose refusal went missing would have ended here and not in a launch."""
    _refused(entry, _args(), b"null pointer")
    _refused(entry, _args(frames=UNREAD, y=NULL), b"null pointer")
    _refused(entry, _args(frames=UNREAD, w=NULL), b"null pointer")
    if entry == "first_block":
        _refused(entry, _args(form=0, panels=NULL, panel_elems=0), b"null pointer")          # form 0 needs no panels


def test_scratch_sizes():
    lib = hip.lib()
    assert [lib.ams_k_first_block_scratch(f) for f in (0, 1, 2)] == [0, 3 * 32 * 32, 2 * 32 * 32 + 2 * 16 * 32]


def test_plan_query_refusals():
    lib = hip.lib()
    p = hip.FirstBlockPlan()
    for over, word in ((dict(dtype=hip.DT_I32), b"frames must be"), (dict(B=0), b"no pixels"), (dict(form=5), b"unknown form 5")):
        a = _args(**over)
        assert lib.ams_k_first_block_plan(a["dtype"], a["B"], a["H"], a["W"], a["form"], MI355X, C.byref(p)) == E_INVALID
        assert word in lib.ams_last_error()
    assert lib.ams_k_first_block_plan(hip.DT_U8, 3, 35, 67, 2, (C.c_int32 * 3)(3, 0, 256), C.byref(p)) == E_INVALID
    assert lib.ams_k_first_block_plan(hip.DT_U8, 3, 35, 67, 2, MI355X, None) == E_INVALID and b"null pointer" in lib.ams_last_error()
