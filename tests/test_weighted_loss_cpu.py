"""The weighted fine-tune loss (per-class weights cw_k, teacher-confidence exponent gamma) where no GPU is needed: header and binding agree on
the two new prototypes, the C ABI refuses invalid weights before it looks at any pointer, run.py's parser and SemanticNetwork's constructor
refuse what they cannot serve and name the argument, balanced_class_weights on hand-worked counts, and two facts the GPU tests lean on: the
f64 objective separates the knob settings by far more than the kernel's bar, and the quantised weight is exact in f32."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from ams_amd import exp_configs, hip, run as R
from ams_amd.semantic_network import SemanticNetwork
from loss_ref import header_prototype
from ams_amd.utils import balanced_class_weights, label_class_counts

ROOT = Path(__file__).resolve().parent.parent
NULL = C.c_void_p(0)
E_INVALID = -1


def _floats(values):
    return (C.c_float * len(values))(*values) if values is not None else None


def _null_call(lib, weights, K, gamma, temperature=2.0, alpha=0.5):
    """Every other pointer null and every size 0: only checks of the weights and gamma in front of everything else let this return in order."""
    return lib.ams_k_ce_loss_grad_weighted(NULL, 0, 0, 0, 0, 0, None, K, 0, 0, NULL, NULL, 0, 0, 0, NULL, NULL, NULL, 0, NULL, temperature, alpha,
                                           _floats(weights), gamma)


def test_error_code_is_the_headers():
    text = (ROOT / "include" / "ams_hip.h").read_text()
    assert int(re.search(r"\bAMS_E_INVALID\s*=\s*(-?\d+)", text).group(1)) == E_INVALID


@pytest.mark.parametrize("name", ["ams_student_set_loss_weights", "ams_k_ce_loss_grad_weighted"])
def test_header_and_binding_agree_on_the_prototypes(name):
    assert header_prototype(name) == tuple(hip.SIGNATURES[name])
    fn = getattr(hip.lib(), name)
    assert fn.restype is hip.SIGNATURES[name][0] and list(fn.argtypes) == hip.SIGNATURES[name][1]
    # the weighted entry is the kd entry with the weight table and gamma behind it
    if name == "ams_k_ce_loss_grad_weighted":
        assert hip.SIGNATURES[name][1] == hip.SIGNATURES["ams_k_ce_loss_grad_kd"][1] + [C.POINTER(C.c_float), C.c_float]


@pytest.mark.parametrize("bad", [float("nan"), -1.0, 2.0 ** -7, 1e-30, 16.5, float("inf")])
def test_kernel_entry_refuses_a_bad_weight_before_any_pointer(bad):
    lib = hip.lib()
    assert _null_call(lib, [1.0, bad, 1.0], 3, 0.0) == E_INVALID
    assert b"class_weights[1]" in lib.ams_last_error()


@pytest.mark.parametrize("gamma", [-0.5, 8.5, float("nan"), float("inf")])
def test_kernel_entry_refuses_a_bad_gamma_before_any_pointer(gamma):
    lib = hip.lib()
    assert _null_call(lib, [1.0, 2.0, 1.0], 3, gamma) == E_INVALID
    assert b"conf_gamma" in lib.ams_last_error() and b"class_weights[" not in lib.ams_last_error()


def test_kd_knobs_are_still_checked_first():
    lib = hip.lib()
    assert _null_call(lib, [float("nan")], 1, float("nan"), temperature=0.0) == E_INVALID
    assert b"temperature" in lib.ams_last_error()


@pytest.mark.parametrize("weights", [[0.0, 2.0 ** -6, 16.0], None])
def test_valid_weights_reach_the_pointer_checks(weights):
    """The edges of the range and the NULL table are accepted; the call is then refused for its null teacher logits (alpha = 0.5), nothing launched."""
    lib = hip.lib()
    assert _null_call(lib, weights, 3, 8.0) == E_INVALID
    assert b"null teacher logits" in lib.ams_last_error()
    # gamma = 0 and alpha = 0 need no teacher logits: the next check speaks
    assert _null_call(lib, weights, 3, 0.0, alpha=0.0) == E_INVALID
    assert b"null class table" in lib.ams_last_error()
    # gamma > 0 with alpha = 0 does
    assert _null_call(lib, weights, 3, 2.0, alpha=0.0) == E_INVALID
    assert b"null teacher logits" in lib.ams_last_error()


def test_set_loss_weights_on_a_null_student_fails_cleanly():
    lib = hip.lib()
    assert lib.ams_student_set_loss_weights(NULL, _floats([1.0]), 1, 0.0) == E_INVALID
    assert b"null student" in lib.ams_last_error()


# ---------------------------------------------------------------------------------------------------------
# run.py's flags
# ---------------------------------------------------------------------------------------------------------
BASE = ["--student_checkpoint", "synthetic:0", "--output_dir", "unused", "--mode", "simple", "--input_video", "synthetic:25-synth:seconds=4:fps=1"]
SOFT = ["--soft_teacher", "--device_memory"]


def _refused(capsys, argv):
    with pytest.raises(SystemExit) as e:
        R.parse_flags(BASE + argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_the_parser_refuses_what_it_cannot_serve(capsys):
    assert "--kd_conf_gamma needs --soft_teacher" in _refused(capsys, ["--kd_conf_gamma", "2"])
    for bad in ("-1", "8.5", "nan", "inf"):
        assert "--kd_conf_gamma must lie in [0, 8]" in _refused(capsys, SOFT + ["--kd_conf_gamma", bad])
    assert "--loss_class_weights needs one weight per class" in _refused(capsys, ["--loss_class_weights", "1,2,3"])
    assert "--loss_class_weights must each be 0 or lie in" in _refused(capsys, ["--loss_class_weights", "1,1,1,1,1,32"])
    assert "--loss_class_weights must each be 0 or lie in" in _refused(capsys, ["--loss_class_weights", "1,1,1,1,1,0.001"])
    assert "--loss_class_weights must be 'balanced' or 6" in _refused(capsys, ["--loss_class_weights", "heavy"])
    flags = R.parse_flags(BASE + ["--loss_class_weights", "1,1,1,4,4,0"])           # class weights need no soft teacher
    assert flags.loss_class_weights == "1,1,1,4,4,0" and flags.kd_conf_gamma is None
    assert R.parse_flags(BASE + ["--loss_class_weights", "balanced"]).loss_class_weights == "balanced"
    flags = R.parse_flags(BASE + SOFT + ["--loss_class_weights", "balanced", "--kd_conf_gamma", "2"])
    assert flags.kd_conf_gamma == 2.0
    flags = R.parse_flags(BASE + SOFT)
    assert flags.loss_class_weights is None and flags.kd_conf_gamma is None          # nothing is passed on: ones and 0
    assert np.array_equal(R.parse_loss_class_weights("1,1,1,4,4,0.5", 6), np.float32([1, 1, 1, 4, 4, 0.5]))


# ---------------------------------------------------------------------------------------------------------
# SemanticNetwork's kwargs: the assertions stand in front of everything that needs a device
# ---------------------------------------------------------------------------------------------------------
KW = dict(class_weights_exp=exp_configs.class_weights(25), height=64, scale=[1], mini_batch_size=2, lr=1e-3, initial_variables={})


@pytest.mark.parametrize("kwargs,word", [(dict(kd_conf_gamma=2.0), "soft_teacher"),
                                         (dict(kd_conf_gamma=9.0, soft_teacher=True), "kd_conf_gamma"),
                                         (dict(kd_conf_gamma=float("nan"), soft_teacher=True), "kd_conf_gamma"),
                                         (dict(loss_class_weights=[1, 2, 3]), "loss_class_weights"),
                                         (dict(loss_class_weights=[1, 1, 1, 1, 1, 17]), "loss_class_weights"),
                                         (dict(loss_class_weights=[1, 1, 1, 1, 1, -1]), "loss_class_weights"),
                                         (dict(loss_class_weights=[1, 1, 1, 1, 1, float("nan")]), "loss_class_weights")])
def test_constructor_refuses_bad_loss_weight_kwargs(kwargs, word):
    with pytest.raises(AssertionError, match=word):
        SemanticNetwork("unused", **KW, **kwargs)


# ---------------------------------------------------------------------------------------------------------
# balanced_class_weights
# ---------------------------------------------------------------------------------------------------------
def test_balanced_class_weights_on_hand_worked_counts():
    # N = 1000, P = 4 present classes: 1000 / (4 n_k); the absent class gets 1
    cw = balanced_class_weights([500, 250, 0, 200, 50])
    assert cw.dtype == np.float32
    assert np.array_equal(cw, np.float32([0.5, 1.0, 1.0, 1.25, 5.0]))
    # a class of 3 pixels among a million: 1000003 / (2 * 3) is far above the cap of 16; the big class gets 1000003 / 2000000
    cw = balanced_class_weights([1000000, 3])
    assert cw[1] == 16.0 and cw[0] == np.float32(1000003 / 2000000)
    # the floor: 2^-6
    assert balanced_class_weights([10 ** 9, 10 ** 9, 10 ** 9] + [1] * 200)[0] == np.float32(2.0 ** -6)
    # a single class: N / (1 * N)
    assert np.array_equal(balanced_class_weights([0, 77, 0]), np.float32([1, 1, 1]))
    assert np.array_equal(balanced_class_weights([0, 0]), np.float32([1, 1]))
    # every value is one the setter takes
    cw = balanced_class_weights(np.random.default_rng(0).integers(0, 10 ** 6, 19))
    assert np.all((cw >= 2.0 ** -6) & (cw <= 16.0))


def test_label_class_counts_fold_labels_as_the_upload_does():
    labels = [np.array([[0, 1, 13, 255], [13, 13, 7, 300]], dtype=np.int32), np.array([[13, 0, 0, 2]], dtype=np.uint8)]
    assert np.array_equal(label_class_counts(labels, [0, 1, 2, 10, 11, 13]), [3, 1, 1, 0, 0, 4])


# ---------------------------------------------------------------------------------------------------------
# what the GPU tests lean on
# ---------------------------------------------------------------------------------------------------------
def test_weighted_objective_values_of_the_kernel_tests_first_shape_are_far_apart():
    """The f64 objective sum w pixel / sum w on the material of tests/test_gpu_weighted_loss.py's first kernel shape (5 x 9 -> 64 x 128, K = 6) under
    (ones, 0), (cw, 0) and (cw, 2), for the hard, soft and mix forms: every pair that a form can tell apart differs by more than ten times the 2e-5
    loss bar, so a kernel that ignored a knob could not pass."""
    import torch
    import loss_ref as WR
    from oracle.student_torch import resize_bilinear_align_corners
    h, w, H, W, NC, cls = 5, 9, 64, 128, 19, WR.CI
    logits, teacher, tl = WR.material(h, w, H, W, NC, H, W, seed=h * w + H)
    lut = np.full(256, -1)
    lut[cls] = np.arange(len(cls))
    valid = torch.as_tensor(lut[teacher] >= 0)
    y = torch.as_tensor(np.where(lut[teacher] >= 0, lut[teacher], 0).astype(np.int64))
    z = resize_bilinear_align_corners(torch.as_tensor(logits).double(), H, W)[..., cls]
    t = torch.as_tensor(tl).double()[..., cls]
    ones, cw = torch.ones(len(cls), dtype=torch.float64), torch.tensor(WR.CW6, dtype=torch.float64)
    for T, alpha in ((1.0, 0.0), (1.0, 1.0), (2.0, 0.5)):
        vals = [float(WR.objective(z, t, y, valid, T, alpha, c, g)[0]) for c, g in ((ones, 0.0), (cw, 0.0), (cw, 2.0))]
        for i, a in enumerate(vals):
            for b in vals[i + 1:]:
                assert abs(a - b) > 10 * 2e-5 * max(a, b), (T, alpha, vals)


def test_the_quantised_weight_is_exact_in_f32():
    """w_q = rint(w 2^20) 2^-20 for w <= 16: w 2^20 <= 2^24, so its rint is an integer f32 holds, and the scaling by 2^-20 is exact; w_q 2^20 is
    that integer again.  Checked on the edges, on every class weight the tests use and on a dense random draw."""
    rng = np.random.default_rng(1)
    w = np.concatenate([np.float32([0, 2.0 ** -6, 16, 1 / 36, 0.3, 1, 2, 4, 0.5, 15.999999, 2.0 ** -20, 2.0 ** -21]),
                        (rng.random(200000) * 16).astype(np.float32), (rng.random(200000) ** 8 * 16).astype(np.float32)])
    scaled = np.rint(w * np.float32(1048576.0))
    assert scaled.dtype == np.float32
    assert np.array_equal(scaled.astype(np.float64), np.rint(w.astype(np.float64) * 1048576.0))        # the f32 product and rint lose nothing
    wq = scaled * np.float32(1.0 / 1048576.0)
    assert np.array_equal(wq.astype(np.float64) * 1048576.0, scaled.astype(np.float64))
    assert np.array_equal(wq * np.float32(1048576.0), scaled)
    assert scaled.max() <= 2 ** 24 and np.abs(wq.astype(np.float64) - w.astype(np.float64)).max() <= 2.0 ** -21
