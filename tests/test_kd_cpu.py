"""The two KD knobs of the soft-teacher step (temperature, soft : hard mix) where no GPU is needed: the C ABI refuses invalid values before it
looks at any pointer, header and binding agree on the two new prototypes, run.py's parser and SemanticNetwork's constructor refuse the knobs
without soft_teacher."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from ams_amd import exp_configs, hip, run as R
from ams_amd.semantic_network import SemanticNetwork
from loss_ref import header_prototype

ROOT = Path(__file__).resolve().parent.parent
NULL = C.c_void_p(0)
E_INVALID = -1


def _kd_null_call(lib, temperature, alpha):
    """Every pointer null and every size 0: only a check of the two floats in front of everything else lets this return in order."""
    return lib.ams_k_ce_loss_grad_kd(NULL, 0, 0, 0, 0, 0, None, 0, 0, 0, NULL, NULL, 0, 0, 0, NULL, NULL, NULL, 0, NULL, temperature, alpha)


def test_error_code_is_the_headers():
    text = (ROOT / "include" / "ams_hip.h").read_text()
    assert int(re.search(r"\bAMS_E_INVALID\s*=\s*(-?\d+)", text).group(1)) == E_INVALID


@pytest.mark.parametrize("temperature", [0.0, -1.0, float("inf"), float("nan")])
def test_kernel_entry_refuses_a_bad_temperature_first(temperature):
    lib = hip.lib()
    assert _kd_null_call(lib, temperature, 0.5) == E_INVALID
    assert b"temperature" in lib.ams_last_error() and b"alpha" not in lib.ams_last_error()


@pytest.mark.parametrize("alpha", [-0.1, 1.1, float("nan")])
def test_kernel_entry_refuses_a_bad_alpha_first(alpha):
    lib = hip.lib()
    assert _kd_null_call(lib, 2.0, alpha) == E_INVALID
    assert b"alpha" in lib.ams_last_error() and b"temperature" not in lib.ams_last_error()


def test_valid_knobs_reach_the_pointer_checks():
    """With (2, 0.5) the same call is refused for its null teacher logits: the two floats were accepted, and still nothing was launched."""
    lib = hip.lib()
    assert _kd_null_call(lib, 2.0, 0.5) == E_INVALID
    assert b"teacher logits" in lib.ams_last_error()


def test_set_kd_on_a_null_student_fails_cleanly():
    lib = hip.lib()
    assert lib.ams_student_set_kd(NULL, 2.0, 0.5) == E_INVALID
    assert b"null student" in lib.ams_last_error()


@pytest.mark.parametrize("name", ["ams_student_set_kd", "ams_k_ce_loss_grad_kd"])
def test_header_and_binding_agree_on_the_prototypes(name):
    assert header_prototype(name) == tuple(hip.SIGNATURES[name])
    fn = getattr(hip.lib(), name)
    assert fn.restype is hip.SIGNATURES[name][0] and list(fn.argtypes) == hip.SIGNATURES[name][1]
    # the kd entry is the soft-layout entry with the two floats behind it
    if name == "ams_k_ce_loss_grad_kd":
        assert hip.SIGNATURES[name][1] == hip.SIGNATURES["ams_k_ce_loss_grad_soft_layout"][1] + [C.c_float, C.c_float]


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


def test_the_parser_refuses_kd_flags_without_soft_teacher_and_out_of_range(capsys):
    assert "--kd_alpha needs --soft_teacher" in _refused(capsys, ["--kd_alpha", "0.5"])
    assert "--kd_temperature needs --soft_teacher" in _refused(capsys, ["--kd_temperature", "2", "--device_memory"])
    for bad in ("0", "-1", "inf", "nan"):
        assert "--kd_temperature must be finite and > 0" in _refused(capsys, SOFT + ["--kd_temperature", bad])
    for bad in ("-0.1", "1.1", "nan"):
        assert "--kd_alpha must lie in [0, 1]" in _refused(capsys, SOFT + ["--kd_alpha", bad])
    flags = R.parse_flags(BASE + SOFT + ["--kd_temperature", "2", "--kd_alpha", "0.5"])
    assert (flags.kd_temperature, flags.kd_alpha) == (2.0, 0.5)
    flags = R.parse_flags(BASE + SOFT)
    assert flags.kd_temperature is None and flags.kd_alpha is None          # nothing is passed on: the constructor's defaults, (1, 1)
    assert R.parse_flags(BASE + SOFT + ["--kd_alpha", "0"]).kd_alpha == 0.0


# ---------------------------------------------------------------------------------------------------------
# SemanticNetwork's kwargs: the assertions stand in front of everything that needs a device
# ---------------------------------------------------------------------------------------------------------
KW = dict(class_weights_exp=exp_configs.class_weights(25), height=64, scale=[1], mini_batch_size=2, lr=1e-3, initial_variables={})


@pytest.mark.parametrize("kwargs", [dict(kd_alpha=0.5), dict(kd_temperature=2.0), dict(kd_temperature=2.0, kd_alpha=0.5, soft_teacher=False)])
def test_constructor_refuses_kd_kwargs_without_soft_teacher(kwargs):
    with pytest.raises(AssertionError, match="soft_teacher"):
        SemanticNetwork("unused", **KW, **kwargs)


@pytest.mark.parametrize("kwargs,word", [(dict(kd_temperature=0.0), "kd_temperature"), (dict(kd_temperature=float("nan")), "kd_temperature"),
                                         (dict(kd_alpha=1.5), "kd_alpha"), (dict(kd_alpha=float("nan")), "kd_alpha")])
def test_constructor_refuses_values_out_of_range(kwargs, word):
    with pytest.raises(AssertionError, match=word):
        SemanticNetwork("unused", soft_teacher=True, **KW, **kwargs)


def test_kd_objective_values_of_the_kernel_tests_first_shape_are_far_apart():
    """The f64 objective at the first shape of tests/test_gpu_kd_loss.py's kernel cases (random student logits, teacher = noise + a bump of 3):
    the (T, alpha) cases differ by far more than the 2e-5 loss bar, so a kernel that ignored either knob could not pass them."""
    import torch
    rng = np.random.default_rng(0)
    K, N = 6, 4096
    z = torch.as_tensor(2 * rng.standard_normal((N, K)))
    y = torch.as_tensor(rng.integers(0, K, N))
    t = torch.as_tensor(rng.standard_normal((N, K)))
    t[torch.arange(N), y] += 3.0

    def objective(T, alpha):
        p = torch.softmax(t / T, -1)
        soft = T * T * (p * (torch.logsumexp(z / T, -1, keepdim=True) - z / T)).sum(-1)
        hard = torch.logsumexp(z, -1) - z[torch.arange(N), y]
        return float((alpha * soft + (1 - alpha) * hard).mean())

    vals = [objective(*ta) for ta in ((1.0, 1.0), (2.0, 1.0), (2.0, 0.5), (0.5, 0.25), (4.0, 1.0))]
    for i, a in enumerate(vals):
        for b in vals[i + 1:]:
            assert abs(a - b) > 0.05 * max(a, b), vals
