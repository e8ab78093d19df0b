"""Hard-pixel mining, the parts that need no GPU: the header's prototypes against the binding, the rank rule and the warm-up schedule, the knobs
and flags refused in words, and the C-ABI refusals that return before a device is touched (in the style of test_loss_entry_refusals_cpu.py: every
call passes NULL student logits, labels and loss, so a row whose expected refusal went missing would still end in AMS_E_INVALID)."""
import ctypes as C

import numpy as np
import pytest

import loss_ref as LR
from ams_amd import hip
from ams_amd.utils import loss_knobs_problem, mining_fraction, mining_rank

NULL = C.c_void_p(0)
UNREAD = C.c_void_p(0x10000)          # non-null, 16-byte aligned, never dereferenced: the checks compare it against NULL and look at its low bits
E_INVALID = -1
CI = [0, 1, 2, 10, 11, 13]
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("name", ["ams_k_ce_loss_grad_mined", "ams_k_loss_mining_scratch", "ams_student_set_loss_mining", "ams_student_mining_result"])
def test_header_prototypes_are_the_bindings(name):
    assert LR.header_prototype(name) == hip.SIGNATURES[name]


def test_result_struct_and_scratch_size():
    assert C.sizeof(hip.MiningResult) == 32 and hip.MiningResult.valid.offset == 8 and hip.MiningResult.kept.offset == 24
    lib = hip.lib()
    n = 2 * 64 * 128
    assert lib.ams_k_loss_mining_scratch(2, 64, 128) == hip.MINING_KEYS_OFFSET + 4 * n + n
    assert lib.ams_k_loss_mining_scratch(1, 3, 5) == hip.MINING_KEYS_OFFSET + 64 + 16          # both maps rounded up to 16 bytes
    assert lib.ams_k_loss_mining_scratch(0, 64, 128) == 0 and lib.ams_k_loss_mining_scratch(2, -1, 128) == 0


def test_mining_rank():
    assert mining_rank(1e-9, 14745) == 1 and mining_rank(1e-3, 999) == 1 and mining_rank(0.25, 1) == 1 and mining_rank(0.25, 0) == 1
    assert mining_rank(0.25, 16384) == 4096 and mining_rank(0.5, 14745) == 7372 and mining_rank(0.25, 4095) == 1023 and mining_rank(0.625, 8) == 5
    assert mining_rank(1.0, 14745) == 14745 and mining_rank(1.0, 2 ** 31 - 1) == 2 ** 31 - 1
    # the fraction is the f32 the C ABI takes: 0.1 as f32 lies above 0.1, 0.3 as f32 above 0.3
    assert mining_rank(0.1, 10 ** 7) == int(np.floor(float(np.float32(0.1)) * 10 ** 7)) == 1000000
    assert mining_rank(0.3, 10 ** 8) == 30000001 and int(np.floor(0.3 * 10 ** 8)) == 30000000
    k, n = 3686, 14745
    assert mining_rank(np.float32((k + 0.5) / n), n) == k


def test_warmup_schedule():
    assert [mining_fraction(0.25, 2, it) for it in range(5)] == [1.0, 0.625, 0.25, 0.25, 0.25]
    assert [mining_fraction(0.25, 0, it) for it in range(3)] == [0.25] * 3
    assert [mining_fraction(0.5, 4, it) for it in range(6)] == [1.0, 0.875, 0.75, 0.625, 0.5, 0.5]
    assert mining_fraction(0.25, 200, 0) == 1.0 and mining_fraction(1.0, 0, 7) == 1.0


@pytest.mark.parametrize("kw,word", [(dict(loss_top_k=0.0), "loss_top_k must lie in (0, 1]"), (dict(loss_top_k=-0.5), "loss_top_k"),
                                     (dict(loss_top_k=1.5), "loss_top_k"), (dict(loss_top_k=NAN), "loss_top_k"), (dict(loss_top_k=INF), "loss_top_k"),
                                     (dict(loss_top_k=0.25, loss_top_k_warmup=-1), "loss_top_k_warmup"),
                                     (dict(loss_top_k=0.25, loss_top_k_warmup=1.5), "loss_top_k_warmup"),
                                     (dict(loss_top_k=0.25, loss_top_k_warmup=NAN), "loss_top_k_warmup"),
                                     (dict(loss_top_k_warmup=3), "needs loss_top_k < 1")])
def test_knobs_are_refused_in_words(kw, word):
    assert word in loss_knobs_problem(False, **kw)
    assert "--loss_top_k" in loss_knobs_problem(False, dash="--", **kw)


def test_knob_defaults_keep_the_callers_unchanged():
    assert loss_knobs_problem(False) is None and loss_knobs_problem(True, 2.0, 0.5, 2.0, [1.0] * 6, 6) is None
    assert loss_knobs_problem(False, loss_top_k=0.25, loss_top_k_warmup=2) is None and loss_knobs_problem(False, loss_top_k=1.0) is None
    assert "kd_alpha" in loss_knobs_problem(True, kd_alpha=1.5, loss_top_k=0.25)


BASE = ["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", "unused/", "--mode", "simple"]


@pytest.mark.parametrize("extra,word", [(["--loss_top_k", "0"], "--loss_top_k must lie in (0, 1]"), (["--loss_top_k", "1.25"], "--loss_top_k"),
                                        (["--loss_top_k", "nan"], "--loss_top_k"), (["--loss_top_k_warmup", "3"], "--loss_top_k_warmup needs --loss_top_k"),
                                        (["--loss_top_k", "0.25", "--loss_top_k_warmup", "-2"], "--loss_top_k_warmup"),
                                        (["--loss_top_k", "1", "--loss_top_k_warmup", "2"], "needs --loss_top_k < 1")])
def test_run_flags_are_refused_in_words(extra, word, capsys):
    from ams_amd import run as R
    with pytest.raises(SystemExit):
        R.parse_flags(BASE + extra)
    assert word in capsys.readouterr().err


def test_run_flags_are_parsed():
    from ams_amd import run as R
    f = R.parse_flags(BASE + ["--loss_top_k", "0.25", "--loss_top_k_warmup", "20"])
    assert f.loss_top_k == 0.25 and f.loss_top_k_warmup == 20
    f = R.parse_flags(BASE)
    assert f.loss_top_k is None and f.loss_top_k_warmup is None


# ---- the kernel-level entry: what it refuses, in which order, before anything is launched ----
def _args(**over):
    a = dict(B=2, h=5, w=9, ld=19, NC=19, cls=CI, K=6, H=64, W=128, tl=UNREAD, th=64, tw=128, layout=hip.TLOGITS_FULL, scratch=UNREAD, short=0,
             T=2.0, alpha=0.5, cw=None, gamma=0.0, top_k=0.25, labels_out=UNREAD, keys=NULL, result=UNREAD, mscratch=UNREAD, mshort=0)
    a.update(over)
    return a


def _call(a):
    lib = hip.lib()
    ci = (C.c_int32 * len(a["cls"]))(*a["cls"]) if a["cls"] is not None else None
    n = lib.ams_k_ce_loss_grad_scratch(a["B"], a["h"], a["w"], a["K"]) - a["short"]
    nm = lib.ams_k_loss_mining_scratch(a["B"], a["H"], a["W"]) - a["mshort"]
    cw = (C.c_float * len(a["cw"]))(*a["cw"]) if a["cw"] is not None else None
    return lib.ams_k_ce_loss_grad_mined(NULL, a["B"], a["h"], a["w"], a["ld"], a["NC"], ci, a["K"], a["H"], a["W"], NULL, a["tl"], a["th"], a["tw"],
                                        a["layout"], NULL, NULL, a["scratch"], n, NULL, C.c_float(a["T"]), C.c_float(a["alpha"]), cw,
                                        C.c_float(a["gamma"]), C.c_float(a["top_k"]), a["labels_out"], a["keys"], a["result"], a["mscratch"], nm)


# in the order of refusal: the weighted entry's own, then the mining's
FAULTS = {
    "temperature": (dict(T=0.0), b"temperature"),
    "alpha": (dict(alpha=1.5), b"alpha"),
    "gamma": (dict(gamma=9.0), b"conf_gamma"),
    "weight": (dict(cw=[1.0, NAN, 1.0, 1.0, 1.0, 1.0]), b"class_weights[1]"),
    "teacher_logits": (dict(tl=NULL), b"null teacher logits"),
    "class_table": (dict(cls=None), b"null class table"),
    "K": (dict(K=33), b"out of range"),
    "layout": (dict(layout=7), b"teacher-logit layout"),
    "stride": (dict(ld=18), b"row stride"),
    "geometry": (dict(w=2), b"one-pass"),
    "scratch": (dict(short=1), b"scratch too small"),
    "top_k": (dict(top_k=0.0), b"top_k"),
    "mining_scratch": (dict(mshort=1), b"mining scratch"),
    "outputs": (dict(result=NULL), b"null output"),
}
RANK = list(FAULTS)
MORE = [("top_k", dict(top_k=-0.25)), ("top_k", dict(top_k=1.5)), ("top_k", dict(top_k=NAN)), ("top_k", dict(top_k=INF)),
        ("mining_scratch", dict(mscratch=NULL)), ("mining_scratch", dict(mscratch=C.c_void_p(0x10008))), ("outputs", dict(labels_out=NULL)),
        ("outputs", dict(labels_out=NULL, top_k=1.0))]


def _refused(a, word):
    assert _call(a) == E_INVALID
    msg = hip.lib().ams_last_error()
    assert word in msg, msg
    return msg


@pytest.mark.parametrize("fault,over", [(f, FAULTS[f][0]) for f in RANK] + MORE, ids=lambda v: v if isinstance(v, str) else "")
def test_each_fault_is_refused_in_words(fault, over):
    _refused(_args(**over), FAULTS[fault][1])


@pytest.mark.parametrize("first,later", [(a, b) for i, a in enumerate(RANK) for b in RANK[i + 1:] if b in ("top_k", "mining_scratch", "outputs")])
def test_the_earlier_ranked_fault_wins(first, later):
    msg = _refused(_args(**dict(FAULTS[first][0], **FAULTS[later][0])), b"class weights" if (first, later) == ("weight", "K") else FAULTS[first][1])
    if first != "teacher_logits":
        assert FAULTS[later][1] not in msg, msg


@pytest.mark.parametrize("top_k", [0.25, 1.0])
def test_a_call_without_fault_reaches_the_null_checks(top_k):
    """Every check of the entry passes; the NULL student logits, labels and loss are refused in front of the first memset or launch."""
    _refused(_args(top_k=top_k), b"null pointer")


def test_the_student_entries_refuse_a_null_student():
    lib = hip.lib()
    assert lib.ams_student_set_loss_mining(None, 0.25, UNREAD, 1 << 30) == E_INVALID and b"null student" in lib.ams_last_error()
    r = hip.MiningResult()
    assert lib.ams_student_mining_result(None, C.byref(r), None) == E_INVALID and b"null pointer" in lib.ams_last_error()
