"""The weighted fine-tune loss: per-class weights cw_k and the teacher-confidence exponent gamma (this project's own objective).  Per valid
pixel, with pixel and d whatever the chosen form (hard, soft, soft at T, mix) computes, p = softmax(t / T) the form's target distribution:

    w = cw_y (max_k p_k)^gamma,      loss = sum w pixel / sum w,      dlogits = sum w d / sum w

Kernel level (ams_k_ce_loss_grad_weighted) against f64 autograd of that formula (for gamma = 0 on the hard form: torch's own weighted
cross_entropy), identities bit for bit, batch-split exactness of the loss pair, weight sums below 0.5, one fine-tune step against the f64
oracle's network, and the SemanticNetwork / scheduler surface."""
import glob
import os

import numpy as np
import pytest
import torch

import loss_ref as LR
from ams_amd import exp_configs, hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine
from ams_amd.replay import draw_samples
from ams_amd.semantic_network import SemanticNetwork
from loss_ref import CI, CW6, Q, rel_err, same

pytestmark = pytest.mark.gpu


def _call(lib, logits, teacher, tl, cls, NC, H, W, T, alpha, cw, gamma, layout=hip.TLOGITS_FULL):
    """ams_k_ce_loss_grad_weighted on host arrays: (loss pair, dlogits).  tl None = NULL teacher logits."""
    return LR.loss_call(lib, "weighted", logits, teacher, tl, cls, NC, H, W, T, alpha, cw, gamma, layout)


def _reference(logits, teacher, tl, cls, H, W, T, alpha, cw, gamma):
    """f64 autograd of the module head's formula: loss, d loss / d low-res logits, f64 sum of the quantised weights, and the summed absolute
    error of the weights an f32 NumPy restatement forms (0 at gamma = 0: the class weights are exact)."""
    from oracle.student_torch import resize_bilinear_align_corners
    valid_np, y_np = LR.targets(teacher, cls)
    valid, y = torch.as_tensor(valid_np), torch.as_tensor(y_np)
    lt = torch.as_tensor(logits).double().requires_grad_(True)
    z = resize_bilinear_align_corners(lt, H, W)[..., cls]
    t = None
    if tl is not None:
        t = torch.as_tensor(tl).double()
        if t.shape[1:3] != (H, W):
            t = resize_bilinear_align_corners(t, H, W)
        t = t[..., cls]
    cwt = torch.as_tensor(np.asarray(cw, dtype=np.float64))
    loss, _ = LR.objective(z, t, y, valid, T, alpha, cwt, gamma)
    loss.backward()
    w64 = LR.pixel_weights(t, y, cwt, T, gamma).numpy()[valid_np]
    sum_wq = float(LR.quantised(w64).sum())
    err32 = 0.0
    if gamma:
        # the f32 restatement starts from the teacher logits as an f32 program has them at the pixel: the f64 interpolation rounded to f32
        w32 = LR.weights_f32(t.numpy().astype(np.float32), y_np, cw, T, gamma)[valid_np]
        err32 = float(np.abs(LR.quantised(w32) - LR.quantised(w64)).sum())
    return float(loss.detach()), lt.grad.numpy(), sum_wq, err32, int(valid_np.sum())


SHAPE0 = (5, 9, 64, 128, 19, CI, 64, 128)
CW_ZERO = [1.0, 0.0, 1.0, 4.0, 4.0, 2.0]


def _drawn_weights(K):
    return np.random.default_rng(K).choice([0.5, 1.0, 2.0, 4.0], K).tolist()


# (shape, form, T, alpha, cw, gamma); form "hard" feeds no teacher logits
KERNEL_CASES = [
    (SHAPE0, "hard", 1.0, 0.0, CW6, 0.0),
    (SHAPE0, "soft", 1.0, 1.0, CW6, 0.0),
    (SHAPE0, "soft", 1.0, 1.0, [1.0] * 6, 1.0),
    (SHAPE0, "soft", 2.0, 0.5, CW6, 2.0),
    (SHAPE0, "soft", 1.0, 0.0, [1.0] * 6, 2.0),                          # alpha = 0, gamma = 2: the weighted mix form
    (SHAPE0, "soft", 2.0, 0.5, CW_ZERO, 0.0),
    (SHAPE0, "hard", 1.0, 0.0, CW_ZERO, 0.0),
    ((9, 17, 128, 256, 19, list(range(19)), 128, 256), "soft", 2.0, 0.5, _drawn_weights(19), 2.0),      # KMAX 20
    ((3, 5, 32, 64, 21, list(range(21)), 32, 64), "soft", 2.0, 0.5, _drawn_weights(21), 2.0),           # KMAX 32
    ((4, 7, 50, 90, 19, [0, 15], 13, 31), "soft", 2.0, 0.5, _drawn_weights(2), 2.0)]                   # odd sizes, a teacher off its grid points


@pytest.mark.parametrize("shape,form,T,alpha,cw,gamma", KERNEL_CASES)
def test_weighted_loss_and_gradient_kernel(shape, form, T, alpha, cw, gamma):
    """ams_k_ce_loss_grad_weighted against f64 autograd of the formula, with the bars of test_kd_loss_and_gradient_kernel: mean loss rel 2e-5,
    max |d - d64| / max |d64| < 3e-5, unselected columns exactly 0, two runs identical; loss[1] equals the f64 sum of the quantised weights
    exactly at gamma = 0.  With gamma > 0 the weight passes through an f32 exp / log before it is quantised, so loss[1] is held to four times the
    summed weight error of an f32 NumPy restatement on the same inputs (both figures are printed)."""
    h, w, H, W, NC, cls, th, tw = shape
    lib = hip.lib()
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    feed = tl if form == "soft" else None
    want, d64, sum_wq, err32, nvalid = _reference(logits, teacher, feed, cls, H, W, T, alpha, cw, gamma)
    outs = [_call(lib, logits, teacher, feed, cls, NC, H, W, T, alpha, cw, gamma) for _ in range(2)]
    got, d = outs[0]
    print("weighted kernel (%s, T=%g, alpha=%g, gamma=%g, K=%d): loss %.6f (f64 %.6f, rel %.2e), gradient err %.2e, sum w %.6f (f64 of w_q %.6f, "
          "off by %.3e; f32 restatement off by %.3e in summed |error|; %d valid pixels)"
          % (form, T, alpha, gamma, len(cls), got[0] / got[1], want, abs(got[0] / got[1] - want) / abs(want), rel_err(d, d64), got[1], sum_wq,
             abs(got[1] - sum_wq), err32, nvalid))
    if gamma == 0:
        assert got[1] == sum_wq
    else:
        assert abs(got[1] - sum_wq) <= 4 * err32
    assert got[1] * Q == np.rint(got[1] * Q)                          # an integer multiple of 2^-20
    assert got[0] / got[1] == pytest.approx(want, rel=2e-5)
    assert rel_err(d, d64) < 3e-5
    unsel = [c for c in range(NC) if c not in cls]
    assert np.all(d[..., unsel] == 0)
    assert same(outs[0], outs[1])


def test_hard_form_is_torchs_weighted_cross_entropy():
    """gamma = 0 on the hard form against torch.nn.functional.cross_entropy(weight=cw, ignore_index, reduction='mean') in f64."""
    from oracle.student_torch import resize_bilinear_align_corners
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, _ = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    valid, y = LR.targets(teacher, cls)
    lt = torch.as_tensor(logits).double().requires_grad_(True)
    z = resize_bilinear_align_corners(lt, H, W)[..., cls]
    target = torch.as_tensor(np.where(valid, y, -100))
    loss = torch.nn.functional.cross_entropy(z.reshape(-1, len(cls)), target.reshape(-1), weight=torch.tensor(CW6, dtype=torch.float64),
                                             ignore_index=-100, reduction="mean")
    loss.backward()
    got, d = _call(hip.lib(), logits, teacher, None, cls, NC, H, W, 1.0, 0.0, CW6, 0.0)
    print("hard form against torch's weighted cross_entropy: loss rel %.2e, gradient err %.2e"
          % (abs(got[0] / got[1] - float(loss.detach())) / float(loss.detach()), rel_err(d, lt.grad.numpy())))
    assert got[1] == float(np.asarray(CW6)[y][valid].sum())
    assert got[0] / got[1] == pytest.approx(float(loss.detach()), rel=2e-5)
    assert rel_err(d, lt.grad.numpy()) < 3e-5


def _existing(lib, logits, teacher, tl, cls, NC, H, W, kind, T=1.0, alpha=1.0):
    """The entry that served the form before the weighted one: ams_k_ce_loss_grad, _soft or _kd."""
    return LR.loss_call(lib, kind, logits, teacher, tl if kind != "hard" else None, cls, NC, H, W, T, alpha)


FORMS = [("hard", 1.0, 0.0), ("soft", 1.0, 1.0), ("kd", 2.0, 1.0), ("kd", 2.0, 0.5)]


def test_identities_bit_for_bit():
    """Ones with gamma = 0 through the new entry are the existing entries (all four forms); cw = 2 everywhere forces the weighted forms and scales
    by a power of two, which commutes with every rounding: the same dlogits bit for bit, twice the count, the mean loss within 2^-20; cw_k = 0
    is the same call with class k's labels rewritten to 255; the selected teacher layout is the full one under weights."""
    lib = hip.lib()
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    a = (lib, logits, teacher, tl, cls, NC, H, W)
    for kind, T, alpha in FORMS:
        old = _existing(*a, kind, T, alpha)
        assert same(_call(*a, T, alpha, [1.0] * 6, 0.0), old), kind
        assert same(_call(*a, T, alpha, None, 0.0), old), kind
        two = _call(*a, T, alpha, [2.0] * 6, 0.0)
        assert np.array_equal(two[1], old[1]), kind
        assert two[0][1] == 2 * old[0][1]
        assert abs(two[0][0] / two[0][1] - old[0][0] / old[0][1]) <= 2.0 ** -20
    # a class of weight 0 is a class of ignored labels
    k = 3
    relabelled = np.where(teacher == cls[k], 255, teacher).astype(np.uint8)
    cw_k0 = [c if i != k else 0.0 for i, c in enumerate(CW6)]
    for T, alpha, gamma in ((1.0, 0.0, 0.0), (2.0, 0.5, 2.0)):
        zero = _call(*a, T, alpha, cw_k0, gamma)
        gone = _call(lib, logits, relabelled, tl, cls, NC, H, W, T, alpha, CW6, gamma)
        assert same(zero, gone)
    # layouts
    full = _call(*a, 2.0, 0.5, CW6, 2.0)
    sel = np.ascontiguousarray(np.take(tl, cls, axis=-1))
    assert same(_call(lib, logits, teacher, sel, cls, NC, H, W, 2.0, 0.5, CW6, 2.0, layout=hip.TLOGITS_SELECTED), full)
    assert not same(full, _call(*a, 2.0, 0.5, CW6, 0.0)) and not same(full, _call(*a, 2.0, 0.5, [1.0] * 6, 2.0))


@pytest.mark.parametrize("T,alpha,gamma", [(1.0, 0.0, 0.0), (2.0, 0.5, 2.0)])
def test_loss_pair_is_exact_under_a_batch_split(T, alpha, gamma):
    """The pair of B = 2 equals the f64 sum of the two B = 1 pairs exactly: both members are sums of integer multiples of 2^-20."""
    lib = hip.lib()
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    both = _call(lib, logits, teacher, tl, cls, NC, H, W, T, alpha, CW6, gamma)[0]
    parts = [_call(lib, logits[b:b + 1], teacher[b:b + 1], tl[b:b + 1], cls, NC, H, W, T, alpha, CW6, gamma)[0] for b in range(2)]
    assert np.array_equal(both, parts[0] + parts[1])
    assert both[1] not in (parts[0][1], parts[1][1])


def test_weight_sums_below_one_half():
    """One valid pixel under gamma = 2 and a flat teacher: w = 1 / K^2, far below the 0.5 the combine kernel once compared against — a finite loss
    and a gradient that holds to the f64 reference.  All class weights 0: NaN loss and all-zero dlogits."""
    lib = hip.lib()
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    one = np.full_like(teacher, 255)
    one[1, 37, 71] = cls[4]
    flat = np.zeros_like(tl)
    want, d64, sum_wq, _err32, nvalid = _reference(logits, one, flat, cls, H, W, 2.0, 0.5, [1.0] * 6, 2.0)
    got, d = _call(lib, logits, one, flat, cls, NC, H, W, 2.0, 0.5, [1.0] * 6, 2.0)
    print("one pixel of weight %.8f: loss %.6f (f64 %.6f), gradient err %.2e" % (got[1], got[0] / got[1], want, rel_err(d, d64)))
    assert nvalid == 1 and got[1] == sum_wq == np.rint(Q / 36) / Q
    assert np.isfinite(got[0]) and got[0] / got[1] == pytest.approx(want, rel=2e-5)
    assert np.abs(d).max() > 0 and rel_err(d, d64) < 3e-5
    got, d = _call(lib, logits, teacher, tl, cls, NC, H, W, 2.0, 0.5, [0.0] * 6, 2.0)
    with np.errstate(invalid="ignore"):
        assert got[1] == 0 and np.isnan(got[0] / got[1])
    assert np.all(d == 0)


# ---------------------------------------------------------------------------------------------------------
# one fine-tune step
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


@pytest.mark.parametrize("low_res", [False, True])
def test_weighted_step_matches_f64_oracle(W0, low_res):
    """One step at 64 x 128, B = 2, under set_loss_weights(cw, 2) + set_kd(2, 0.5), teacher logits at the label size and on 9 x 17, with the bars of
    test_kd_step_matches_f64_oracle; then ones and gamma = 0 again: the step of an engine that never called the setter, bit for bit."""
    from oracle.student_torch import StudentOracle
    H, B, lr, T, alpha, gamma = 64, 2, 1e-3, 2.0, 0.5, 2.0
    frames, labels = synth.SyntheticVideo(H, B, CI, seed=5).clip()
    tl = LR.teacher_logits(labels.astype(np.int64), np.random.default_rng(17), th=9 if low_res else None, tw=17)
    f32 = frames.astype(np.float32)
    loss_o, sum_w, grads_o = LR.oracle_gradients(StudentOracle(W0, CI, dtype=torch.float64), f32, labels, tl, T, alpha, CW6, gamma)
    _, _, grads_32 = LR.oracle_gradients(StudentOracle(W0, CI), f32, labels, tl, T, alpha, CW6, gamma)
    loss_plain, _, _ = LR.oracle_gradients(StudentOracle(W0, CI, dtype=torch.float64), f32, labels, tl, T, alpha, [1.0] * 6, 0.0)
    eng = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W0)
    eng.set_soft_teacher(True)
    eng.set_kd(T, alpha)
    eng.set_loss_weights(CW6, gamma)
    ls = eng.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    g = eng.grads.cpu().numpy().astype(np.float64)
    flat = np.concatenate([grads_o[v.name].numpy().reshape(-1) for v in eng.spec.trainable])
    cos = float(g @ flat / (np.linalg.norm(g) * np.linalg.norm(flat)))
    print("weighted step: loss %.6f (f64 oracle %.6f; unweighted %.6f), sum w %.4f (f64 %.4f), cosine %.6f"
          % (ls[0] / ls[1], loss_o, loss_plain, ls[1], sum_w, cos))
    assert ls[0] / ls[1] == pytest.approx(loss_o, rel=1e-3)
    assert ls[1] == pytest.approx(sum_w, rel=1e-3) and ls[1] != float(np.isin(labels, CI).sum())
    assert cos > 0.9995, cos
    gnorm = max(float(gv.abs().max()) for gv in grads_o.values())
    for v in eng.spec.trainable:
        want = grads_o[v.name].numpy().reshape(-1)
        floor = max(np.linalg.norm(want), 1e-3 * gnorm * np.sqrt(want.size))
        e_gpu = np.linalg.norm(g[v.offset:v.offset + v.size] - want) / floor
        e_f32 = np.linalg.norm(grads_32[v.name].numpy().reshape(-1).astype(np.float64) - want) / floor
        assert e_gpu < max(6e-2, 4 * e_f32), (v.name, e_gpu, e_f32)
    # invalid values are refused and change nothing
    for bad in (([1.0] * 5, 0.0), ([1.0] * 5 + [17.0], 0.0), ([1.0] * 5 + [float("nan")], 0.0), ([1.0] * 5 + [0.001], 0.0), (CW6, 9.0), (CW6, float("nan"))):
        with pytest.raises(RuntimeError):
            eng.set_loss_weights(*bad)
    assert np.array_equal(eng.loss_class_weights, np.float32(CW6)) and eng.conf_gamma == gamma
    # back to ones and 0: the KD step of an engine that never heard of the weights
    eng.set_loss_weights(None, 0.0)
    eng.load_variables(W0)
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.adam_step = 0
    ls_1 = eng.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    fresh = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    fresh.load_variables(W0)
    fresh.set_soft_teacher(True)
    fresh.set_kd(T, alpha)
    ls_f = fresh.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    assert np.array_equal(ls_1, ls_f)
    a, b = eng.get_variables(), fresh.get_variables()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert torch.equal(eng.adam_m, fresh.adam_m) and torch.equal(eng.adam_v, fresh.adam_v)
    # gamma > 0 without soft teacher is refused in words, by the step
    fresh.set_soft_teacher(False)
    fresh.set_loss_weights(None, 2.0)
    with pytest.raises(RuntimeError, match="soft_teacher"):
        fresh.train_step(frames, labels, lr)
    eng.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------
# SemanticNetwork on a DeviceReplayMemory
# ---------------------------------------------------------------------------------------------------------
H, BATCH, ITERS, SLOTS, SEED, GRID = 64, 2, 3, 4, 3, (9, 17)


@pytest.mark.parametrize("weighted", [True, False], ids=["cw_gamma_2", "default"])
def test_semantic_network_weighted_phase_equals_hand_made_steps(W0, weighted):
    """SemanticNetwork(soft_teacher=True[, loss_class_weights=cw, kd_conf_gamma=2]) for three iterations on a replay memory of four 64 x 128 slots
    with 9 x 17 teacher logits, against engine.train_step on the same draws — on an engine under set_loss_weights(cw, 2), or, without the two
    kwargs, on one that never called the setter: every variable and last_losses equal bit for bit.  The memory's class histogram is the labels'."""
    mem, frames, labels, logits = LR.memory(np.random.default_rng(12), H, SLOTS, GRID)
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=BATCH, lr=1e-3, initial_variables=W0,
              soft_teacher=True)
    net = SemanticNetwork("unused", **kw, **(dict(loss_class_weights=CW6, kd_conf_gamma=2) if weighted else {}))
    from ams_amd.utils import label_class_counts
    counts = mem.class_counts(net)
    assert counts.dtype == np.int64 and np.array_equal(counts, label_class_counts(list(labels), net.class_indices_graph)) and counts.sum() > 0
    LR.seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    assert len(net.last_losses) == ITERS and all(np.isfinite(net.last_losses))
    LR.seed(SEED)
    desc = draw_samples(len(mem), (H, 2 * H), [H, 2 * H], [1], BATCH, ITERS, flip=False)
    eng = StudentEngine(net.class_indices_graph.tolist(), H, 2 * H, max_batch=BATCH, trainable=True)
    eng.load_variables(W0)
    eng.set_soft_teacher(True)
    if weighted:
        eng.set_loss_weights(CW6, 2.0)
    want = []
    for it in range(ITERS):
        picks = desc[it][:, 0]
        ls = eng.train_step(frames[picks], labels[picks], 1e-3, teacher_logits=logits[picks]).cpu().numpy()
        want.append(float(ls[0] / ls[1]))
    assert [float(x) for x in net.last_losses] == want
    a, b = net.get_vars(), eng.get_variables()
    assert all(np.array_equal(a[k], b[k]) for k in b), [k for k in b if not np.array_equal(a[k], b[k])][:5]
    assert torch.equal(net.engine.adam_m, eng.adam_m) and torch.equal(net.engine.adam_v, eng.adam_v)
    assert not np.array_equal(a["aspp0/weights:0"], W0["aspp0/weights:0"])
    net.close_model()
    eng.close()


# ---------------------------------------------------------------------------------------------------------
# the scheduler: --loss_class_weights balanced
# ---------------------------------------------------------------------------------------------------------
def test_scheduler_balanced_weights_on_host_deques_and_device_memory(tmp_path):
    """python -m ams_amd.run --loss_class_weights balanced on the same seeded 8-second clip (height 32) with the replay memory on the host and on
    the device: identical <results>_loss_weights.npy [phases, K]; against an unweighted run the other files keep their names, and the published
    model differs."""
    from ams_amd import run as R
    from ams_amd.semantic_network import FrozenGraph
    out = {}
    for tag, extra in (("plain", []), ("host", ["--loss_class_weights", "balanced"]), ("device", ["--loss_class_weights", "balanced", "--device_memory"])):
        out[tag] = str(tmp_path / tag) + "/"
        os.makedirs(out[tag])
        LR.seed(1)
        summary = R.main(["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", out[tag],
                          "--gpu", "0", "--mode", "simple", "--height", "32", "--batch_size", "2", "--iter", "1", "--send_period", "2",
                          "--train_period", "2", "--first_train_time", "2", "--memory_len", "4"] + extra)
        assert summary["frames"] == 16
    names = {tag: sorted(os.path.basename(p) for p in glob.glob(o + "*")) for tag, o in out.items()}
    assert not any(n.endswith("_loss_weights.npy") for n in names["plain"])
    assert [n for n in names["host"] if not n.endswith("_loss_weights.npy")] == names["plain"] and names["host"] == names["device"]

    def load(tag, suffix):
        hits = glob.glob(out[tag] + "*" + suffix)
        assert len(hits) == 1, hits
        return hits[0]

    wh, wd = np.load(load("host", "_loss_weights.npy")), np.load(load("device", "_loss_weights.npy"))
    assert wh.dtype == np.float32 and wh.ndim == 2 and wh.shape[1] == 6 and wh.shape[0] >= 2
    assert np.array_equal(wh, wd) and not np.all(wh == 1) and np.all((wh >= 2.0 ** -6) & (wh <= 16))
    models = {}
    for tag in ("plain", "host"):
        with open(load(tag, "_2_*_final.pb"), "rb") as f:
            models[tag] = FrozenGraph.ParseFromString(f.read()).variables
    assert any(not np.array_equal(models["plain"][k], models["host"][k]) for k in models["plain"])


def test_scheduler_soft_teacher_run_with_balanced_weights_and_gamma(tmp_path):
    """--device_memory --soft_teacher --loss_class_weights balanced --kd_conf_gamma 2 on the seeded clip completes and writes _loss_weights.npy
    beside the files of a soft-teacher run, with finite unweighted evaluation rows."""
    from ams_amd import run as R
    out = str(tmp_path / "soft") + "/"
    os.makedirs(out)
    LR.seed(1)
    summary = R.main(["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", out,
                      "--gpu", "0", "--mode", "simple", "--height", "32", "--batch_size", "2", "--iter", "1", "--send_period", "2",
                      "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--device_memory", "--soft_teacher",
                      "--loss_class_weights", "balanced", "--kd_conf_gamma", "2"])
    assert summary["frames"] == 16
    weights = glob.glob(out + "*_loss_weights.npy")
    soft = glob.glob(out + "*_soft_eval.npy")
    assert len(weights) == 1 and len(soft) == 1
    w, e = np.load(weights[0]), np.load(soft[0])
    assert w.shape == (e.shape[0], 6) and w.dtype == np.float32 and np.all((w >= 2.0 ** -6) & (w <= 16)) and np.isfinite(e[:, 1]).all()
