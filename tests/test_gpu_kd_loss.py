"""The soft-teacher step under a temperature T and a soft : hard mix alpha (this project's own objective; the reference's soft loss is T = 1,
alpha = 1).  Per valid pixel, z the student's K upsampled logits, t the teacher's, y the hard label's index in the subset:

    pixel = alpha T^2 sum_k softmax(t / T)_k (logsumexp(z / T) - z_k / T) + (1 - alpha) (logsumexp(z) - z_y),    loss = mean over the valid pixels

Kernel level (ams_k_ce_loss_grad_kd) against f64 autograd of that formula, the identities with the two existing kernels bit for bit, one
fine-tune step against the f64 oracle's network under the formula, and the SemanticNetwork surface on a DeviceReplayMemory."""
import numpy as np
import pytest
import torch

import loss_ref as LR
from ams_amd import exp_configs, hip, spec as S, synth, weights as Wt
from ams_amd.engine import StudentEngine
from ams_amd.replay import draw_samples
from ams_amd.semantic_network import SemanticNetwork
from loss_ref import CI, DEV, rel_err

pytestmark = pytest.mark.gpu


def _kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, T, alpha, layout=hip.TLOGITS_FULL):
    assert tuple(tld.shape[1:3]) == (th, tw)
    return LR.loss_call(lib, "kd", ld, td, tld, cls, NC, H, W, T, alpha, layout=layout)


SHAPE0 = (5, 9, 64, 128, 19, CI, 64, 128)
KERNEL_CASES = [SHAPE0 + ta for ta in ((2.0, 1.0), (2.0, 0.5), (0.5, 0.25), (4.0, 1.0))] + [
    (9, 17, 128, 256, 19, list(range(19)), 128, 256, 2.0, 0.5),          # KMAX 20
    (3, 5, 32, 64, 21, list(range(21)), 32, 64, 2.0, 0.5),               # KMAX 32
    (4, 7, 50, 90, 19, [0, 15], 13, 31, 2.0, 0.5),                       # odd sizes, a low-resolution teacher off its grid points
    (5, 9, 64, 128, 19, CI, 1, 1, 2.0, 1.0)]


@pytest.mark.parametrize("h,w,H,W,NC,cls,th,tw,T,alpha", KERNEL_CASES)
def test_kd_loss_and_gradient_kernel(h, w, H, W, NC, cls, th, tw, T, alpha):
    """ams_k_ce_loss_grad_kd against f64 autograd of the formula, with the bars of test_soft_teacher_loss_and_gradient_kernel (f32 __expf / __logf,
    2^-20 fixed-point loss): count, mean loss rel 2e-5, max |d - d64| / max |d64| < 3e-5, unselected columns exactly 0, run-to-run identical."""
    from oracle.student_torch import resize_bilinear_align_corners
    lib = hip.lib()
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    K = len(cls)
    valid, y = (torch.as_tensor(a) for a in LR.targets(teacher, cls))
    lt = torch.as_tensor(logits).double().requires_grad_(True)
    zf = resize_bilinear_align_corners(lt, H, W)[..., cls]
    tf_ = torch.as_tensor(tl).double()
    if (th, tw) != (H, W):
        tf_ = resize_bilinear_align_corners(tf_, H, W)
    objective, _ = LR.objective(zf, tf_[..., cls], y, valid, T, alpha)
    objective.backward()
    want = float(objective.detach())
    ld, td, tld = torch.as_tensor(logits).to(DEV), torch.as_tensor(teacher).to(DEV), torch.as_tensor(tl).to(DEV)
    outs = [_kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, T, alpha) for _ in range(2)]
    got, d = outs[0]
    print("kd kernel (T=%g, alpha=%g, K=%d): loss %.6f (f64 %.6f, rel %.2e), gradient err %.2e"
          % (T, alpha, K, got[0] / got[1], want, abs(got[0] / got[1] - want) / abs(want), rel_err(d, lt.grad.numpy())))
    assert got[1] == int(valid.sum())
    assert got[0] / got[1] == pytest.approx(want, rel=2e-5)
    assert rel_err(d, lt.grad.numpy()) < 3e-5
    unsel = [c for c in range(NC) if c not in cls]
    assert np.all(d[..., unsel] == 0)
    assert np.array_equal(d, outs[1][1]) and np.array_equal(got, outs[1][0])


def test_kd_identities_bit_for_bit():
    """(1, 1) is ams_k_ce_loss_grad_soft, alpha = 0 is ams_k_ce_loss_grad at any T, and the selected teacher layout is the full one."""
    lib = hip.lib()
    h, w, H, W, NC, cls, th, tw = SHAPE0
    logits, teacher, tl = LR.material(h, w, H, W, NC, th, tw, seed=h * w + th)
    ld, td, tld = torch.as_tensor(logits).to(DEV), torch.as_tensor(teacher).to(DEV), torch.as_tensor(tl).to(DEV)

    def existing(soft):
        return LR.loss_call(lib, "soft" if soft else "hard", ld, td, tld if soft else None, cls, NC, H, W)

    def same(a, b):
        return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    soft, hard = existing(True), existing(False)
    assert not same(soft, hard)
    assert same(_kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, 1.0, 1.0), soft)
    assert same(_kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, 2.0, 0.0), hard)
    assert same(_kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, 1.0, 0.0), hard)
    full = _kd_call(lib, ld, td, tld, cls, NC, H, W, th, tw, 2.0, 0.5)
    sel = torch.as_tensor(np.ascontiguousarray(np.take(tl, cls, axis=-1))).to(DEV)
    assert same(_kd_call(lib, ld, td, sel, cls, NC, H, W, th, tw, 2.0, 0.5, layout=hip.TLOGITS_SELECTED), full)
    assert not same(full, soft) and not same(full, hard)


# ---------------------------------------------------------------------------------------------------------
# one fine-tune step
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


@pytest.mark.parametrize("low_res", [False, True])
def test_kd_step_matches_f64_oracle(W0, low_res):
    """One step at 64 x 128 under set_kd(2, 0.5), teacher logits at the label size and on 9 x 17: the bars of
    test_soft_teacher_step_matches_f64_oracle; the objective is not the T = 1, alpha = 1 soft loss; set_kd(1, 1) is the soft step again, bit for bit."""
    from oracle.student_torch import StudentOracle
    H, B, lr, T, alpha = 64, 4, 1e-3, 2.0, 0.5
    frames, labels = synth.SyntheticVideo(H, B, CI, seed=5).clip()
    tl = LR.teacher_logits(labels.astype(np.int64), np.random.default_rng(17), th=9 if low_res else None, tw=17)
    f32 = frames.astype(np.float32)
    loss_o, _, grads_o = LR.oracle_gradients(StudentOracle(W0, CI, dtype=torch.float64), f32, labels, tl, T, alpha)
    _, _, grads_32 = LR.oracle_gradients(StudentOracle(W0, CI), f32, labels, tl, T, alpha)
    loss_soft, _ = StudentOracle(W0, CI, dtype=torch.float64).gradients(f32, labels, teacher_logits=tl)
    assert abs(loss_o - loss_soft) > 1e-2 * abs(loss_soft)
    eng = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W0)
    eng.set_soft_teacher(True)
    eng.set_kd(T, alpha)
    ls = eng.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    g = eng.grads.cpu().numpy().astype(np.float64)
    flat = np.concatenate([grads_o[v.name].numpy().reshape(-1) for v in eng.spec.trainable])
    cos = float(g @ flat / (np.linalg.norm(g) * np.linalg.norm(flat)))
    print("kd step: loss %.6f (f64 oracle %.6f; its T = 1 soft loss %.6f), cosine %.6f" % (ls[0] / ls[1], loss_o, loss_soft, cos))
    assert ls[0] / ls[1] == pytest.approx(loss_o, rel=1e-3)
    assert ls[1] == float(np.isin(labels, CI).sum())
    assert cos > 0.9995, cos
    gnorm = max(float(gv.abs().max()) for gv in grads_o.values())
    for v in eng.spec.trainable:
        want = grads_o[v.name].numpy().reshape(-1)
        floor = max(np.linalg.norm(want), 1e-3 * gnorm * np.sqrt(want.size))
        e_gpu = np.linalg.norm(g[v.offset:v.offset + v.size] - want) / floor
        e_f32 = np.linalg.norm(grads_32[v.name].numpy().reshape(-1).astype(np.float64) - want) / floor
        assert e_gpu < max(6e-2, 4 * e_f32), (v.name, e_gpu, e_f32)
    # invalid values are refused and change nothing
    for bad in ((0.0, 0.5), (float("nan"), 0.5), (2.0, 1.5)):
        with pytest.raises(RuntimeError):
            eng.set_kd(*bad)
    assert (eng.kd_temperature, eng.kd_alpha) == (T, alpha)
    # back to (1, 1): the soft step of an engine that never heard of the two knobs
    eng.set_kd(1.0, 1.0)
    eng.load_variables(W0)                      # the weights and statistics; the optimizer's state goes back to its start beside them
    eng.adam_m.zero_()
    eng.adam_v.zero_()
    eng.adam_step = 0
    ls_1 = eng.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    fresh = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    fresh.load_variables(W0)
    fresh.set_soft_teacher(True)
    ls_f = fresh.train_step(frames, labels, lr, teacher_logits=tl).cpu().numpy()
    assert np.array_equal(ls_1, ls_f)
    a, b = eng.get_variables(), fresh.get_variables()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert torch.equal(eng.adam_m, fresh.adam_m) and torch.equal(eng.adam_v, fresh.adam_v)
    eng.close()
    fresh.close()


# ---------------------------------------------------------------------------------------------------------
# SemanticNetwork on a DeviceReplayMemory
# ---------------------------------------------------------------------------------------------------------
H, BATCH, ITERS, SLOTS, SEED, GRID = 64, 2, 3, 4, 3, (9, 17)


@pytest.mark.parametrize("kd", [(2.0, 0.5), None], ids=["kd_2_0.5", "default"])
def test_semantic_network_kd_phase_equals_hand_made_steps(W0, kd):
    """SemanticNetwork(soft_teacher=True[, kd_temperature=2, kd_alpha=0.5]) for three iterations on a replay memory of four 64 x 128 slots with
    9 x 17 teacher logits, against engine.train_step on the same draws — on an engine under set_kd(2, 0.5), or, without the two kwargs, on one
    that never called set_kd: every variable and last_losses equal bit for bit."""
    mem, frames, labels, logits = LR.memory(np.random.default_rng(12), H, SLOTS, GRID)
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=BATCH, lr=1e-3, initial_variables=W0,
              soft_teacher=True)
    net = SemanticNetwork("unused", **kw, **(dict(kd_temperature=kd[0], kd_alpha=kd[1]) if kd else {}))
    LR.seed(SEED)
    net.train_with_deque(mem, None, ITERS)
    assert len(net.last_losses) == ITERS and all(np.isfinite(net.last_losses))
    LR.seed(SEED)
    desc = draw_samples(len(mem), (H, 2 * H), [H, 2 * H], [1], BATCH, ITERS, flip=False)
    ci = net.class_indices_graph.tolist()
    eng = StudentEngine(ci, H, 2 * H, max_batch=BATCH, trainable=True)
    eng.load_variables(W0)
    eng.set_soft_teacher(True)
    if kd:
        eng.set_kd(*kd)
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


def test_semantic_network_kd_kwargs_need_soft_teacher(W0):
    kw = dict(class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=BATCH, lr=1e-3, initial_variables=W0)
    with pytest.raises(AssertionError, match="soft_teacher"):
        SemanticNetwork("unused", kd_alpha=0.5, **kw)
    with pytest.raises(AssertionError, match="soft_teacher"):
        SemanticNetwork("unused", kd_temperature=2.0, **kw)


# ---------------------------------------------------------------------------------------------------------
# the scheduler: --kd_temperature / --kd_alpha
# ---------------------------------------------------------------------------------------------------------
def test_scheduler_run_with_kd_flags_writes_the_same_files_with_other_losses(tmp_path):
    """python -m ams_amd.run --soft_teacher --device_memory with and without --kd_temperature 2 --kd_alpha 0.5 on the same seeded 8-second clip
    (height 32, as tests/test_gpu_soft_scheduler.py): the same set of result files, other training losses, another published model."""
    import glob
    import os
    from ams_amd import run as R
    from ams_amd.semantic_network import FrozenGraph
    out = {}
    for tag, extra in (("soft", []), ("kd", ["--kd_temperature", "2", "--kd_alpha", "0.5"])):
        out[tag] = str(tmp_path / tag) + "/"
        os.makedirs(out[tag])
        LR.seed(1)
        summary = R.main(["--input_video", "synthetic:25-synth:seconds=8:fps=2", "--student_checkpoint", "synthetic:0", "--output_dir", out[tag],
                          "--gpu", "0", "--mode", "simple", "--height", "32", "--batch_size", "2", "--iter", "1", "--send_period", "2",
                          "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--device_memory", "--soft_teacher"] + extra)
        assert summary["frames"] == 16
    names = {tag: sorted(os.path.basename(p) for p in glob.glob(o + "*")) for tag, o in out.items()}
    assert names["soft"] == names["kd"] and any(n.endswith("_soft_eval.npy") for n in names["kd"]) and any(n.endswith("_loss.npy") for n in names["kd"])

    def load(tag, suffix):
        hits = glob.glob(out[tag] + "*" + suffix)
        assert len(hits) == 1, hits
        return hits[0]

    ls, lk = np.load(load("soft", "_loss.npy")), np.load(load("kd", "_loss.npy"))
    assert ls.shape == lk.shape and np.isfinite(lk).all() and not np.array_equal(ls, lk)
    models = {}
    for tag in out:
        with open(load(tag, "_2_*_final.pb"), "rb") as f:
            models[tag] = FrozenGraph.ParseFromString(f.read()).variables
    assert any(not np.array_equal(models["soft"][k], models["kd"][k]) for k in models["soft"])
