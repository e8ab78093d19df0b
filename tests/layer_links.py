"""The fine-tune step held link by link, teacher-forced.  TEST INFRASTRUCTURE ONLY (a helper module, not a conftest).

A free-running comparison of two evaluations of this graph (engine vs oracle) amplifies every ReLU6 mask flip through the chain of
training-mode BN backwards, which is why the end-to-end gradient bars are percent-level.  Here nothing runs free: every
intermediate tensor is taken from ONE run (the engine's own step, or a CPU oracle's as a stand-in), and for each layer only that layer's
link is recomputed in f64 from the run's own inputs to the link and compared with what the run wrote.  No error travels further than
one link, so the bars are f32 rounding and a wrong wire (a tensor from the wrong layer, a coefficient a few percent off, a padding parity
slip, a 1/HW applied twice) shows at full size.

The f64 side is built only from what oracle/student_torch.py provides (preprocess, conv_same, batch_norm_train, StudentOracle._act,
resize_bilinear_align_corners, ema_update, the loss functions) and the layer table of ams_amd.spec; every backward link is torch.autograd
over such a forward piece — no backward formula is restated by hand.

A run is a dict of f64 torch tensors, activations NCHW, layers keyed by their 1-based ``Layer.idx``:
    class_indices, frames [B,H,W,3], labels [B,H,W], teacher_logits (None: hard labels),
    params / grads {variable name: tensor} (params BEFORE the update), stats_before / stats_after {moving statistic name: tensor},
    z, a, dz, da {idx: tensor} (the pool branch's z / a are [B,C,1,1]), logits [B,num_classes,h,w], loss (CE sum, valid-pixel count),
    dlogits [B,num_classes,h,w] or absent.

Links of layer l, x = the stored output a of layer l-1 (the preprocessed frames for the stem; the global mean of the last backbone
layer's a for image_pooling; concat(broadcast image_pooling a, aspp0 a), pool branch first, for concat_projection):
    F1  z_l            against conv(x, W_l)                                        (logits: + bias, against the stored logits)
    F2  a_l            against act(BN_batch(z_l; gamma, beta, eps_l)) + stored a of residual_from
    F3  moving statistics after the step against the batch mean / unbiased variance of the stored z_l through the reference's decay
    L   CE sum, valid count (and dlogits where the run stores it) against the loss of the stored logits, resized and class-gathered
    B1  grads of W_l (and the logits bias) against autograd of <conv(x, W_l), dz_l> with the stored dz_l
    B2  dz_l, dgamma_l, dbeta_l against autograd through F2 from the stored z_l, the cotangent of a_l formed in f64 from the stored dz of
        every consumer (next layer's input gradient; the stored da of a residual block that reads a_l; for the last backbone layer aspp0's
        input gradient plus the pooled gradient broadcast with 1/HW); where the run keeps a true da (project layers of residual blocks)
        that da is checked on its own (link DA)

Two tensors of the head have no handle in the engine's C ABI (ams_student_layer_tensor / ams_student_region): dz of image_pooling and
dlogits.  Where a run does not store them they are derived in f64 one link further (dlogits from the stored logits through L, the pool
branch's dz through its B2 from the stored dz of concat_projection), so they are checked through every quantity that reads them
(logits weights and bias, concat_projection's dz, image_pooling's weights / dgamma / dbeta, the last backbone layer's dz) instead of
element by element.

MASKS.  B2 takes the activation mask from the run's own stored a_l (a > 0, and a < 6 for relu6), not from the f64 y.  The engine's
backward DOES form y = z * scale + shift with the same operations as its forward: bn_act_kernel, the BN-backward reduction (OpBnBwd) and
bn_bwd_apply_kernel (k_elementwise.hip) all call muladd4_pk(z, scale, shift) (common.hpp) on the same stored z, scale and shift, and
a = med3(y, 0, 6) is > 0 / < 6 exactly where y is.  So the mask of the stored a IS the mask backward used, no element is left out of
any comparison, and a single disagreeing element fails the dz link of its layer.

ERROR MEASURES (no others).  Elementwise tensors (z, a, dz, da, dlogits): max|got - ref| / max|ref| over the tensor.  Reduced quantities
(every GRADS slice, moving statistics, the CE sum): max_e |got_e - ref_e| / max_e S_e with S_e the f64 sum of the absolute values of the
terms of element e (sum |dy| for dbeta, sum |x||dz| for a weight gradient, ...) — dbeta of a project layer in front of a training-mode BN
is exactly 0 in real arithmetic, so its naive relative error is O(1) for any f32 evaluation.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np
import torch

from ams_amd import spec as S
from oracle.student_torch import (StudentOracle, batch_norm_train, conv_same, ema_update, preprocess,
                                  resize_bilinear_align_corners)

F64 = torch.float64
ELEMENTWISE_KINDS = ("conv_stem", "conv_dw", "conv_1x1", "bn_act", "dz", "da", "dlogits")
REDUCED_KINDS = ("wgrad", "dgamma", "dbeta", "stats", "loss")
KINDS = ELEMENTWISE_KINDS + REDUCED_KINDS

# Link kinds whose kernel family already has an f64 bar under the same (elementwise) measure in tests/test_gpu_kernels.py
KERNEL_BARS = {
    "conv_stem": (1e-5, "test_stem_conv"),
    "conv_dw": (1e-5, "test_depthwise_forward_and_backward"),
    "conv_1x1": (2e-5, "test_pointwise_forward"),
    "da": (2e-5, "test_pointwise_image_bias_and_transposed_weights"),          # the expand layer's input-gradient GEMM (transposed weights)
    "dlogits": (2e-5, "test_upsample_argmax_metrics_and_ce_grad"),
}
BAR_CAP = 1e-4            # anything above is a defect, not rounding

Result = namedtuple("Result", "link kind name err")


def bars_from_levels(levels: Dict[str, float]) -> Dict[str, Tuple[float, str]]:
    """kind -> (bar, where it comes from): the kernel family's own f64 bar where tests/test_gpu_kernels.py has one under the same measure,
    4 x the worst f32 CPU error of that kind otherwise (a different summation order and the 22-bit split products)."""
    out = {}
    for k in KINDS:
        if k in KERNEL_BARS:
            out[k] = (KERNEL_BARS[k][0], "tests/test_gpu_kernels.py::" + KERNEL_BARS[k][1])
        elif k in levels:
            out[k] = (4.0 * levels[k], "4 x f32 CPU level %.2e" % levels[k])
    assert all(b <= BAR_CAP for b, _ in out.values()), out
    return out


def elementwise_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def reduced_err(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor) -> float:
    assert got.shape == ref.shape == scale.shape, (got.shape, ref.shape, scale.shape)
    return float((got - ref).abs().max() / scale.max().clamp_min(1e-300))


def _leaf(t: torch.Tensor) -> torch.Tensor:
    return t.detach().clone().requires_grad_(True)


class Links:
    """Closes the links of one run.  ``close(plan)`` -> [Result]; ``plan`` None = every link of the step."""

    def __init__(self, run: dict, num_classes: int = 19):
        self.r = run
        self.spec = S.build_spec(num_classes)
        L = self.spec.layers
        self.by_idx = {l.idx: l for l in L}
        self.backbone = [l for l in L if l.scope.startswith("MobilenetV2")]
        self.nb = self.backbone[-1].idx
        self.lp, self.la, self.lc, self.ll = L[-4], L[-3], L[-2], L[-1]
        self.o = StudentOracle({**run["params"], **run["stats_before"]}, run["class_indices"], num_classes, dtype=F64)
        self._cache: dict = {}

    # ------------------------------------------------------------------ pieces
    def P(self, name: str) -> torch.Tensor:
        return self.r["params"][name]

    def x_in(self, l: S.Layer) -> torch.Tensor:
        a = self.r["a"]
        if l.idx == 1:
            return preprocess(self.r["frames"])
        if l is self.lp:
            return a[self.nb].mean(dim=(2, 3), keepdim=True)                       # node Mean
        if l is self.la:
            return a[self.nb]
        if l is self.lc:
            return self._concat(a[self.lp.idx], a[self.la.idx])
        return a[l.idx - 1]

    @staticmethod
    def _concat(pool_a: torch.Tensor, aspp_a: torch.Tensor) -> torch.Tensor:
        return torch.cat([pool_a.expand(-1, -1, aspp_a.shape[2], aspp_a.shape[3]), aspp_a], dim=1)     # concat_2: pool branch first

    def conv(self, l: S.Layer, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return conv_same(x, w, l.kind, l.stride, l.rate)

    def _bn(self, l: S.Layer, z, gamma, beta):
        return batch_norm_train(z, gamma, beta, l.bn_eps)

    def mask(self, l: S.Layer) -> torch.Tensor:
        a = self.r["a"][l.idx]
        if l.act == "relu6":
            return ((a > 0) & (a < 6)).to(F64)
        if l.act == "relu":
            return (a > 0).to(F64)
        return torch.ones_like(a)

    def _gb(self, l: S.Layer):
        return self.P(l.scope + "/BatchNorm/gamma:0"), self.P(l.scope + "/BatchNorm/beta:0")

    # ------------------------------------------------------------------ forward links
    def F1(self, l: S.Layer) -> List[Result]:
        ref = self.conv(l, self.x_in(l), self.P(l.weight_name))
        if l is self.ll:
            ref = ref + self.P(l.scope + "/biases:0").view(1, -1, 1, 1)
            got = self.r["logits"]
        else:
            got = self.r["z"][l.idx]
        kind = "conv_stem" if l.idx == 1 else "conv_dw" if l.kind == "dw" else "conv_1x1"
        return [Result("F1", kind, l.scope, elementwise_err(got, ref))]

    def F2(self, l: S.Layer) -> List[Result]:
        y, _, _ = self._bn(l, self.r["z"][l.idx], *self._gb(l))
        ref = StudentOracle._act(y, l.act)
        if l.residual_from is not None:
            ref = ref + self.r["a"][l.residual_from]
        return [Result("F2", "bn_act", l.scope, elementwise_err(self.r["a"][l.idx], ref))]

    def F3(self, l: S.Layer) -> List[Result]:
        z = self.r["z"][l.idx]
        _, mu, var_unbiased = self._bn(l, z, *self._gb(l))                         # what last_batch_stats feeds in the oracle
        omd = float(np.float32(1.0) - np.float32(S.BN_DECAY))
        mname, vname = l.scope + "/BatchNorm/moving_mean:0", l.scope + "/BatchNorm/moving_variance:0"
        m0, v0 = self.r["stats_before"][mname], self.r["stats_before"][vname]
        s_mean = m0.abs() * (1.0 - omd) + omd * z.abs().mean(dim=(0, 2, 3))
        s_var = v0.abs() * (1.0 - omd) + omd * var_unbiased                        # a sum of squares: every term is positive
        return [Result("F3", "stats", mname, reduced_err(self.r["stats_after"][mname], ema_update(m0, mu), s_mean)),
                Result("F3", "stats", vname, reduced_err(self.r["stats_after"][vname], ema_update(v0, var_unbiased), s_var))]

    # ------------------------------------------------------------------ loss
    def _loss(self):
        if "loss" not in self._cache:
            r, o = self.r, self.o
            low = _leaf(r["logits"].permute(0, 2, 3, 1))
            H, W = r["frames"].shape[1], r["frames"].shape[2]
            zsel = o.reduced_logits(resize_bilinear_align_corners(low, H, W))
            target, weight = o.label_targets(r["labels"])
            if r.get("teacher_logits") is not None:
                loss = o.soft_loss_from_reduced(zsel, o.soft_targets(r["teacher_logits"], H, W), weight)
            else:
                loss = o.loss_from_reduced(zsel, target, weight)
            count = int((weight > 0).sum())
            dlow = torch.autograd.grad(loss, low)[0].permute(0, 3, 1, 2)
            self._cache["loss"] = (loss.detach() * count, count, dlow)
        return self._cache["loss"]

    def L(self) -> List[Result]:
        ref_sum, count, dlow = self._loss()
        got_sum, got_count = self.r["loss"]
        # every pixel's cross entropy is >= 0, so the sum of the absolute values of the terms is the sum itself
        out = [Result("L", "loss", "CE sum", abs(float(got_sum) - float(ref_sum)) / float(ref_sum)),
               Result("L", "loss", "valid-pixel count", abs(float(got_count) - count))]
        if self.r.get("dlogits") is not None:
            out.append(Result("L", "dlogits", "dlogits", elementwise_err(self.r["dlogits"], dlow)))
        return out

    # ------------------------------------------------------------------ backward links
    def dz(self, idx: int) -> torch.Tensor:
        """The run's stored dz of layer idx; the two head tensors without an ABI handle are derived in f64 where the run has none."""
        if idx == self.ll.idx:
            return self.r["dlogits"] if self.r.get("dlogits") is not None else self._loss()[2]
        t = self.r["dz"].get(idx)
        if t is None:
            assert idx == self.lp.idx, "the run stores no dz of layer %d" % idx
            t = self._bn_backward(self.lp, self.cot_a(idx))[0]
        return t

    def cot_parts(self, idx: int) -> List[torch.Tensor]:
        """The cotangent of the stored a of layer idx as the list of its consumers' contributions."""
        a = self.r["a"]
        if idx in (self.lp.idx, self.la.idx):
            ap, aa = _leaf(a[self.lp.idx]), _leaf(a[self.la.idx])
            out = self.conv(self.lc, self._concat(ap, aa), self.P(self.lc.weight_name))
            gp, ga = torch.autograd.grad((out * self.dz(self.lc.idx)).sum(), [ap, aa])
            return [gp if idx == self.lp.idx else ga]
        x = _leaf(a[idx])
        if idx == self.nb:
            g_aspp = torch.autograd.grad((self.conv(self.la, x, self.P(self.la.weight_name)) * self.dz(self.la.idx)).sum(), x)[0]
            pooled = x.mean(dim=(2, 3), keepdim=True)
            g_pool = torch.autograd.grad((self.conv(self.lp, pooled, self.P(self.lp.weight_name)) * self.dz(self.lp.idx)).sum(), x)[0]
            return [g_aspp, g_pool]
        c = self.by_idx[idx + 1]
        parts = [torch.autograd.grad((self.conv(c, x, self.P(c.weight_name)) * self.dz(c.idx)).sum(), x)[0]]
        for rl in self.backbone:
            if rl.residual_from == idx:
                parts.append(self.r["da"][rl.idx])                                   # the skip gradient: that block's stored da
        return parts

    def cot_a(self, idx: int) -> torch.Tensor:
        if ("cot", idx) not in self._cache:
            self._cache[("cot", idx)] = sum(self.cot_parts(idx))
        return self._cache[("cot", idx)]

    def _bn_backward(self, l: S.Layer, cot: torch.Tensor):
        """autograd through F2 from the stored z_l with the stored a_l's mask -> (dz, dgamma, dbeta, S_gamma, S_beta)"""
        z = _leaf(self.r["z"][l.idx])
        gamma, beta = (_leaf(t) for t in self._gb(l))
        y, _, _ = self._bn(l, z, gamma, beta)
        mk = self.mask(l)
        dz, dg, db = torch.autograd.grad((y * mk * cot).sum(), [z, gamma, beta])
        with torch.no_grad():
            xhat, _, _ = self._bn(l, z, torch.ones_like(gamma), torch.zeros_like(beta))
            dy = cot * mk
            s_g, s_b = (dy * xhat).abs().sum(dim=(0, 2, 3)), dy.abs().sum(dim=(0, 2, 3))
        return dz, dg, db, s_g, s_b

    def B1(self, l: S.Layer) -> List[Result]:
        x, dz = self.x_in(l).detach(), self.dz(l.idx)
        w = _leaf(self.P(l.weight_name))
        ref = torch.autograd.grad((self.conv(l, x, w) * dz).sum(), w)[0]
        scale = torch.autograd.grad((self.conv(l, x.abs(), w) * dz.abs()).sum(), w)[0]
        out = [Result("B1", "wgrad", l.weight_name, reduced_err(self.r["grads"][l.weight_name], ref, scale))]
        if l is self.ll:
            name = l.scope + "/biases:0"
            out.append(Result("B1", "wgrad", name, reduced_err(self.r["grads"][name], dz.sum(dim=(0, 2, 3)), dz.abs().sum(dim=(0, 2, 3)))))
        return out

    def B2(self, l: S.Layer) -> List[Result]:
        dz, dg, db, s_g, s_b = self._bn_backward(l, self.cot_a(l.idx))
        out = []
        if self.r["dz"].get(l.idx) is not None:
            out.append(Result("B2", "dz", l.scope, elementwise_err(self.r["dz"][l.idx], dz)))
        gname, bname = l.scope + "/BatchNorm/gamma:0", l.scope + "/BatchNorm/beta:0"
        out.append(Result("B2", "dgamma", gname, reduced_err(self.r["grads"][gname], dg, s_g)))
        out.append(Result("B2", "dbeta", bname, reduced_err(self.r["grads"][bname], db, s_b)))
        return out

    def DA(self, l: S.Layer) -> List[Result]:
        return [Result("DA", "da", l.scope, elementwise_err(self.r["da"][l.idx], self.cot_a(l.idx)))]

    # ------------------------------------------------------------------ plans
    def full_plan(self) -> List[Tuple[str, int]]:
        plan = [("L", 0)]
        for l in self.spec.layers:
            plan += [("F1", l.idx), ("B1", l.idx)]
            if l.bn_eps is not None:
                plan += [("F2", l.idx), ("F3", l.idx), ("B2", l.idx)]
            if l.residual_from is not None:
                plan.append(("DA", l.idx))
        return plan

    def close(self, plan: Optional[Iterable[Tuple[str, int]]] = None) -> List[Result]:
        out: List[Result] = []
        for link, idx in (self.full_plan() if plan is None else plan):
            out += self.L() if link == "L" else getattr(self, link)(self.by_idx[idx])
        return out


def worst_by_kind(results: Iterable[Result]) -> Dict[str, Result]:
    worst: Dict[str, Result] = {}
    for r in results:
        if r.kind not in worst or not (r.err <= worst[r.kind].err):               # NaN counts as worst
            worst[r.kind] = r
    return worst


def failures(results: Iterable[Result], bars: Dict[str, Tuple[float, str]]) -> List[Result]:
    """every result over its kind's bar (the valid-pixel count must be exact)"""
    return [r for r in results if not (r.err <= (0.0 if r.name == "valid-pixel count" else bars[r.kind][0]))]


def report(results: Iterable[Result], bars: Optional[Dict[str, Tuple[float, str]]] = None) -> str:
    rows = []
    for k, r in sorted(worst_by_kind(results).items()):
        rows.append("%-9s worst %.2e  (%s %s)%s" % (k, r.err, r.link, r.name, "  bar %.2e: %s" % bars[k] if bars and k in bars else ""))
    return "\n".join(rows)


# ---------------------------------------------------------------------------------------------------------
# runs
# ---------------------------------------------------------------------------------------------------------
def _to64(t) -> torch.Tensor:
    return (t.detach() if torch.is_tensor(t) else torch.as_tensor(np.asarray(t))).to(F64)


def oracle_run(W: Dict[str, np.ndarray], class_indices, frames, labels, dtype, teacher_logits=None) -> dict:
    """One free-running step of the CPU oracle in ``dtype`` as a run: the stand-in for the engine.  The forward is the oracle's own
    (forward_lowres with its taps); the gradients with respect to z, to the a of the residual blocks' project layers and to the
    low-resolution logits come from one autograd call over that graph."""
    o = StudentOracle(W, class_indices, dtype=dtype)
    sp = o.spec
    params = dict(o.vars)
    leaves = {}
    for v in sp.trainable:
        leaves[v.name] = params[v.name] = o.vars[v.name].clone().requires_grad_(True)
    taps: Dict[str, torch.Tensor] = {}
    ztaps: Dict[str, torch.Tensor] = {}
    fr = torch.as_tensor(np.asarray(frames, dtype=np.float32)).to(dtype)
    low = o.forward_lowres(fr, "train", params, taps, ztaps)
    H, Wd = fr.shape[1], fr.shape[2]
    zsel = o.reduced_logits(resize_bilinear_align_corners(low, H, Wd))
    target, weight = o.label_targets(labels)
    if teacher_logits is not None:
        loss = o.soft_loss_from_reduced(zsel, o.soft_targets(teacher_logits, H, Wd), weight)
    else:
        loss = o.loss_from_reduced(zsel, target, weight)
    count = int((weight > 0).sum())
    backbone = [l for l in sp.layers if l.scope.startswith("MobilenetV2")]
    lp, la, lc = sp.layers[-4], sp.layers[-3], sp.layers[-2]
    zl = [l for l in sp.layers if l.scope in ztaps]
    rl = [l for l in backbone if l.residual_from is not None]
    a_graph = {l.idx: taps[l.scope]._base for l in backbone}             # the NCHW tensors the taps are views of: part of the graph
    g = torch.autograd.grad(loss, list(leaves.values()) + [ztaps[l.scope] for l in zl] + [a_graph[l.idx] for l in rl] + [low])
    n = len(leaves)
    run = {"class_indices": list(class_indices), "frames": _to64(fr), "labels": np.asarray(labels), "teacher_logits": teacher_logits,
           "params": {k: _to64(v) for k, v in o.vars.items() if k in leaves},
           "stats_before": {v.name: _to64(o.vars[v.name]) for v in sp.stats},
           "grads": {k: _to64(t) for k, t in zip(leaves, g[:n])},
           "z": {l.idx: _to64(ztaps[l.scope]) for l in zl},
           "a": {l.idx: _to64(taps[l.scope].permute(0, 3, 1, 2)) for l in sp.layers if l.scope in taps},
           "dz": {l.idx: _to64(t) for l, t in zip(zl, g[n:n + len(zl)])},
           "da": {l.idx: _to64(t) for l, t in zip(rl, g[n + len(zl):n + len(zl) + len(rl)])},
           "logits": _to64(low.permute(0, 3, 1, 2)), "dlogits": _to64(g[-1].permute(0, 3, 1, 2)),
           "loss": (float(loss.detach()) * count, count)}
    # the pool branch's raw conv output is no tap of the oracle: the same two operations on the same tensor give the same bits
    with torch.no_grad():
        pooled = a_graph[backbone[-1].idx].mean(dim=(2, 3), keepdim=True)
        run["z"][lp.idx] = _to64(torch.nn.functional.conv2d(pooled, o.vars[lp.weight_name].permute(3, 2, 0, 1)))
    run["stats_after"] = {}
    for l in sp.layers:
        if l.bn_eps is None:
            continue
        mu, var_unbiased = o.last_batch_stats[l.scope]
        for name, stat in ((l.scope + "/BatchNorm/moving_mean:0", mu), (l.scope + "/BatchNorm/moving_variance:0", var_unbiased)):
            run["stats_after"][name] = _to64(ema_update(o.vars[name], stat))
    return run


def copy_run(run: dict) -> dict:
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in run.items()}


# ---------------------------------------------------------------------------------------------------------
# the cases both test modules share, and the f32 reference levels the bars come from
# ---------------------------------------------------------------------------------------------------------
CI = [0, 1, 2, 10, 11, 13]
SIZES = ((64, 2), (62, 3), (34, 5))          # height (width = 2 x height), frames: even block inputs, even and odd ones (SAME pads differ), odd tiny maps
SOFT_GRID = (9, 17)
_memo: dict = {}


def case_weights() -> Dict[str, np.ndarray]:
    from ams_amd import weights
    if "W" not in _memo:
        _memo["W"] = weights.synthetic_weights(S.build_spec(), seed=3)
    return _memo["W"]


def case_clip(H: int, B: int):
    from ams_amd import synth
    return synth.SyntheticVideo(H, B, CI, seed=3).clip()


def case_teacher_logits(B: int) -> np.ndarray:
    return (np.random.default_rng(17).standard_normal((B,) + SOFT_GRID + (19,)) * 3).astype(np.float32)


def f32_run_results(H: int, B: int, soft: bool = False) -> List[Result]:
    """Every link (soft: link L only) closed on the f32 CPU oracle's own step of case (H, B); computed once per process."""
    key = ("f32", H, B, soft)
    if key not in _memo:
        frames, labels = case_clip(H, B)
        run = oracle_run(case_weights(), CI, frames, labels, torch.float32, teacher_logits=case_teacher_logits(B) if soft else None)
        _memo[key] = Links(run).close([("L", 0)] if soft else None)
    return _memo[key]


def f32_levels(sizes=SIZES, soft: bool = False) -> Dict[str, float]:
    """Worst error per link kind of the f32 CPU oracle's own step over ``sizes``: the f32 reference levels"""
    worst: Dict[str, float] = {}
    for H, B in sizes:
        for kind, r in worst_by_kind(f32_run_results(H, B, soft)).items():
            worst[kind] = max(worst.get(kind, 0.0), r.err)
    return worst


# ---------------------------------------------------------------------------------------------------------
# the engine's tensors
# ---------------------------------------------------------------------------------------------------------
def layer_view(eng, layer: int, which: int, B: int, h: int, w: int, c: int) -> np.ndarray:
    """Tensor ``which`` (0 z, 1 a, 2 da, 3 dz) of 1-based ``layer`` as f64 NHWC (ams_student_layer_tensor)"""
    from ams_amd import hip
    off, n = C.c_size_t(), C.c_size_t()
    hip.check(eng.lib.ams_student_layer_tensor(eng._h, layer, which, C.byref(off), C.byref(n)))
    assert B * h * w * c <= n.value
    return eng.arena[off.value:off.value + 4 * B * h * w * c].view(torch.float32).view(B, h, w, c).cpu().numpy().astype(np.float64)


def engine_run(eng, W: Dict[str, np.ndarray], class_indices, frames, labels, loss, teacher_logits=None) -> dict:
    """The tensors of the engine's last train_step as a run.  ``W``: the variables the step started from (Adam has changed the arena's);
    gradients and moving statistics are read from the arena (Adam touches neither); ``loss``: what train_step returned.
    Every layer tensor the ABI has a handle for is read; which of them a step wrote with their plain meaning is the caller's plan."""
    sp = eng.spec
    B = frames.shape[0]
    sizes = S.feature_sizes(frames.shape[1], frames.shape[2], sp.layers)
    nhwc = lambda t: torch.from_numpy(t).permute(0, 3, 1, 2).contiguous()  # noqa: E731
    g = eng.grads.cpu().numpy().astype(np.float64)
    st = eng.stats.cpu().numpy().astype(np.float64)
    ls = loss.cpu().numpy()
    h, w = eng.lowres
    run = {"class_indices": list(class_indices), "frames": _to64(np.asarray(frames, dtype=np.float32)),
           "labels": np.asarray(labels), "teacher_logits": teacher_logits,
           "params": {v.name: _to64(W[v.name]) for v in sp.trainable},
           "stats_before": {v.name: _to64(W[v.name]) for v in sp.stats},
           "stats_after": {v.name: torch.from_numpy(st[v.offset:v.offset + v.size].reshape(v.shape)) for v in sp.stats},
           "grads": {v.name: torch.from_numpy(g[v.offset:v.offset + v.size].reshape(v.shape)) for v in sp.trainable},
           "z": {}, "a": {}, "dz": {}, "da": {},
           "logits": nhwc(eng.logits_lowres.view(-1, h, w, 32)[:B, :, :, :sp.num_classes].cpu().numpy().astype(np.float64)),
           "loss": (float(ls[0]), float(ls[1]))}
    for l, (lh, lw) in zip(sp.layers, sizes):
        if l.bn_eps is None:
            continue                                                              # the logits layer lives in AMS_REGION_LOGITS
        shape = (B, lh, lw, l.cout)
        run["z"][l.idx] = nhwc(layer_view(eng, l.idx, 0, *shape))
        run["a"][l.idx] = nhwc(layer_view(eng, l.idx, 1, *shape))
        if l.scope == "image_pooling":
            continue                                                              # its da / dz live in buffers without a handle
        run["dz"][l.idx] = nhwc(layer_view(eng, l.idx, 3, *shape))
        if l.residual_from is not None:
            run["da"][l.idx] = nhwc(layer_view(eng, l.idx, 2, *shape))
    return run
