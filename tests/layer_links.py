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

WITHHELD TENSORS.  The default (fused) step stores only some of z, a, da, dz (default_step_stored gives the set with the engine's source
line behind each rule).  ``Links(run, stored=...)`` reads only those entries; ``z(idx)``, ``a(idx)``, ``da(idx)`` and ``dz(idx)`` return
the stored tensor or derive it in f64 from the nearest stored one: z by the conv of the a in front, a as act(BN_batch(z)), dz by
autograd through F2 from the cotangent of its consumers (as dlogits and the pool branch's dz above).  A link then closes across the
withheld tensors (composite_plan): the depthwise z of a recompute block against conv(act(BN(conv(stored block input)))), the expand
weight gradient of that block through the derived dz_e, and so on.  Nothing is compared that the run did not write; every gradient
tensor and moving statistic of the step is compared in one of the two plans.

MASKS OF WITHHELD ACTIVATIONS (resolved_mask).  Where a_l is withheld the mask comes from the f64 y = BN_batch(z_l).  An element with
|y - knee| <= tau_l (knee 0, and 6 for relu6) is ambiguous: the run may have put it on either side, and its bit is an unknown of the run.
tau_l = 8 x the largest |y_f32 - y_f64| the f32 CPU oracle's own step shows at that layer under the same derivation (f32_bands): from
the reference, never from the engine; the 8 is for the engine's other summation order and its 22-bit split products.  The backward is
linear in the mask, so per channel the assignment of its few ambiguous bits that best fits the run's (dgamma_c, dbeta_c) is taken (one
autograd call per bit), and EVERY quantity that depends on the mask (dgamma, dbeta, dz, the weight gradient through a derived dz, the
input gradient) is then compared under that one assignment: no element is left out or given slack.  More than 64 ambiguous elements in a
layer, more than 1e-4 of its elements or more than 8 in one channel fail the run.

THE DATA-PARALLEL STEP (tests/test_gpu_dp_links.py) is held by the same links.  With an all-reduce the engine takes other launches (the
reductions' second stages stop at the f64 sums, the cross-rank sum, then separate finalize / coefficient kernels; dgamma / dbeta from
the local sums) and mixes local row counts with global ones.  One rank with a reduce function that does nothing (or a one-rank RCCL
communicator) is such a step whose run is a plain run.  Two ranks each leave a run of their own shard: z, a, dz, da, logits of their
frames, but grads, moving statistics and loss of the whole batch, the same bits on every rank.  ``join_rank_runs`` asserts that
invariant and concatenates the shards into the run of the global batch, and the links then close over it exactly as over a
single-process run: F2 / F3 / B2 fail on statistics or coefficients formed from one rank's rows, B1 and dgamma / dbeta on gradients
that were not summed, or summed twice.  The bars are the f32 CPU oracle's at the GLOBAL size, by the same rule.

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

    def __init__(self, run: dict, num_classes: int = 19, stored: Optional[Iterable[Tuple[str, int]]] = None,
                 bands: Optional[Dict[int, float]] = None):
        """``stored``: the (kind, idx) entries of the run that hold their plain meaning (None: whatever the run's dicts have); every other
        tensor is derived in f64 from the nearest stored one.  ``bands``: {idx: tau} of the layers whose a may be withheld (f32_bands)."""
        self.r = run
        self.stored = None if stored is None else frozenset(stored)
        self.bands = dict(bands or {})
        self.ambiguous: Dict[int, dict] = {}          # idx -> what resolving that layer's mask met (resolved_mask)
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

    def has(self, kind: str, idx: int) -> bool:
        """the run holds tensor ``kind`` ('z', 'a', 'da', 'dz'; 'dy': see default_step_stored) of layer idx with its plain meaning"""
        if self.stored is not None:
            return (kind, idx) in self.stored
        return self.r.get(kind, {}).get(idx) is not None

    def z(self, idx: int) -> torch.Tensor:
        """the stored z of layer idx, or the conv of the stored or derived a in front of it"""
        if self.has("z", idx):
            return self.r["z"][idx]
        if ("z", idx) not in self._cache:
            l = self.by_idx[idx]
            self._cache[("z", idx)] = self.conv(l, self.x_in(l), self.P(l.weight_name))
        return self._cache[("z", idx)]

    def a(self, idx: int) -> torch.Tensor:
        """the stored a of layer idx, or act(BN_batch(z)) (+ the a of residual_from) of the stored or derived z"""
        if self.has("a", idx):
            return self.r["a"][idx]
        if ("a", idx) not in self._cache:
            l = self.by_idx[idx]
            y, _, _ = self._bn(l, self.z(idx), *self._gb(l))
            t = StudentOracle._act(y, l.act)
            self._cache[("a", idx)] = t if l.residual_from is None else t + self.a(l.residual_from)
        return self._cache[("a", idx)]

    def da(self, idx: int) -> torch.Tensor:
        return self.r["da"][idx] if self.has("da", idx) else self.cot_a(idx)

    def x_in(self, l: S.Layer) -> torch.Tensor:
        if l.idx == 1:
            return preprocess(self.r["frames"])
        if l is self.lp:
            return self.a(self.nb).mean(dim=(2, 3), keepdim=True)                  # node Mean
        if l is self.la:
            return self.a(self.nb)
        if l is self.lc:
            return self._concat(self.a(self.lp.idx), self.a(self.la.idx))
        return self.a(l.idx - 1)

    @staticmethod
    def _concat(pool_a: torch.Tensor, aspp_a: torch.Tensor) -> torch.Tensor:
        return torch.cat([pool_a.expand(-1, -1, aspp_a.shape[2], aspp_a.shape[3]), aspp_a], dim=1)     # concat_2: pool branch first

    def conv(self, l: S.Layer, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        return conv_same(x, w, l.kind, l.stride, l.rate)

    def _bn(self, l: S.Layer, z, gamma, beta):
        return batch_norm_train(z, gamma, beta, l.bn_eps)

    def mask(self, l: S.Layer) -> torch.Tensor:
        if l.act not in ("relu", "relu6"):
            return torch.ones_like(self.z(l.idx))
        if not self.has("a", l.idx):
            return self.resolved_mask(l)
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
        y, _, _ = self._bn(l, self.z(l.idx), *self._gb(l))
        ref = StudentOracle._act(y, l.act)
        if l.residual_from is not None:
            ref = ref + self.a(l.residual_from)
        return [Result("F2", "bn_act", l.scope, elementwise_err(self.r["a"][l.idx], ref))]

    def F3(self, l: S.Layer) -> List[Result]:
        z = self.z(l.idx)
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
        if self.has("dz", idx):
            return self.r["dz"][idx]
        # a run that declares nothing derives only the head tensor without a handle: any other missing dz is a mistake of the run
        assert self.stored is not None or idx == self.lp.idx, "the run stores no dz of layer %d" % idx
        if ("dz", idx) not in self._cache:                                         # one link further: autograd through F2 from its consumers' cotangent
            self._cache[("dz", idx)] = self._bn_backward(self.by_idx[idx], self.cot_a(idx))[0]
        return self._cache[("dz", idx)]

    def cot_parts(self, idx: int) -> List[torch.Tensor]:
        """The cotangent of the stored a of layer idx as the list of its consumers' contributions."""
        if idx in (self.lp.idx, self.la.idx):
            ap, aa = _leaf(self.a(self.lp.idx)), _leaf(self.a(self.la.idx))
            out = self.conv(self.lc, self._concat(ap, aa), self.P(self.lc.weight_name))
            gp, ga = torch.autograd.grad((out * self.dz(self.lc.idx)).sum(), [ap, aa])
            return [gp if idx == self.lp.idx else ga]
        x = _leaf(self.a(idx))
        if idx == self.nb:
            g_aspp = torch.autograd.grad((self.conv(self.la, x, self.P(self.la.weight_name)) * self.dz(self.la.idx)).sum(), x)[0]
            pooled = x.mean(dim=(2, 3), keepdim=True)
            g_pool = torch.autograd.grad((self.conv(self.lp, pooled, self.P(self.lp.weight_name)) * self.dz(self.lp.idx)).sum(), x)[0]
            return [g_aspp, g_pool]
        c = self.by_idx[idx + 1]
        parts = [torch.autograd.grad((self.conv(c, x, self.P(c.weight_name)) * self.dz(c.idx)).sum(), x)[0]]
        for rl in self.backbone:
            if rl.residual_from == idx:
                parts.append(self.da(rl.idx))                                        # the skip gradient: that block's stored da
        return parts

    def cot_a(self, idx: int) -> torch.Tensor:
        if ("cot", idx) not in self._cache:
            self._cache[("cot", idx)] = sum(self.cot_parts(idx))
        return self._cache[("cot", idx)]

    def _bn_backward(self, l: S.Layer, cot: torch.Tensor):
        """autograd through F2 from the stored z_l with the stored a_l's mask -> (dz, dgamma, dbeta, S_gamma, S_beta)"""
        mk = self.mask(l)
        z = _leaf(self.z(l.idx))
        gamma, beta = (_leaf(t) for t in self._gb(l))
        y, _, _ = self._bn(l, z, gamma, beta)
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
        if self.has("dz", l.idx):
            out.append(Result("B2", "dz", l.scope, elementwise_err(self.r["dz"][l.idx], dz)))
        elif self.has("dy", l.idx):
            # the handle holds dy = da * act': the apply pass ran inside the depthwise backward kernel and dz was never formed
            # (default_step_stored decides dy or dz per layer from the engine's predicates; a step that fell back to dz fails here)
            out.append(Result("B2", "dz", l.scope + " (dy)", elementwise_err(self.r["dz"][l.idx], self.cot_a(l.idx) * self.mask(l))))
        gname, bname = l.scope + "/BatchNorm/gamma:0", l.scope + "/BatchNorm/beta:0"
        out.append(Result("B2", "dgamma", gname, reduced_err(self.r["grads"][gname], dg, s_g)))
        out.append(Result("B2", "dbeta", bname, reduced_err(self.r["grads"][bname], db, s_b)))
        return out

    def DA(self, l: S.Layer) -> List[Result]:
        return [Result("DA", "da", l.scope, elementwise_err(self.r["da"][l.idx], self.cot_a(l.idx)))]

    # ------------------------------------------------------------------ the mask of an activation that is not stored
    def resolved_mask(self, l: S.Layer) -> torch.Tensor:
        """The mask of layer l from the f64 y = BN_batch(z_l).  An element within bands[l.idx] of a knee (0; 6 for relu6) is ambiguous: its
        bit is an unknown of the run.  dgamma_c and dbeta_c are linear in the mask, so the contribution of every ambiguous element to
        them is one autograd call on its channel; per channel the assignment of its bits that best fits the run's (dgamma_c, dbeta_c)
        (ties: the fewest bits away from the f64 mask) is taken, and every quantity of the link is then compared under that ONE mask.
        A layer with more than 64 ambiguous elements, more than 1e-4 of its elements or more than 8 in one channel fails."""
        if ("mask", l.idx) in self._cache:
            return self._cache[("mask", l.idx)]
        z = self.z(l.idx)
        gamma, beta = self._gb(l)
        with torch.no_grad():
            y, _, _ = self._bn(l, z, gamma, beta)
        knees = (0.0, 6.0) if l.act == "relu6" else (0.0,)
        base = (y > 0) & (y < 6) if l.act == "relu6" else (y > 0)
        tau = float(self.bands.get(l.idx, 0.0))
        dist = torch.stack([(y - k).abs() for k in knees]).min(dim=0).values
        amb = dist <= tau
        n_amb = int(amb.sum())
        per_channel = amb.sum(dim=(0, 2, 3))
        info = {"tau": tau, "ambiguous": n_amb, "share": n_amb / y.numel(), "per_channel": int(per_channel.max()), "resolved": 0,
                "nearest": float(dist.min())}
        self.ambiguous[l.idx] = info
        assert n_amb <= 64 and info["share"] <= 1e-4 and info["per_channel"] <= 8, \
            "%s: %d elements within %.2e of a knee (%.2e of the layer, %d in one channel)" % (l.scope, n_amb, tau, info["share"], info["per_channel"])
        mk = base.to(F64)
        if n_amb:
            cot = self.cot_a(l.idx)
            gname, bname = l.scope + "/BatchNorm/gamma:0", l.scope + "/BatchNorm/beta:0"
            for c in torch.nonzero(per_channel).flatten().tolist():
                zc, cc = z[:, c:c + 1], cot[:, c:c + 1]

                def part(m):                                                     # (dgamma_c, dbeta_c) of mask m, and the sums of |terms|
                    g, b = _leaf(gamma[c:c + 1]), _leaf(beta[c:c + 1])
                    yc, _, _ = self._bn(l, zc, g, b)
                    dg, db = torch.autograd.grad((yc * m * cc).sum(), [g, b])
                    return torch.stack([dg[0], db[0]])
                where = torch.nonzero(amb[:, c:c + 1])
                fixed = (base[:, c:c + 1] & ~amb[:, c:c + 1]).to(F64)
                p0 = part(fixed)
                bits = []
                for i in where.tolist():
                    e = torch.zeros_like(fixed)
                    e[tuple(i)] = 1.0
                    bits.append(part(e))
                with torch.no_grad():
                    xhat, _, _ = self._bn(l, zc, torch.ones(1, dtype=F64), torch.zeros(1, dtype=F64))
                    scale = torch.stack([(cc * xhat).abs().sum(), cc.abs().sum()]).clamp_min(1e-300)
                got = torch.stack([self.r["grads"][gname][c], self.r["grads"][bname][c]])
                f64_bits = [bool(base[:, c:c + 1][tuple(i)]) for i in where.tolist()]
                best = None
                for code in range(1 << len(bits)):
                    on = [bool(code >> k & 1) for k in range(len(bits))]
                    pred = p0 + sum((bits[k] for k in range(len(bits)) if on[k]), torch.zeros(2, dtype=F64))
                    cost = (float(((pred - got).abs() / scale).max()), sum(a != b for a, b in zip(on, f64_bits)))
                    if best is None or cost < best[0]:
                        best = (cost, on)
                for i, bit, was in zip(where.tolist(), best[1], f64_bits):
                    mk[:, c:c + 1][tuple(i)] = float(bit)
                    info["resolved"] += int(bit != was)
        self._cache[("mask", l.idx)] = mk
        return mk

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


# ---------------------------------------------------------------------------------------------------------
# what the default (fused) step stores, and the links that close across what it does not
# ---------------------------------------------------------------------------------------------------------
def recompute_expand(spec) -> set:
    """idx of the expand layers of the recompute blocks, expanded_conv_1 .. _6 (train_recompute_block, engine_forward.hip:508-516:
    xdw_train_supported = block input of 8 .. 32 channels, a multiple of 4)"""
    return {l.idx for l in spec.layers if l.scope.startswith("MobilenetV2") and l.scope.endswith("/expand") and 8 <= l.cin <= 32 and l.cin % 4 == 0}


def default_step_stored(spec, H: int, B: int) -> frozenset:
    """The (kind, idx) entries the DEFAULT step (train_recompute 2, fuse_dgrad_bn 3, fuse_gemm_red 3, fuse_operand_bn 1; default product
    mode) writes with their plain meaning on B frames of H x 2H, from the layer table and the case's size alone.  Each rule mirrors a
    predicate of the engine (scratch sizes are taken to fit):

      z   every BN layer but the recompute blocks' expand layers: train_recompute_block (engine_forward.hip:508-516) sends the block
          through launch_expand_dw, which writes the depthwise z only (:641-678)
      a   the project layers (:708 act_pass: role project, and operand_bn_act is false for them) and image_pooling, aspp0,
          concat_projection (:718, :725, :729).  NOT the stem (stem_fused_train :530-535 makes dw_fused_train_fwd(2) true, :636), NOT the
          late expand layers (dw_fused_train :521-527 / dw_fused_train_fwd :536-540: stride-1 depthwise behind an expand layer outside a
          recompute block, :708), NOT any depthwise layer (operand_bn_act :544-549: a depthwise layer in front of a project layer whose
          channels are a multiple of 4, :676, :708)
      dz  the project layers (dzp for the residual ones, engine_plan.hip:266, else in place: engine_backward.hip:210, :223, :226); the late
          expand layers (in place behind launch_depthwise_dgrad_bn's rows, :215-223); the depthwise layers of the recompute blocks and of
          the first block (fold_apply needs dw_fused_train, false for them: :213, so :223 or :226 writes dz in place); aspp0 and
          concat_projection (:149, :182).  NOT the stem and the recompute expand layers (:228-302: never formed in memory), NOT
          image_pooling (no handle)
      da  the residual project layers (their dz goes to dzp, so what launch_xdw_bwd_dx, :254-257, or the expand layer's input-gradient
          GEMM, :347-351, wrote survives)
      dy  SPECIAL CASE, a late depthwise layer whose project layer has M = B * pixels >= 256 rows: the project layer's input-gradient GEMM
          multiplies da by act' on the way out and leaves the BN-backward sums (red_mode 2, engine_backward.hip:355-360); only the
          split-product kernels fuse that reduction, and live_pointwise takes them from 256 rows on (split_pays, engine_forward.hip:10-13:
          K >= 32, K % 8 == 0, M >= 256; K = the project layer's output channels, 64 .. 320).  With those rows fold_apply holds (:213-214:
          channels a multiple of 64, dw_fused_train) and the apply pass runs inside launch_depthwise_dgrad_bn2 (:311-323): the handle
          keeps dy = da * act' and dz is never formed in memory.  Below 256 rows the GEMM runs unfused, :226 (plain bn_backward) writes
          dz in place, and the layer is listed under dz.  Link B2 checks exactly the one listed here and fails on the other."""
    backbone = [l for l in spec.layers if l.scope.startswith("MobilenetV2")]
    head = [l.idx for l in spec.layers[-4:-1]]                                   # image_pooling, aspp0, concat_projection
    rec = recompute_expand(spec)
    project = {l.idx for l in backbone if l.scope.endswith("/project")}
    late_expand = {l.idx for l in backbone if l.scope.endswith("/expand")} - rec
    early_dw = {i + 1 for i in rec} | {2}
    late_dw = {l.idx for l in backbone if l.scope.endswith("/depthwise")} - early_dw
    out = {("z", l.idx) for l in spec.layers if l.bn_eps is not None and l.idx not in rec}
    out |= {("a", i) for i in project | set(head)}
    sizes = S.feature_sizes(H, 2 * H, spec.layers)
    rows = {l.idx: B * h * w for l, (h, w) in zip(spec.layers, sizes)}
    by_idx = {l.idx: l for l in spec.layers}
    folded = {i for i in late_dw if rows[i + 1] >= 256 and by_idx[i + 1].cout >= 32 and by_idx[i + 1].cout % 8 == 0 and by_idx[i].cin % 64 == 0}
    out |= {("dz", i) for i in project | late_expand | early_dw | (late_dw - folded) | set(head[1:])}
    out |= {("da", l.idx) for l in backbone if l.residual_from is not None}
    out |= {("dy", i) for i in folded}
    return frozenset(out)


def default_step_plan(links):
    """The links whose inputs and outputs the DEFAULT (fused) step provably writes with their plain meaning.

    Recompute blocks = expanded_conv_1 .. _6 (block input <= 32 channels, xdw_train_supported); "late" blocks = expanded_conv_7 .. _16.

    Covered
      F1  the stem (frames -> z, launch_stem); the expand layers of the late blocks (x = the previous project layer's a, always
          written: engine_forward.hip:708-710 act_pass is true for a project layer); image_pooling, aspp0, concat_projection, logits
      F2  every project layer (its a and its residual source, another project layer's a, are written); image_pooling, aspp0,
          concat_projection
      F3  every layer whose z is written: all but the expand layers of the recompute blocks
      L   loss sums from AMS_REGION_LOGITS
      B1  logits (weights and bias), concat_projection, aspp0, image_pooling; the expand layers of the late blocks (x = a stored project a,
          dz written in place by launch_bn_bwd_apply, engine_backward.hip:216)
      B2  concat_projection, aspp0, image_pooling; the last backbone layer (engine_backward.hip:219: first iteration, plain bn_backward);
          every project layer that feeds a late block (its consumers' dz are the late expand layer's, and the stored da of the residual
          project layer; its own dz goes to dzp or in place through launch_bn_bwd_apply, :216)
      DA  the residual project layers of the late blocks but the last (da written by the expand layer's input-gradient GEMM with the skip
          gradient added, engine_backward.hip:340-352; dz goes to dzp, so da survives)
    Covered by the composite plan (layer_links.composite_plan, test_every_link_of_the_default_step: the links close across the tensors
    that are not stored, from the nearest stored one)
      F1 / F2 / F3 / B1 / B2 of the recompute blocks' expand layers: z_e, a_e, da_e, dz_e are never stored (engine_forward.hip:642-679,
          engine_backward.hip:221-275)
      F1 of every depthwise layer, F2 of every expand layer and of the stem: the expand layer's / the stem's a is applied on the depthwise
          kernel's tap loads and not written (engine_forward.hip:637, :682-691, :709)
      F1 and B1 of every project layer, F2 of every depthwise layer: the depthwise a is applied on the project GEMM's operand loads and not
          written (operand_bn_act, engine_forward.hip:697-701, engine_backward.hip:331)
      B1 / B2 of every depthwise layer: with the apply pass folded into the depthwise backward kernel its dz is never formed, the da buffer
          keeps dy = da * mask (engine_backward.hip:206-216, :305-308); the recompute blocks' depthwise dz is formed but its consumer's
          tensors are not
      B2 of the late expand layers: their consumer's dz (depthwise) is not stored; their da buffer holds dy before dz overwrites it
          (launch_depthwise_dgrad_bn, engine_backward.hip:311)
      B2 of the project layers that feed a recompute block or the first block, and B1 / B2 of the stem: the consumer's dz is not stored
          (engine_backward.hip:237-250, :277-294)
    """
    sp = links.spec
    recompute_expand = {l.idx for l in links.backbone if l.scope.endswith("/expand") and 8 <= l.cin <= 32 and l.cin % 4 == 0}
    late_expand = {l.idx for l in links.backbone if l.scope.endswith("/expand")} - recompute_expand
    project = {l.idx for l in links.backbone if l.scope.endswith("/project")}
    head = [links.lp.idx, links.la.idx, links.lc.idx]
    plan = [("L", 0), ("F1", 1)]
    plan += [("F1", i) for i in sorted(late_expand) + head + [links.ll.idx]]
    plan += [("F2", i) for i in sorted(project) + head]
    plan += [("F3", l.idx) for l in sp.layers if l.bn_eps is not None and l.idx not in recompute_expand]
    plan += [("B1", i) for i in sorted(late_expand) + head + [links.ll.idx]]
    feeds_late = sorted(i for i in project if i + 1 in late_expand)
    plan += [("B2", i) for i in feeds_late + [links.nb] + head]
    plan += [("DA", i) for i in feeds_late if links.by_idx[i].residual_from is not None]
    return plan


def composite_plan(spec) -> List[Tuple[str, int]]:
    """The complement of default_step_plan: every link of the default step that closes only across a
    tensor the step does not store (default_step_stored).
      F1  every depthwise layer (x = act(BN(z)) of the stored stem / late expand z; for the recompute blocks z_e itself is the conv of the
          stored block input) and every project layer (x = act(BN(z_d)))
      F3  the recompute blocks' expand layers, from the derived z_e
      B1  the stem and the recompute expand layers (derived dz, derived mask), every depthwise layer (derived x; derived dz for the late
          ones), every project layer (derived x)
      B2  the stem, every expand layer, every depthwise layer, and the project layers in front of a recompute block or of the first block
          (the consumer's dz is derived)
      DA  the residual project layers in front of a recompute block"""
    backbone = [l for l in spec.layers if l.scope.startswith("MobilenetV2")]
    rec = recompute_expand(spec)
    dw = [l.idx for l in backbone if l.scope.endswith("/depthwise")]
    project = [l.idx for l in backbone if l.scope.endswith("/project")]
    expand = [l.idx for l in backbone if l.scope.endswith("/expand")]
    feeds_rec = [i for i in project if i + 1 in rec]
    plan = [("F1", i) for i in dw + project]
    plan += [("F3", i) for i in sorted(rec)]
    plan += [("B1", i) for i in [1] + sorted(rec) + dw + project]
    plan += [("B2", i) for i in [1] + expand + dw + feeds_rec]
    plan += [("DA", i) for i in feeds_rec if spec.layers[i - 1].residual_from is not None]
    return plan


def plan_names(spec, plan) -> set:
    """the gradient tensors and moving statistics the links of ``plan`` compare"""
    by_idx = {l.idx: l for l in spec.layers}
    out = set()
    for link, idx in plan:
        if link == "B1":
            out.add(by_idx[idx].weight_name)
            if by_idx[idx].bn_eps is None:
                out.add(by_idx[idx].scope + "/biases:0")
        elif link == "B2":
            out |= {by_idx[idx].scope + "/BatchNorm/gamma:0", by_idx[idx].scope + "/BatchNorm/beta:0"}
        elif link == "F3":
            out |= {by_idx[idx].scope + "/BatchNorm/moving_mean:0", by_idx[idx].scope + "/BatchNorm/moving_variance:0"}
    return out


def withhold(run: dict, stored) -> dict:
    """``run`` as a step that stores only ``stored`` would leave it: every other z / a / da / dz is dropped, and the dz handle of a
    ("dy", idx) layer holds dy = da * act' (oracle_run keeps it under "dy")."""
    out = copy_run(run)
    for kind in ("z", "a", "da", "dz"):
        out[kind] = {i: t for i, t in run[kind].items() if (kind, i) in stored}
    for kind, i in stored:
        if kind == "dy":
            out["dz"][i] = run["dy"][i]
    out.pop("dy", None)
    out["dlogits"] = None                                                        # no handle either
    return out


def ambiguity_report(links: "Links") -> str:
    rows = ["%-46s band %.2e  ambiguous %2d (%.1e of the layer, at most %d per channel)  resolved away from f64: %d  nearest %.2e"
            % (links.by_idx[i].scope, d["tau"], d["ambiguous"], d["share"], d["per_channel"], d["resolved"], d["nearest"])
            for i, d in sorted(links.ambiguous.items())]
    return "\n".join(rows)


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
    dwl = [l for l in backbone if l.kind == "dw"]
    g = torch.autograd.grad(loss, list(leaves.values()) + [ztaps[l.scope] for l in zl] + [a_graph[l.idx] for l in rl] + [low] +
                            [a_graph[l.idx] for l in dwl])
    g, g_dw = g[:len(g) - len(dwl)], g[len(g) - len(dwl):]
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
    # y: the BN output in front of the activation, by the oracle's own function on the oracle's own z (the same operations: the same bits);
    # dy: what the dz handle of a late depthwise layer holds in the default step (default_step_stored), autograd through the activation
    run["y"], run["dy"] = {}, {}
    for l in backbone:
        if l.act == "none":
            continue
        y = batch_norm_train(ztaps[l.scope].detach(), o.vars[l.scope + "/BatchNorm/gamma:0"], o.vars[l.scope + "/BatchNorm/beta:0"], l.bn_eps)[0]
        run["y"][l.idx] = _to64(y)
        if l in dwl:
            y = _leaf(y)
            run["dy"][l.idx] = _to64(torch.autograd.grad((StudentOracle._act(y, l.act) * g_dw[dwl.index(l)]).sum(), y)[0])
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


def join_rank_runs(runs: List[dict], identical: bool = True) -> dict:
    """The runs of the ranks of ONE data-parallel step, each on its own shard of the batch, as the run of the whole batch: frames, labels,
    teacher logits, logits and every z / a / dz / da (dlogits, y, dy where the runs keep them) concatenated along the batch in rank order;
    params and stats_before from rank 0.  grads, stats_after and loss are what the step leaves AFTER its cross-rank sums, so every rank
    must hold the same bits (identical Adam input on every rank is the data-parallel invariant): asserted, with the name of the first
    tensor that differs, and taken once.  ``identical`` False takes rank 0's without looking (un-synchronised stand-ins on the CPU)."""
    r0 = runs[0]
    if identical:
        for k, r in enumerate(runs[1:], 1):
            for key in ("grads", "stats_after"):
                assert list(r[key]) == list(r0[key]), "rank %d names other %s than rank 0" % (k, key)
                for name, t in r0[key].items():
                    assert torch.equal(r[key][name], t), "%s of %s on rank %d is not rank 0's, bit for bit (worst |difference| %.3e)" % (
                        key, name, k, float((r[key][name] - t).abs().max()))
            assert tuple(r["loss"]) == tuple(r0["loss"]), "loss (CE sum, valid count) on rank %d %r is not rank 0's %r" % (k, r["loss"], r0["loss"])
    out = copy_run(r0)
    for key in ("frames", "logits", "dlogits"):
        if r0.get(key) is not None:
            out[key] = torch.cat([r[key] for r in runs], dim=0)
    for key in ("labels", "teacher_logits"):
        if r0.get(key) is not None:
            out[key] = np.concatenate([np.asarray(r[key]) for r in runs], axis=0)
    for kind in ("z", "a", "dz", "da", "y", "dy"):
        if kind in r0:
            out[kind] = {i: torch.cat([r[kind][i] for r in runs], dim=0) for i in r0[kind]}
    return out


# ---------------------------------------------------------------------------------------------------------
# the cases both test modules share, and the f32 reference levels the bars come from
# ---------------------------------------------------------------------------------------------------------
CI = [0, 1, 2, 10, 11, 13]
SIZES = ((64, 2), (62, 3), (34, 5))          # height (width = 2 x height), frames: even block inputs, even and odd ones (SAME pads differ), odd tiny maps
SOFT_GRID = (9, 17)
FUSED_SIZE = (128, 2)          # the smallest case whose stride-16 GEMMs have 256 rows: the split-product kernels, their fused sums, fold_apply
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


def f32_run(H: int, B: int, soft: bool = False) -> dict:
    """The f32 CPU oracle's own step of case (H, B); computed once per process."""
    key = ("f32 run", H, B, soft)
    if key not in _memo:
        frames, labels = case_clip(H, B)
        _memo[key] = oracle_run(case_weights(), CI, frames, labels, torch.float32, teacher_logits=case_teacher_logits(B) if soft else None)
    return _memo[key]


def f32_run_results(H: int, B: int, soft: bool = False) -> List[Result]:
    """Every link (soft: link L only) closed on the f32 CPU oracle's own step of case (H, B); computed once per process."""
    key = ("f32", H, B, soft)
    if key not in _memo:
        _memo[key] = Links(f32_run(H, B, soft)).close([("L", 0)] if soft else None)
    return _memo[key]


def f32_levels(sizes=SIZES, soft: bool = False) -> Dict[str, float]:
    """Worst error per link kind of the f32 CPU oracle's own step over ``sizes``: the f32 reference levels"""
    worst: Dict[str, float] = {}
    for H, B in sizes:
        for kind, r in worst_by_kind(f32_run_results(H, B, soft)).items():
            worst[kind] = max(worst.get(kind, 0.0), r.err)
    return worst


BAND_MARGIN = 8.0          # x the f32 CPU oracle's own |y_f32 - y_f64|: the engine sums in another order and multiplies 22-bit split parts


def f32_bands(sizes=SIZES, margin: float = BAND_MARGIN) -> Dict[int, float]:
    """{idx: tau} of every layer whose a the default step withholds: ``margin`` x the largest |y_f32 - y_f64| over ``sizes``, y_f32 the f32
    CPU oracle's own BN output of that layer and y_f64 = BN_batch in f64 of the z that Links derives from the same run with the default
    step's tensors withheld.  Measured on the reference, never on the engine."""
    key = ("bands", tuple(sizes), margin)
    if key not in _memo:
        spec = S.build_spec()
        out: Dict[int, float] = {}
        for H, B in sizes:
            stored = default_step_stored(spec, H, B)
            run = f32_run(H, B)
            links = Links(withhold(run, stored), stored=stored)
            for l in links.backbone:
                if l.act != "none" and ("a", l.idx) not in stored:
                    y64 = links._bn(l, links.z(l.idx), *links._gb(l))[0]
                    out[l.idx] = max(out.get(l.idx, 0.0), margin * float((run["y"][l.idx] - y64).abs().max()))
        _memo[key] = out
    return _memo[key]


def late_plan(plan) -> List[Tuple[str, int]]:
    """the links of ``plan`` on the stride-16 blocks, expanded_conv_7 .. _16 (the layers behind the last recompute block)"""
    first = max(recompute_expand(S.build_spec())) + 3
    return [(k, i) for k, i in plan if i >= first]


def f32_composite_results(H: int, B: int, late: bool = False) -> Tuple[List[Result], "Links"]:
    """composite_plan (late: its links on the stride-16 blocks) closed on the f32 CPU oracle's own step of case (H, B) with the default
    step's tensors withheld; the bands are those of the case's own size where ``late``"""
    key = ("f32 composite", H, B, late)
    if key not in _memo:
        spec = S.build_spec()
        stored = default_step_stored(spec, H, B)
        links = Links(withhold(f32_run(H, B), stored), stored=stored, bands=f32_bands(((H, B),)) if late else f32_bands())
        plan = composite_plan(spec)
        _memo[key] = (links.close(late_plan(plan) if late else plan), links)
    return _memo[key]


def f32_composite_levels(sizes=SIZES, late: bool = False) -> Dict[str, float]:
    """Worst error per link kind of the composite links on the f32 CPU oracle's own step over ``sizes``"""
    worst: Dict[str, float] = {}
    for H, B in sizes:
        for kind, r in worst_by_kind(f32_composite_results(H, B, late)[0]).items():
            worst[kind] = max(worst.get(kind, 0.0), r.err)
    return worst


def composite_bars(levels: Dict[str, float]) -> Dict[str, Tuple[float, str]]:
    """kind -> (bar, source) of the composite links: 4 x the f32 CPU oracle's own error on the same links with the same tensors withheld
    (the link ends in more than one kernel family, so no kernel test's bar is its measure); none above BAR_CAP."""
    out = {k: (4.0 * v, "4 x f32 CPU composite level %.2e" % v) for k, v in levels.items()}
    assert all(b <= BAR_CAP for b, _ in out.values()), out
    return out


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
