"""The engine's fine-tune step held to f64 link by link, teacher-forced (tests/layer_links.py; proved on the CPU in
tests/test_layer_links_cpu.py).

One train_step of a trainable StudentEngine with synthetic weights; every intermediate tensor is the engine's own, and each layer's link
(conv forward, BN + activation + residual, moving statistics, loss, weight gradient, BN backward with the cotangent formed from the
stored dz of every consumer) is recomputed in f64 from the engine's own inputs to that link.  What this holds that the free-running
bars (tests/test_gpu_network.py, tests/test_gpu_train_recompute.py: percent level) cannot: which tensor feeds which kernel, skip
gradients and dzp, the pooled-gradient broadcast, the BN coefficient plumbing, the moving-statistics update and the offsets into the
gradient arena — a wire from the wrong layer or a coefficient a few percent off is orders of magnitude above these bars.

BARS (layer_links.bars_from_levels).  A link kind whose kernel family has an f64 bar under the same elementwise measure in
tests/test_gpu_kernels.py uses that bar: conv_stem 1e-5 (test_stem_conv), conv_dw 1e-5 (test_depthwise_forward_and_backward), conv_1x1
2e-5 (test_pointwise_forward), da 2e-5 (test_pointwise_image_bias_and_transposed_weights: the input-gradient GEMM), dlogits 2e-5
(test_upsample_argmax_metrics_and_ce_grad).  Every other kind (bn_act, dz, wgrad, dgamma, dbeta, stats, loss) has no such bar (the
kernel tests measure reduced quantities against max|ref|, not against the sum of the absolute terms): its bar is 4 x the worst error of
the f32 CPU oracle's own step on that kind over the same sizes, computed here from the reference, never from the engine.  No bar
exceeds 1e-4.
"""
import pytest
import torch

import layer_links as LL
from ams_amd import hip
from ams_amd.engine import StudentEngine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bars():
    return LL.bars_from_levels(LL.f32_levels())


def _engine_run(H, B, matmul=None, soft=False, layerwise=True):
    W = LL.case_weights()
    frames, labels = LL.case_clip(H, B)
    tl = LL.case_teacher_logits(B) if soft else None
    eng = StudentEngine(LL.CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W)
    if layerwise:
        # every fine-tune fusion off: the state in which include/ams_hip.h promises that z, a, da and dz of every layer are written
        eng.set_train_recompute(False, fuse_dgrad_bn=0, fuse_gemm_red=0)
        eng.set_fuse_operand_bn(0)
    if matmul is not None:
        eng.set_matmul_mode(matmul)
    if soft:
        eng.set_soft_teacher(True)
    loss = eng.train_step(frames, labels, 1e-3, teacher_logits=tl)
    torch.cuda.synchronize()
    run = LL.engine_run(eng, W, LL.CI, frames, labels, loss, tl)       # W: the parameters before Adam changed them
    eng.close()
    return run


def _hold(tag, res, bars):
    print("%s: engine errors per link kind\n%s" % (tag, LL.report(res, bars)))
    bad = LL.failures(res, bars)
    assert not bad, "%s: %d links over their bar, worst first: %s" % (tag, len(bad), sorted(bad, key=lambda r: -r.err)[:8])


@pytest.mark.parametrize("H,B,matmul", [(64, 2, None), (62, 3, None), (34, 5, None), (64, 2, hip.MATMUL_F32)])
def test_every_link_of_the_layerwise_step(bars, H, B, matmul):
    """Every link of the step on the engine's tensors, all fine-tune fusions off; default product mode at three sizes, exact f32 at one."""
    res = LL.Links(_engine_run(H, B, matmul)).close()
    assert {r.kind for r in res} == set(LL.KINDS) - {"dlogits"}            # dlogits has no ABI handle: held through the links that read it
    _hold("%dx%d x %d, matmul %s" % (H, 2 * H, B, matmul), res, bars)


def test_soft_teacher_loss_link(bars):
    """Link L with soft teacher logits on a 9 x 17 grid; the rest of the step as in the hard case (the loss's gradient reaches the logits
    layer's weights and bias and concat_projection's dz, held by B1 / B2 of those layers)."""
    H, B = 64, 2
    soft_bars = dict(bars)
    soft_bars["loss"] = LL.bars_from_levels(LL.f32_levels(((H, B),), soft=True))["loss"]
    res = LL.Links(_engine_run(H, B, soft=True)).close()
    _hold("soft teacher %dx%d x %d" % (H, 2 * H, B), res, soft_bars)


def test_image_pooling_statistics_of_two_similar_frames(bars):
    """Regression.  The image-pooling BN normalises over the batch alone; two frames of one clip pool to nearly the same vector, so the batch
    variance is far below the squared distance of the batch mean from the moving mean the sums are centred on.  With (z - centre)^2
    formed in f32 that variance was lost: a of image_pooling 1.2e-4 off, its weight gradient 4e-5, dgamma 7e-5 and the last backbone
    layer's dz (which receives the pooled gradient) 3e-5, at 64x128 x 2 frames.  The sums of this layer are formed in f64 now."""
    links = LL.Links(_engine_run(64, 2))
    res = links.close([("F2", links.lp.idx), ("F3", links.lp.idx), ("B1", links.lp.idx), ("B2", links.lp.idx), ("B2", links.nb)])
    _hold("image pooling, 64x128 x 2", res, bars)


def default_step_plan(links):
    """The links whose inputs and outputs the DEFAULT (fused) step provably writes with their plain meaning.

    Recompute blocks = expanded_conv_1 .. _6 (block input <= 32 channels, xdw_train_supported); "late" blocks = expanded_conv_7 .. _16.

    Covered
      F1  the stem (frames -> z, launch_stem); the expand layers of the late blocks (x = the previous project layer's a, always
          written: engine_forward.hip:696-698 act_pass is true for a project layer); image_pooling, aspp0, concat_projection, logits
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
    Not covered
      F1 / F2 / F3 / B1 / B2 of the recompute blocks' expand layers: z_e, a_e, da_e, dz_e are never stored (engine_forward.hip:632-667,
          engine_backward.hip:221-275)
      F1 of every depthwise layer, F2 of every expand layer and of the stem: the expand layer's / the stem's a is applied on the depthwise
          kernel's tap loads and not written (engine_forward.hip:627, :670-679, :697)
      F1 and B1 of every project layer, F2 of every depthwise layer: the depthwise a is applied on the project GEMM's operand loads and not
          written (operand_bn_act, engine_forward.hip:685-689, engine_backward.hip:331)
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


@pytest.mark.parametrize("H,B", [(64, 2), (62, 3)])
def test_links_of_the_default_step(bars, H, B):
    """What production runs: the default fused step, on the links listed in default_step_plan, at the same bars."""
    links = LL.Links(_engine_run(H, B, layerwise=False))
    plan = default_step_plan(links)
    assert len(plan) == len(set(plan)) == 1 + 15 + 20 + 48 + 14 + 14 + 7
    res = links.close(plan)
    _hold("default step %dx%d x %d" % (H, 2 * H, B), res, bars)
