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

THE DEFAULT STEP is held by two plans that together name all 164 gradient tensors and all 108 moving statistics: default_step_plan (the
links whose inputs and outputs the step stores) at the bars above, and layer_links.composite_plan (the links that close across a tensor
the step does not store: everything inside the recompute blocks, the first block, the depthwise and project layers' operand transforms,
the late expand layers' BN backward) at 4 x the f32 CPU oracle's own error on the same composite links with the same tensors withheld.
Which tensors the step stores depends on the size (layer_links.default_step_stored): from 256 rows in the stride-16 GEMMs on, the late
depthwise layers' dz handle holds dy and their backward runs through the fused kernels; 128x256 x 2 is the case that holds that path.
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


default_step_plan = LL.default_step_plan          # the plan lives beside composite_plan


@pytest.mark.parametrize("H,B", [(64, 2), (62, 3)])
def test_links_of_the_default_step(bars, H, B):
    """What production runs: the default fused step, on the links listed in default_step_plan, at the same bars."""
    links = LL.Links(_engine_run(H, B, layerwise=False))
    plan = default_step_plan(links)
    assert len(plan) == len(set(plan)) == 1 + 15 + 20 + 48 + 14 + 14 + 7
    res = links.close(plan)
    _hold("default step %dx%d x %d" % (H, 2 * H, B), res, bars)


@pytest.fixture(scope="module")
def composite():
    """bars and bands of the composite links: from the f32 CPU oracle's own step with the default step's tensors withheld, over the sizes"""
    levels = LL.f32_composite_levels()
    bands = LL.f32_bands()
    print("f32 CPU composite levels: %s\nbands (tau per layer): %s" % (levels, bands))
    return LL.composite_bars(levels), bands


def _hold_composite(tag, H, B, run, composite_bars, bands, late=False):
    sp = LL.S.build_spec()
    stored = LL.default_step_stored(sp, H, B)
    links = LL.Links(run, stored=stored, bands=bands)
    plan = LL.composite_plan(sp)
    # the two plans together name every gradient tensor and every moving statistic of the step
    both = LL.plan_names(sp, plan) | LL.plan_names(sp, default_step_plan(links))
    assert both == {v.name for v in sp.trainable} | {v.name for v in sp.stats} and len(sp.trainable) == 164
    assert not set(plan) & set(default_step_plan(links))
    try:
        res = links.close(LL.late_plan(plan) if late else plan)
    finally:
        print("%s: masks of the activations that are not stored\n%s" % (tag, LL.ambiguity_report(links)))
    _hold(tag, res, composite_bars)
    return res


@pytest.mark.parametrize("H,B", LL.SIZES)
def test_every_link_of_the_default_step(composite, H, B):
    """What production runs, on the links default_step_plan leaves out: each closes in f64 across the tensors the default step does not
    store (layer_links.default_step_stored), the masks of the withheld activations resolved element by element (Links.resolved_mask),
    at 4 x the f32 CPU oracle's own error on the same composite links.  At these sizes the stride-16 GEMMs have 64 .. 96 rows, so the
    late depthwise layers' dz is written in place by the unfused BN backward and is checked as dz; the fused path of those blocks is
    test_late_blocks_of_the_default_step_with_fused_gemms."""
    res = _hold_composite("default step, composite links, %dx%d x %d" % (H, 2 * H, B), H, B, _engine_run(H, B, layerwise=False), *composite)
    assert not [r for r in res if r.name.endswith(" (dy)")]


def test_every_link_of_the_default_step_soft_teacher(composite):
    """The same with the soft-teacher feed on the 9 x 17 grid: the plan does not depend on the form of the loss."""
    _hold_composite("default step, composite links, soft teacher 64x128 x 2", 64, 2, _engine_run(64, 2, soft=True, layerwise=False), *composite)


def test_late_blocks_of_the_default_step_with_fused_gemms():
    """128x256 x 2: the smallest case whose stride-16 GEMMs have 256 rows, from which live_pointwise takes the split-product kernels
    (split_pays).  Only there does the project layers' input-gradient GEMM apply act' and leave the BN-backward sums (red_mode 2), and only
    then does fold_apply send the depthwise layer's apply pass through launch_depthwise_dgrad_bn2 with cA / cB / cC, the expand layer's
    scale / shift / mean / rstd and the layer's own partial rows: what production runs for expanded_conv_7 .. _16.  default_step_stored
    lists every late depthwise handle as dy for this size, and B2 checks it as dy only: a step that fell back to the unfused path fails.
    The composite links of the stride-16 blocks (one engine step; the f64 side works on 8 x 16 maps), bars and bands from the f32 CPU
    oracle's own step at this size."""
    H, B = LL.FUSED_SIZE
    sizes = (LL.FUSED_SIZE,)
    levels, bands = LL.f32_composite_levels(sizes, late=True), LL.f32_bands(sizes)
    print("f32 CPU composite levels, stride-16 blocks: %s" % levels)
    res = _hold_composite("default step, stride-16 blocks, %dx%d x %d" % (H, 2 * H, B), H, B, _engine_run(H, B, layerwise=False),
                          LL.composite_bars(levels), bands, late=True)
    assert len([r for r in res if r.name.endswith(" (dy)")]) == 10                # every late depthwise handle was checked as dy
