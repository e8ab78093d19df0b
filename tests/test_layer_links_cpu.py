"""The link-by-link check of the fine-tune step (tests/layer_links.py) proved on the CPU, before any kernel is involved.

(a) Every link — head, loss and moving statistics included — closes to 1e-10 on the f64 oracle's own free-running step: the helper's
    topology (residual sources, concat order, pooled broadcast, statistics update, which dz feeds which cotangent) is the oracle's.
(b) The same on the f32 oracle's step gives the f32 reference level of every link kind; 4 x that level is the bar of every kind that has no
    kernel-level f64 bar of its own (tests/test_gpu_layer_links.py).
(c) Negative controls: five wrong wires, each made on a copy of the f64 run's tensors, fail the link they belong to at those bars.

Sizes: 64x128 x 2 frames and 62x124 x 3 frames (even and odd block inputs pad differently under SAME).
"""
import pytest
import torch

import layer_links as LL

SIZES = LL.SIZES[:2]


@pytest.fixture(scope="module")
def runs64():
    out = {}
    for H, B in SIZES:
        frames, labels = LL.case_clip(H, B)
        out[(H, B)] = LL.oracle_run(LL.case_weights(), LL.CI, frames, labels, torch.float64)
    return out


@pytest.fixture(scope="module")
def bars():
    return LL.bars_from_levels(LL.f32_levels())           # the bars of the GPU test: levels over all of its sizes


@pytest.mark.parametrize("H,B", SIZES)
def test_every_link_closes_on_the_f64_oracle_step(runs64, H, B):
    res = LL.Links(runs64[(H, B)]).close()
    print(LL.report(res))
    assert {r.kind for r in res} == set(LL.KINDS)
    # L (sum, count, dlogits), F1, B1 (+ the logits bias), F2, F3 (mean, variance), B2 (dz, dgamma, dbeta; no stored dz of image_pooling), DA
    assert len(res) == 3 + 55 + 56 + 54 + 2 * 54 + (3 * 54 - 1) + 10
    bad = [r for r in res if not r.err <= 1e-10]
    assert not bad, bad


def test_soft_teacher_loss_link_closes_on_the_f64_oracle_step():
    H, B = SIZES[0]
    frames, labels = LL.case_clip(H, B)
    run = LL.oracle_run(LL.case_weights(), LL.CI, frames, labels, torch.float64, teacher_logits=LL.case_teacher_logits(B))
    res = LL.Links(run).close()
    assert not [r for r in res if not r.err <= 1e-10]
    hard = LL.oracle_run(LL.case_weights(), LL.CI, frames, labels, torch.float64)
    assert abs(run["loss"][0] - hard["loss"][0]) > 1e-3 * hard["loss"][0]          # the soft targets were really used


def test_f32_oracle_step_gives_the_reference_levels(bars):
    """The f32 CPU oracle's own step, link by link against f64: rounding of one link, nothing amplified — every kind far below 1e-5
    (LL.BAR_CAP / 4 would already void the bars, bars_from_levels asserts it)."""
    for H, B in SIZES:
        print("f32 CPU oracle, %dx%d x %d:" % (H, 2 * H, B))
        print(LL.report(LL.f32_run_results(H, B)))
    levels = LL.f32_levels(SIZES)
    assert set(levels) == set(LL.KINDS) and all(0 < v for k, v in levels.items())
    assert set(bars) == set(LL.KINDS)


def _fails(run, bars, expect, around):
    """the backward links (B1, B2, DA) of the layers within three of ``around`` that fail on ``run``; ``expect`` must be among them"""
    links = LL.Links(run)
    near = [l for l in links.spec.layers if abs(l.idx - around.idx) <= 3]
    plan = [(k, l.idx) for l in near for k in ("B1", "B2", "DA") if (k == "B1" or l.bn_eps is not None) and (k != "DA" or l.residual_from is not None)]
    res = links.close(plan)
    bad = {(r.link, r.name) for r in LL.failures(res, bars)}
    assert expect <= bad, (expect, bad)
    return bad


@pytest.mark.parametrize("H,B", SIZES)
def test_negative_controls(runs64, bars, H, B):
    run = runs64[(H, B)]
    links = LL.Links(run)
    assert not LL.failures(links.close(), bars)
    L = {l.scope: l for l in links.spec.layers}

    # 1. one weight-gradient slice scaled by 1 + 1e-4
    name = "MobilenetV2/expanded_conv_3/depthwise/depthwise_weights:0"
    bad = LL.copy_run(run)
    bad["grads"][name] = run["grads"][name] * (1 + 1e-4)
    assert _fails(bad, bars, {("B1", name)}, L[name.rsplit("/", 1)[0]]) == {("B1", name)}

    # 2. a skip gradient taken from the neighbouring block (blocks 4 and 5: same shape)
    a, b = L["MobilenetV2/expanded_conv_4/project"], L["MobilenetV2/expanded_conv_5/project"]
    bad = LL.copy_run(run)
    bad["da"][a.idx] = run["da"][b.idx]
    src = links.by_idx[a.residual_from]
    assert _fails(bad, bars, {("B2", src.scope), ("DA", a.scope)}, a) <= {("B2", src.scope), ("B2", src.scope + "/BatchNorm/gamma:0"),
                                                                        ("B2", src.scope + "/BatchNorm/beta:0"), ("DA", a.scope)}

    # 3. a stride-2 depthwise dz shifted by one pixel
    d = L["MobilenetV2/expanded_conv_3/depthwise"]
    assert d.stride == 2
    bad = LL.copy_run(run)
    bad["dz"][d.idx] = torch.roll(run["dz"][d.idx], 1, dims=3)
    _fails(bad, bars, {("B1", d.weight_name), ("B2", d.scope)}, d)

    # 4. the pooled gradient scaled by 1 / HW once more: what the last backbone layer's dz would then be
    last = links.by_idx[links.nb]
    g_aspp, g_pool = links.cot_parts(last.idx)
    hw = g_pool.shape[2] * g_pool.shape[3]
    bad = LL.copy_run(run)
    bad["dz"][last.idx] = links._bn_backward(last, g_aspp + g_pool / hw)[0]
    _fails(bad, bars, {("B2", last.scope)}, last)

    # 5. dgamma and dbeta of one layer swapped
    e = L["MobilenetV2/expanded_conv_7/expand"]
    gname, bname = e.scope + "/BatchNorm/gamma:0", e.scope + "/BatchNorm/beta:0"
    bad = LL.copy_run(run)
    bad["grads"][gname], bad["grads"][bname] = run["grads"][bname], run["grads"][gname]
    assert _fails(bad, bars, {("B2", gname), ("B2", bname)}, e) == {("B2", gname), ("B2", bname)}
