"""The link-by-link check of the fine-tune step (tests/layer_links.py) proved on the CPU, before any kernel is involved.

(a) Every link — head, loss and moving statistics included — closes to 1e-10 on the f64 oracle's own free-running step: the helper's
    topology (residual sources, concat order, pooled broadcast, statistics update, which dz feeds which cotangent) is the oracle's.
(b) The same on the f32 oracle's step gives the f32 reference level of every link kind; 4 x that level is the bar of every kind that has no
    kernel-level f64 bar of its own (tests/test_gpu_layer_links.py).
(c) Negative controls: five wrong wires, each made on a copy of the f64 run's tensors, fail the link they belong to at those bars.
(d) The default step: the same runs with every tensor the default (fused) step does not store withheld (LL.default_step_stored).  Both
    plans together close to 1e-10 across the withheld tensors; the f32 run gives the levels of the composite links and the band of every
    withheld activation; six more wrong wires and two planted mask bits fail or pass as they must.
(e) The data-parallel step (LL.join_rank_runs, tests/test_gpu_dp_links.py): the f32 oracle's step of 4 frames cut into the runs of two ranks
    (3 + 1 frames) and joined is the original and passes every link; un-synchronised BN (each rank's own oracle step), gradients that
    were not summed over the ranks, dgamma / dbeta summed twice each fail the links they belong to, and moving statistics that differ
    between the ranks stop the join.

Sizes: 64x128 x 2 frames and 62x124 x 3 frames (even and odd block inputs pad differently under SAME); 62x124 x 4 frames for (e).
"""
import numpy as np
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


# ---------------------------------------------------------------------------------------------------------
# the default step: the same runs with the tensors it does not store withheld (LL.default_step_stored)
# ---------------------------------------------------------------------------------------------------------
SPEC = LL.S.build_spec()
ALL_SIZES = SIZES + (LL.FUSED_SIZE,)
STORED = {(H, B): LL.default_step_stored(SPEC, H, B) for H, B in ALL_SIZES}


@pytest.fixture(scope="module")
def fused64():
    """the f64 oracle's step at the size from which the stride-16 GEMMs fuse their sums and the late depthwise handles hold dy"""
    H, B = LL.FUSED_SIZE
    frames, labels = LL.case_clip(H, B)
    return LL.oracle_run(LL.case_weights(), LL.CI, frames, labels, torch.float64)


@pytest.fixture(scope="module")
def composite():
    """(bars, bands) of the composite links as the GPU test takes them: f32 levels and bands over all of its sizes"""
    return LL.composite_bars(LL.f32_composite_levels()), LL.f32_bands()


_default_plan = LL.default_step_plan


def test_the_two_plans_name_every_gradient_and_statistic(runs64):
    links = LL.Links(runs64[SIZES[0]])
    a, b = LL.composite_plan(SPEC), _default_plan(links)
    assert not set(a) & set(b) and len(a) == len(set(a)) == 34 + 6 + 41 + 40 + 3
    assert LL.plan_names(SPEC, a) | LL.plan_names(SPEC, b) == {v.name for v in SPEC.trainable} | {v.name for v in SPEC.stats}
    assert len(SPEC.trainable) == 164 and len(SPEC.stats) == 108
    # the special case: a late depthwise handle holds dy from 256 rows in the stride-16 GEMMs on, dz below; never both, never neither
    late_dw = {l.idx for l in links.backbone if l.kind == "dw" and l.idx >= 23}
    for (H, B), stored in STORED.items():
        dy, dz = {i for k, i in stored if k == "dy"}, {i for k, i in stored if k == "dz"}
        assert (dy, dz & late_dw) == ((late_dw, set()) if (H // 16) * (H // 8) * B >= 256 else (set(), late_dw)), (H, B)
        assert not {i for k, i in stored if k == "z"} & LL.recompute_expand(SPEC)
    assert LL.recompute_expand(SPEC) == {4, 7, 10, 13, 16, 19}
    assert {(k, i) for k, i in LL.late_plan(a)} == {(k, i) for k, i in a if i >= 22}


@pytest.mark.parametrize("H,B", SIZES)
def test_the_default_plan_closes_on_the_f64_oracle_step_with_tensors_withheld(runs64, composite, H, B):
    stored = STORED[(H, B)]
    links = LL.Links(LL.withhold(runs64[(H, B)], stored), stored=stored, bands=composite[1])
    res = links.close(_default_plan(links) + LL.composite_plan(SPEC))
    print(LL.report(res))
    print(LL.ambiguity_report(links))
    assert {r.kind for r in res} == set(LL.KINDS) - {"dlogits"}
    bad = [r for r in res if not r.err <= 1e-10]
    assert not bad, bad
    assert not [r for r in res if r.name.endswith(" (dy)")]                         # under 256 rows: the late depthwise handles hold dz
    assert not any(d["resolved"] for d in links.ambiguous.values())                 # the f64 run's masks are the f64 masks
    assert len(links.ambiguous) == 34 and all(d["tau"] > 0 for d in links.ambiguous.values())


def test_f32_oracle_step_gives_the_composite_levels_and_bands(composite):
    """The f32 CPU oracle's own step with the default step's tensors withheld: the level of every kind of composite link (4 x that is its
    bar; composite_bars asserts the cap), the band of every withheld activation and how many elements fall into it."""
    bars, bands = composite
    for H, B in LL.SIZES:
        res, links = LL.f32_composite_results(H, B)
        print("f32 CPU oracle, composite links, %dx%d x %d:\n%s\n%s" % (H, 2 * H, B, LL.report(res, bars), LL.ambiguity_report(links)))
        assert not LL.failures(res, bars)
    print("bands: %s" % {SPEC.layers[i - 1].scope: "%.2e" % t for i, t in sorted(bands.items())})
    assert set(bars) == set(LL.KINDS) - {"conv_stem", "bn_act", "loss", "dlogits"}
    assert all(0 < b <= LL.BAR_CAP for b, _ in bars.values())
    assert len(bands) == 34 and all(0 < t < 1e-4 for t in bands.values())


def test_the_stride_16_blocks_close_where_the_handles_hold_dy(fused64):
    """At LL.FUSED_SIZE every late depthwise handle holds dy: the links of the stride-16 blocks of both plans close on the f64 step, each
    handle is checked as dy, and the two ways a step can betray the declaration fail that layer's B2 and nothing else: dy left unmasked
    (da where da * act' belongs), and dz written in place (the unfused path) where dy is declared."""
    stored = STORED[LL.FUSED_SIZE]
    bands = LL.f32_bands((LL.FUSED_SIZE,))
    bars = LL.composite_bars(LL.f32_composite_levels((LL.FUSED_SIZE,), late=True))
    good = LL.withhold(fused64, stored)
    links = LL.Links(good, stored=stored, bands=bands)
    plan = LL.late_plan(LL.composite_plan(SPEC))
    res = links.close(plan + LL.late_plan(_default_plan(links)))
    bad = [r for r in res if not r.err <= 1e-10]
    assert not bad, bad
    assert len([r for r in res if r.name.endswith(" (dy)")]) == 10
    d = [l for l in SPEC.layers if l.scope == "MobilenetV2/expanded_conv_8/depthwise"][0]
    full = LL.Links(fused64)
    for wrong in (full.cot_a(d.idx), fused64["dz"][d.idx]):
        run = LL.copy_run(good)
        run["dz"][d.idx] = wrong
        got = LL.failures(LL.Links(run, stored=stored, bands=bands).close(plan), bars)
        assert {(r.link, r.name) for r in got} == {("B2", d.scope + " (dy)")}, got


def _failing(run_w, composite, bars, around, bands=None, plan=None):
    """{(link, name)} of the links of both plans on the layers within three of ``around`` that fail on the withheld run"""
    links = LL.Links(run_w, stored=STORED[(run_w["frames"].shape[1], run_w["frames"].shape[0])], bands=composite[1] if bands is None else bands)
    near = lambda p: [(k, i) for k, i in p if abs(i - around.idx) <= 3]  # noqa: E731
    cplan = near(LL.composite_plan(SPEC)) if plan is None else plan
    bad = LL.failures(links.close(cplan), composite[0])
    if plan is None:
        bad += LL.failures(links.close(near(_default_plan(links))), bars)
    return {(r.link, r.name) for r in bad}, links


@pytest.mark.parametrize("H,B", SIZES)
def test_negative_controls_with_tensors_withheld(runs64, composite, bars, H, B):
    run = runs64[(H, B)]
    full = LL.Links(run)
    good = LL.withhold(run, STORED[(H, B)])
    L = {l.scope: l for l in SPEC.layers}

    # 1. the expand weight gradient of a recompute block scaled by 1 + 1e-4
    e = L["MobilenetV2/expanded_conv_3/expand"]
    bad = LL.copy_run(good)
    bad["grads"][e.weight_name] = good["grads"][e.weight_name] * (1 + 1e-4)
    assert _failing(bad, composite, bars, e)[0] == {("B1", e.weight_name)}

    # 2. dgamma of a recompute block's expand layer with the variance over n - 1 samples
    e = L["MobilenetV2/expanded_conv_5/expand"]
    gname = e.scope + "/BatchNorm/gamma:0"
    z, g = run["z"][e.idx], LL._leaf(run["params"][gname])
    n = z.numel() // z.shape[1]
    mu = z.mean(dim=(0, 2, 3), keepdim=True)
    y = (z - mu) * torch.rsqrt(((z - mu) ** 2).sum(dim=(0, 2, 3), keepdim=True) / (n - 1) + e.bn_eps) * g.view(1, -1, 1, 1)
    bad = LL.copy_run(good)
    bad["grads"][gname] = torch.autograd.grad((y * full.mask(e) * full.cot_a(e.idx)).sum(), g)[0]
    assert _failing(bad, composite, bars, e)[0] == {("B2", gname)}

    # 3. the skip gradient into a recompute block's input gradient taken from the neighbouring block (blocks 4 and 5: same shape)
    a, b = L["MobilenetV2/expanded_conv_4/project"], L["MobilenetV2/expanded_conv_5/project"]
    src = full.by_idx[a.residual_from]
    bad = LL.copy_run(good)
    bad["da"][a.idx] = good["da"][b.idx]
    got = _failing(bad, composite, bars, a)[0]
    assert {("DA", a.scope), ("B2", src.scope)} <= got <= {("DA", a.scope), ("B2", src.scope), ("B2", src.scope + "/BatchNorm/gamma:0"),
                                                            ("B2", src.scope + "/BatchNorm/beta:0")}, got

    # 4. a stride-2 recompute block's depthwise dz rolled by one pixel: every link that reads it, and no other
    d, e, p = (L["MobilenetV2/expanded_conv_3/" + s] for s in ("depthwise", "expand", "project"))
    assert d.stride == 2 and e.idx in LL.recompute_expand(SPEC)
    bad = LL.copy_run(good)
    bad["dz"][d.idx] = torch.roll(good["dz"][d.idx], 1, dims=3)
    got = _failing(bad, composite, bars, d)[0]
    front = full.by_idx[e.idx - 1]
    assert {("B1", d.weight_name), ("B2", d.scope), ("B1", e.weight_name), ("B2", e.scope + "/BatchNorm/gamma:0"), ("B2", front.scope),
            ("DA", front.scope)} <= got, got
    assert all(name.startswith((d.scope, e.scope, front.scope)) for _, name in got), got

    # 5. the stem weight gradient built from the first block's dz of the wrong frame
    stem = L["MobilenetV2/Conv"]
    wrong = LL.copy_run(good)
    wrong["dz"][2] = torch.roll(good["dz"][2], 1, dims=0)
    dz_stem = LL.Links(wrong, stored=STORED[(H, B)], bands=composite[1]).dz(stem.idx)
    bad = LL.copy_run(good)
    w = LL._leaf(full.P(stem.weight_name))
    bad["grads"][stem.weight_name] = torch.autograd.grad((full.conv(stem, full.x_in(stem), w) * dz_stem).sum(), w)[0]
    assert _failing(bad, composite, bars, stem)[0] == {("B1", stem.weight_name)}

    # 6. (dy of a late depthwise layer left unmasked: test_the_stride_16_blocks_close_where_the_handles_hold_dy, at the size where it is dy)


@pytest.mark.parametrize("H,B", SIZES[:1])
def test_mask_controls(runs64, composite, bars, H, B):
    """One mask bit of a withheld activation planted the other way round, with everything the step derives from it (the layer's dz, dgamma,
    dbeta and weight gradient, the input gradient and the BN backward of the layer in front): far outside the band it fails, inside the
    band it is resolved, reported, and every quantity passes under the resolved mask."""
    run = runs64[(H, B)]
    good = LL.withhold(run, STORED[(H, B)])
    e = [l for l in SPEC.layers if l.scope == "MobilenetV2/expanded_conv_3/expand"][0]
    front = SPEC.layers[e.idx - 2]
    assert front.residual_from is not None                                       # its da is stored: the input gradient is checked on its own
    plan = [("B1", e.idx), ("B2", e.idx), ("DA", front.idx), ("B2", front.idx)]
    ref = LL.Links(good, stored=STORED[(H, B)], bands=composite[1])
    y = ref._bn(e, ref.z(e.idx), *ref._gb(e))[0]
    dist = torch.minimum(y.abs(), (y - 6).abs())
    cot = ref.cot_a(e.idx)

    def planted(where):
        pl = LL.Links(good, stored=STORED[(H, B)], bands=composite[1])
        mk = ref.mask(e).clone()
        mk[where] = 1.0 - mk[where]
        pl._cache[("mask", e.idx)] = mk                                          # the step's own mask: this one bit the other way round
        bad = LL.copy_run(good)
        dz, dg, db, _, _ = pl._bn_backward(e, pl.cot_a(e.idx))
        w = LL._leaf(pl.P(e.weight_name))
        bad["grads"][e.weight_name] = torch.autograd.grad((pl.conv(e, pl.x_in(e), w) * dz).sum(), w)[0]
        bad["grads"][e.scope + "/BatchNorm/gamma:0"], bad["grads"][e.scope + "/BatchNorm/beta:0"] = dg, db
        bad["da"][front.idx] = pl.cot_a(front.idx)
        dz, dg, db, _, _ = pl._bn_backward(front, bad["da"][front.idx])
        bad["dz"][front.idx] = dz
        bad["grads"][front.scope + "/BatchNorm/gamma:0"], bad["grads"][front.scope + "/BatchNorm/beta:0"] = dg, db
        return bad

    inside = cot.abs() * ((y - 3).abs() < 2)                                     # the largest cotangent on an element well between the knees
    far = tuple(torch.nonzero(inside == inside.max())[0].tolist())
    assert dist[far] > 0.5
    got, links = _failing(planted(far), composite, bars, e, plan=plan)
    assert ("B2", e.scope + "/BatchNorm/beta:0") in got and links.ambiguous[e.idx]["resolved"] == 0, got

    near = tuple(torch.nonzero(dist == dist.min())[0].tolist())
    bands = dict(composite[1])
    bands[e.idx] = max(bands[e.idx], 2 * float(dist[near]))                       # this control's own band: the nearest element is inside it
    got, links = _failing(planted(near), composite, bars, e, bands=bands, plan=plan)
    print(LL.ambiguity_report(links))
    assert not got and links.ambiguous[e.idx]["resolved"] == 1, (got, links.ambiguous[e.idx])
    # ... and without the band the same run fails: the bit is no rounding
    bands[e.idx] = 0.0
    assert _failing(planted(near), composite, bars, e, bands=bands, plan=plan)[0]


# ---------------------------------------------------------------------------------------------------------
# the data-parallel step: runs of the ranks joined into the run of the whole batch (LL.join_rank_runs)
# ---------------------------------------------------------------------------------------------------------
DP_CASE = (62, 4)                          # odd maps; 4 frames over two ranks (case A of tests/test_gpu_dp_links.py)
DP_SHARDS = ((0, 3), (3, 4))               # uneven: local and global row counts differ on every layer


@pytest.fixture(scope="module")
def dp():
    """the f32 CPU oracle's step of the whole batch as the stand-in for a synchronised step, and the bars of its own size"""
    return LL.f32_run(*DP_CASE), LL.bars_from_levels(LL.f32_levels((DP_CASE,)))


def _rank_slice(run, lo, hi):
    """What the rank that holds frames lo .. hi - 1 leaves of a synchronised step: its rows of every batched tensor, and the whole
    batch's gradients, moving statistics and loss."""
    out = LL.copy_run(run)
    for key in ("frames", "labels", "logits", "dlogits"):
        out[key] = run[key][lo:hi]
    for kind in ("z", "a", "dz", "da", "y", "dy"):
        out[kind] = {i: t[lo:hi] for i, t in run[kind].items()}
    return out


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


def _backward_plan(links):
    plan = []
    for l in links.spec.layers:
        plan.append(("B1", l.idx))
        if l.bn_eps is not None:
            plan.append(("B2", l.idx))
        if l.residual_from is not None:
            plan.append(("DA", l.idx))
    return plan


def _rank_grads(links, lo, hi):
    """What frames lo .. hi - 1 alone add to every gradient of the run's step: the f64 links B1 and B2 (statistics, mask and cotangent of
    the WHOLE batch) summed over those rows only.  The engine forms exactly this on a rank before the gradient all-reduce."""
    g = {}
    for l in links.spec.layers:
        x, dz = links.x_in(l).detach()[lo:hi], links.dz(l.idx)[lo:hi]
        w = LL._leaf(links.P(l.weight_name))
        g[l.weight_name] = torch.autograd.grad((links.conv(l, x, w) * dz).sum(), w)[0]
        if l.bn_eps is None:
            g[l.scope + "/biases:0"] = dz.sum(dim=(0, 2, 3))
            continue
        gamma, beta = (LL._leaf(t) for t in links._gb(l))
        y, _, _ = links._bn(l, links.z(l.idx), gamma, beta)
        dg, db = torch.autograd.grad((y * links.mask(l) * links.cot_a(l.idx))[lo:hi].sum(), [gamma, beta])
        g[l.scope + "/BatchNorm/gamma:0"], g[l.scope + "/BatchNorm/beta:0"] = dg, db
    return g


def _grad_names(spec):
    w = {l.weight_name for l in spec.layers} | {spec.layers[-1].scope + "/biases:0"}
    dg = {l.scope + "/BatchNorm/gamma:0" for l in spec.layers if l.bn_eps is not None}
    db = {l.scope + "/BatchNorm/beta:0" for l in spec.layers if l.bn_eps is not None}
    assert len(w | dg | db) == 164
    return w, dg, db


def test_rank_runs_joined_are_the_run_of_the_whole_batch(dp):
    """(a) of the data-parallel proofs: cut into 3 + 1 frames and joined, the run is the original, tensor for tensor, and passes every link"""
    run, bars = dp
    ranks = [_rank_slice(run, lo, hi) for lo, hi in DP_SHARDS]
    assert [r["frames"].shape[0] for r in ranks] == [3, 1]
    joined = LL.join_rank_runs(ranks)
    assert _same(joined, run)
    res = LL.Links(joined).close()
    assert {r.kind for r in res} == set(LL.KINDS) and len(res) == 3 + 55 + 56 + 54 + 2 * 54 + (3 * 54 - 1) + 10
    assert not LL.failures(res, bars)
    # rank order matters: the shards the other way round are another batch, and the loss no longer belongs to it
    swapped = LL.join_rank_runs(ranks[::-1])
    assert not _same(swapped["z"], run["z"])


def test_unsynchronised_batch_norm_fails_its_links(dp):
    """(b): each rank's own oracle step normalises with the statistics of its own rows.  The ranks then disagree on gradients and
    statistics (the join refuses them); taken as one run anyway, BN + activation, the moving statistics and the BN backward of every
    layer fail, the convolutions (frame by frame the same operation) do not."""
    _, bars = dp
    frames, labels = LL.case_clip(*DP_CASE)
    ranks = [LL.oracle_run(LL.case_weights(), LL.CI, frames[lo:hi], labels[lo:hi], torch.float32) for lo, hi in DP_SHARDS]
    with pytest.raises(AssertionError, match="grads of MobilenetV2/Conv/weights:0 on rank 1"):
        LL.join_rank_runs(ranks)
    links = LL.Links(LL.join_rank_runs(ranks, identical=False))
    bad = LL.failures(links.close(), bars)
    bn = [l for l in links.spec.layers if l.bn_eps is not None]
    assert {r.name for r in bad if r.link == "F2"} == {l.scope for l in bn}
    # every moving variance; a moving mean may survive: behind a project layer without a skip each rank's own BN leaves the same mean (beta),
    # so the expand layer's batch mean is the same on every rank
    assert {r.name for r in bad if r.link == "F3"} >= {n for n in links.r["stats_after"] if n.endswith("moving_variance:0")}
    assert len(links.r["stats_after"]) == 108
    assert {r.name for r in bad if r.link == "B2" and r.kind == "dz"} == {l.scope for l in bn if l is not links.lp}
    assert {r.name for r in bad if r.kind == "dgamma"} == {l.scope + "/BatchNorm/gamma:0" for l in bn}
    assert not [r for r in bad if r.link == "F1"]


def test_gradients_not_summed_or_summed_twice_fail_their_links(dp):
    """(c) and (d): the step's gradients replaced by what rank 0's frames alone add to them (the gradient all-reduce left out) fail the
    weight-gradient link and the dgamma / dbeta links of every layer and nothing else; dgamma / dbeta formed from the sums AFTER their
    cross-rank sum and then added up by the gradient all-reduce come out twice as large, and fail.  The two ranks' shares added up
    pass: the shares are the step's own."""
    run, bars = dp
    joined = LL.join_rank_runs([_rank_slice(run, lo, hi) for lo, hi in DP_SHARDS])
    links = LL.Links(joined)
    plan = _backward_plan(links)
    weights, dgamma, dbeta = _grad_names(links.spec)
    share = [_rank_grads(links, lo, hi) for lo, hi in DP_SHARDS]

    def failing(grads):
        bad = LL.copy_run(joined)
        bad["grads"] = grads
        return {r.name for r in LL.failures(LL.Links(bad).close(plan), bars)}

    assert not failing({k: share[0][k] + share[1][k] for k in share[0]})
    assert failing(share[0]) == weights | dgamma | dbeta                         # (c): every gradient tensor, no dz and no da
    twice = dict(joined["grads"])
    for k in dgamma | dbeta:
        twice[k] = 2.0 * joined["grads"][k]
    got = failing(twice)                                                        # (d)
    # dbeta of a project layer is 0 in real arithmetic (the training-mode BN behind it removes a constant), and so is twice it
    zero = {l.scope + "/BatchNorm/beta:0" for l in links.backbone if l.act == "none"}
    assert dgamma | (dbeta - zero) <= got <= dgamma | dbeta, (dgamma | dbeta) - got


def test_join_refuses_ranks_that_disagree(dp):
    """(e): one moving statistic one ulp off on one rank, and the loss: the join names what differs"""
    run, _ = dp
    ranks = [_rank_slice(run, lo, hi) for lo, hi in DP_SHARDS]
    name = "MobilenetV2/expanded_conv_9/depthwise/BatchNorm/moving_variance:0"
    ranks[1]["stats_after"][name] = torch.nextafter(run["stats_after"][name], torch.full_like(run["stats_after"][name], 1e30))
    with pytest.raises(AssertionError, match="stats_after of " + name + " on rank 1"):
        LL.join_rank_runs(ranks)
    ranks = [_rank_slice(run, lo, hi) for lo, hi in DP_SHARDS]
    ranks[1]["loss"] = (run["loss"][0] * (1 + 1e-12), run["loss"][1])
    with pytest.raises(AssertionError, match="loss"):
        LL.join_rank_runs(ranks)
