"""The DATA-PARALLEL fine-tune step held to f64 link by link, teacher-forced (tests/layer_links.py; the joined run proved on the CPU in
tests/test_layer_links_cpu.py, (e)).

With an all-reduce the engine runs other kernels and other wiring than the single-process step of tests/test_gpu_layer_links.py:
forward BN through launch_colstats / launch_partials_to_sums, the cross-rank sum and launch_bn_finalize (engine_forward.hip, bn_train
and bn_from_partials); backward BN through launch_bn_bwd_reduce / launch_partials_to_sums, launch_bn_param_grads from the LOCAL sums,
the cross-rank sum and launch_bn_bwd_coef without dgamma / dbeta (engine_backward.hip, bn_backward and bn_bwd_from_partials); local row
counts beside global ones; loss sum and valid count summed before the backward; one flat gradient sum before Adam.

ONE RANK.  train_step(allreduce=<reduce function that does nothing>, global_batch=B) takes every one of those branches in one process
(the same with a genuine one-rank RCCL communicator, the engine issuing ncclAllReduce itself), and its run is a plain run: the cases,
plans, fixtures and BARS of tests/test_gpu_layer_links.py, unchanged.  No bit equality with the plain step is asked (the f64 second
stages add in another order); the measure is f64.

TWO RANKS (gloo, both on device 0, ArenaAllReduce), spawned once for the module; every rank saves its run of each case:
  A  layerwise step, 62x124, global batch 4 as 3 + 1 frames: odd maps, local rows and batch differ from the global ones on every layer
  B  default step, 64x128, global batch 4 as 2 + 2 frames: both plans; what the step stores is keyed on LOCAL rows
     (default_step_stored(spec, 64, 2), the same set on both ranks and at the global batch: asserted)
layer_links.join_rank_runs asserts the data-parallel invariant (gradients, moving statistics and loss bit-identical on the ranks) and
concatenates the shards; the links close over the joined run.  Bars by the module's rule, 4 x the f32 CPU oracle's own error, with the
oracle run at the GLOBAL size of the case: ((62, 4),) and ((64, 4),).  Never from the engine; none above 1e-4.

MEASURED on an MI355X, the engine's worst error per link kind | its bar (what _hold prints).  No link failed, on one rank or two:
                A, every link          B, default_step_plan   B, composite plan
  conv_stem     2.7e-7 | 1e-5          2.0e-7 | 1e-5          -
  conv_dw       1.8e-7 | 1e-5          -                      2.5e-7 | 9.9e-7
  conv_1x1      8.0e-7 | 2e-5          6.3e-7 | 2e-5          8.2e-7 | 3.5e-6
  bn_act        2.0e-7 | 9.6e-7        2.0e-7 | 9.3e-7        -
  stats         1.1e-7 | 4.7e-7        9.3e-8 | 5.0e-7        6.9e-8 | 4.5e-7
  loss          1.2e-8 | 1.2e-7        1.1e-8 | 1.2e-7        -
  wgrad         5.4e-7 | 1.8e-6        1.6e-7 | 1.3e-6        1.1e-7 | 6.8e-7
  dz            1.0e-6 | 4.2e-6        8.2e-7 | 3.4e-6        4.4e-7 | 2.4e-6
  dgamma        2.1e-7 | 1.3e-6        1.9e-7 | 8.9e-7        1.3e-7 | 5.0e-7
  dbeta         2.3e-7 | 1.4e-6        1.6e-7 | 1.2e-6        7.6e-8 | 2.8e-7
  da            1.1e-6 | 2e-5          1.1e-6 | 2e-5          4.5e-7 | 2.6e-6
One rank, at the bars of tests/test_gpu_layer_links.py: the errors of the single-process step to within its own scatter (worst: a of
image_pooling at 64x128 x 2, 3.0e-6 | 3.4e-6, as there); callback and RCCL transport give the same figures.
(The f32 CPU levels behind the bars move by some ten percent with the oracle's thread count.)
"""
import datetime
import os
import socket
import time

import pytest
import torch

import layer_links as LL
from ams_amd.engine import StudentEngine
from test_gpu_layer_links import _hold, _hold_composite

pytestmark = pytest.mark.gpu

COLLECTIVES = 54 * 2 + 2                   # BN forward + BN backward per layer, loss, gradients


@pytest.fixture(scope="module")
def bars():
    return LL.bars_from_levels(LL.f32_levels())


@pytest.fixture(scope="module")
def composite():
    return LL.composite_bars(LL.f32_composite_levels()), LL.f32_bands()


def _set_layerwise(eng):
    # every fine-tune fusion off: the state in which include/ams_hip.h promises that z, a, da and dz of every layer are written
    eng.set_train_recompute(False, fuse_dgrad_bn=0, fuse_gemm_red=0)
    eng.set_fuse_operand_bn(0)


def _engine_run(H, B, transport="callback", layerwise=True):
    """One train_step as a run.  ``transport``: None = the single-process step; "callback" = the data-parallel step of one rank through a
    host callback whose reduce function does nothing; "rccl" = the same through a genuine one-rank RCCL communicator."""
    from ams_amd.dist import ArenaAllReduce, RcclComm
    W = LL.case_weights()
    frames, labels = LL.case_clip(H, B)
    eng = StudentEngine(LL.CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W)
    if layerwise:
        _set_layerwise(eng)
    if transport is None:
        loss = eng.train_step(frames, labels, 1e-3)
    elif transport == "callback":
        red = ArenaAllReduce(eng.arena, reduce_fn=lambda t: None)
        loss = eng.train_step(frames, labels, 1e-3, allreduce=red, global_batch=B)
        assert red.calls == COLLECTIVES
    else:
        assert transport == "rccl"
        comm = RcclComm(0, 1, torch.device("cuda:0"), real_single_rank=True)
        loss = eng.train_step(frames, labels, 1e-3, comm=comm, global_batch=B)
        torch.cuda.synchronize()
        assert comm.stats()[0] == COLLECTIVES
        comm.close()
    torch.cuda.synchronize()
    run = LL.engine_run(eng, W, LL.CI, frames, labels, loss)           # W: the parameters before Adam changed them
    eng.close()
    return run


def _hold_default(tag, H, B, run, bars, composite):
    """both plans of the default step over ``run`` of B frames"""
    links = LL.Links(run)
    plan = LL.default_step_plan(links)
    assert len(plan) == len(set(plan)) == 1 + 15 + 20 + 48 + 14 + 14 + 7
    _hold(tag + ", default_step_plan", links.close(plan), bars)
    res = _hold_composite(tag + ", composite links", H, B, run, *composite)      # asserts that the two plans name all 164 + 108 tensors
    assert not [r for r in res if r.name.endswith(" (dy)")]


# ---------------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,B", [(64, 2), (34, 5)])
def test_every_link_of_the_layerwise_step_one_rank(bars, H, B):
    res = LL.Links(_engine_run(H, B)).close()
    assert {r.kind for r in res} == set(LL.KINDS) - {"dlogits"}
    _hold("one rank, layerwise %dx%d x %d" % (H, 2 * H, B), res, bars)


@pytest.mark.parametrize("H,B", [(64, 2), (62, 3)])
def test_every_link_of_the_default_step_one_rank(bars, composite, H, B):
    _hold_default("one rank, default step %dx%d x %d" % (H, 2 * H, B), H, B, _engine_run(H, B, layerwise=False), bars, composite)


def test_late_blocks_of_the_default_step_with_fused_gemms_one_rank():
    """128x256 x 2 (layer_links.FUSED_SIZE): only here do bn_bwd_from_partials and bn_from_partials run their cross-rank form on the partial
    rows of the stride-16 blocks' fused kernels (the project layers' input-gradient GEMMs, launch_depthwise_dgrad_bn2, the forward GEMMs'
    epilogues).  Bars and bands as in test_late_blocks_of_the_default_step_with_fused_gemms."""
    H, B = LL.FUSED_SIZE
    sizes = (LL.FUSED_SIZE,)
    levels, bands = LL.f32_composite_levels(sizes, late=True), LL.f32_bands(sizes)
    res = _hold_composite("one rank, default step, stride-16 blocks, %dx%d x %d" % (H, 2 * H, B), H, B, _engine_run(H, B, layerwise=False),
                          LL.composite_bars(levels), bands, late=True)
    assert len([r for r in res if r.name.endswith(" (dy)")]) == 10                # every late depthwise handle was checked as dy


def test_every_link_of_the_default_step_one_rank_rccl(bars, composite):
    """The production transport: the engine's own ncclAllReduce calls on the launch stream between the same kernels."""
    _hold_default("one rank (RCCL), default step 64x128 x 2", 64, 2, _engine_run(64, 2, "rccl", layerwise=False), bars, composite)


# ---------------------------------------------------------------------------------------------------------
# two ranks, joined
# ---------------------------------------------------------------------------------------------------------
#          tag  H   shards of the global batch  layerwise
CASES = (("A", 62, ((0, 3), (3, 4)), True),
         ("B", 64, ((0, 2), (2, 4)), False))
WORLD = 2
GROUP_TIMEOUT_S, PARENT_TIMEOUT_S = 120, 300


def _rank_worker(rank, world, port, tmp):
    import torch.distributed as dist
    from ams_amd.dist import ArenaAllReduce, init_from_env
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    init_from_env("gloo", timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))
    W = LL.case_weights()
    for tag, H, shards, layerwise in CASES:
        GB = shards[-1][1]
        frames, labels = LL.case_clip(H, GB)
        b, e = shards[rank]
        eng = StudentEngine(LL.CI, H, 2 * H, max_batch=e - b, trainable=True)
        eng.load_variables(W)
        if layerwise:
            _set_layerwise(eng)
        red = ArenaAllReduce(eng.arena)
        loss = eng.train_step(frames[b:e], labels[b:e], 1e-3, allreduce=red, global_batch=GB)
        torch.cuda.synchronize()
        run = LL.engine_run(eng, W, LL.CI, frames[b:e], labels[b:e], loss)
        run["collectives"] = red.calls
        torch.save(run, os.path.join(tmp, "%s_rank%d.pt" % (tag, rank)))
        eng.close()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def rank_runs(tmp_path_factory):
    """{tag: [run of rank 0, run of rank 1]}: both ranks spawned once; a rank that dies or hangs ends the wait"""
    import torch.multiprocessing as mp
    tmp = tmp_path_factory.mktemp("dp_links")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.spawn(_rank_worker, args=(WORLD, port, str(tmp)), nprocs=WORLD, join=False)
    deadline = time.monotonic() + PARENT_TIMEOUT_S
    while not ctx.join(timeout=5):                  # raises when a rank failed (and ends the other)
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail("the ranks did not finish within %d s" % PARENT_TIMEOUT_S)
    out = {tag: [torch.load(tmp / ("%s_rank%d.pt" % (tag, r)), weights_only=False) for r in range(WORLD)] for tag, *_ in CASES}
    for f in tmp.iterdir():
        f.unlink()                                  # tens of megabytes a rank and case
    for runs in out.values():
        assert [r.pop("collectives") for r in runs] == [COLLECTIVES] * WORLD
    return out


def test_every_link_of_the_layerwise_step_two_ranks(rank_runs):
    tag, H, shards, _ = CASES[0]
    GB = shards[-1][1]
    assert [r["frames"].shape[0] for r in rank_runs[tag]] == [3, 1]
    run = LL.join_rank_runs(rank_runs[tag])
    assert run["frames"].shape[0] == GB == 4
    res = LL.Links(run).close()
    assert {r.kind for r in res} == set(LL.KINDS) - {"dlogits"}
    _hold("two ranks (3 + 1), layerwise %dx%d x %d" % (H, 2 * H, GB), res, LL.bars_from_levels(LL.f32_levels(((H, GB),))))


def _case_b(rank_runs):
    """case B joined (once), its global size and the batch its storing rules are keyed on"""
    tag, H, shards, _ = CASES[1]
    GB = shards[-1][1]
    sp = LL.S.build_spec()
    # every storing rule of the engine is keyed on a rank's own rows: the same set on every rank, and the one the f32 CPU oracle's bars
    # and bands at the global size are measured with
    stored = {LL.default_step_stored(sp, H, e - b) for b, e in shards}
    assert len(stored) == 1 and stored == {LL.default_step_stored(sp, H, GB)}
    if "joined" not in rank_runs:
        rank_runs["joined"] = LL.join_rank_runs(rank_runs[tag])               # a rank out of step fails every test that asks
    run = rank_runs["joined"]
    assert run["frames"].shape[0] == GB == 4
    return run, H, GB, shards[0][1] - shards[0][0]


def test_links_of_the_default_step_two_ranks(rank_runs):
    run, H, GB, _ = _case_b(rank_runs)
    links = LL.Links(run)
    plan = LL.default_step_plan(links)
    assert len(plan) == len(set(plan)) == 1 + 15 + 20 + 48 + 14 + 14 + 7
    _hold("two ranks (2 + 2), default step %dx%d x %d, default_step_plan" % (H, 2 * H, GB), links.close(plan),
          LL.bars_from_levels(LL.f32_levels(((H, GB),))))


def test_every_link_of_the_default_step_two_ranks(rank_runs):
    run, H, GB, local = _case_b(rank_runs)
    sizes = ((H, GB),)
    res = _hold_composite("two ranks (2 + 2), default step %dx%d x %d, composite links" % (H, 2 * H, GB), H, local, run,
                          LL.composite_bars(LL.f32_composite_levels(sizes)), LL.f32_bands(sizes))      # asserts: all 164 + 108 tensors named
    assert not [r for r in res if r.name.endswith(" (dy)")]
