"""The picture path on the device (k_render.hip, ams_amd/render.py) against the NumPy helpers of SemanticNetwork, bit for bit: the kernel
through the C ABI (both paths, both label types, three class subsets), the rounding of the blend, view selection, labels out of range, refused
calls, the SemanticNetwork methods, and the scheduler with --save_pic / --device_render."""
import ctypes as C
import filecmp
import glob
import gzip
import os
import random

import numpy as np
import pytest
import torch

from ams_amd import exp_configs, hip, render, run as R, spec as S, synth, weights as Wt
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
from ams_amd.utils import colormap

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CI = [0, 1, 2, 10, 11, 13]
SUBSETS = {"six": CI, "all19": list(range(19)), "without_class_0": [5, 7, 18]}
SENTINEL = 7


class HostPainter:
    """The NumPy helpers of SemanticNetwork themselves (the yardstick) on the tables SemanticNetwork.__init__ forms, without an engine and
    without the 2:1 shape assertion, so that they can be asked about any [H, W]."""
    WHITE = SemanticNetwork.WHITE
    _on_device = staticmethod(SemanticNetwork._on_device)
    _overlay = staticmethod(SemanticNetwork._overlay)
    _paint = SemanticNetwork._paint
    colorize = SemanticNetwork.colorize
    colorize_teacher = SemanticNetwork.colorize_teacher
    cross_ignore = SemanticNetwork.cross_ignore

    def __init__(self, subset, total=19):
        cw = np.zeros((total, 1))
        cw[subset] = 1
        self.total = total
        self.color_map_reduced_ = np.take(colormap(), np.where(cw == 1)[0], axis=0)
        ranks = np.cumsum(cw).reshape(total) * cw.reshape(total)
        self.take_array = np.where(ranks != 0, ranks - 1, ranks).astype(int)

    def _check_hw(self, *args, **kw):
        pass

    def views(self, frames, student, teacher):
        """the six views [B,H,W,3] of a batch, frame by frame through the helpers"""
        out = {v: [] for v in render.VIEWS}
        for f, s, t in zip(frames, student, teacher):
            cs, os_ = self.colorize(frame=f, label=s)
            ct, ot = self.colorize_teacher(label=t, frame=f)
            # cross_ignore raises on a teacher id its take table does not cover; the documented device result there is "ignored"
            known = t < self.total
            cross, ignore = self.cross_ignore(label_teacher=np.where(known, t, 0), label_student=s)
            cross[~known], ignore[~known] = 0, 255
            for name, image in zip(render.VIEWS, (cs, os_, ct, ot, ignore, cross)):
                out[name].append(image)
        return {k: np.stack(v) for k, v in out.items()}


def _renderer(subset):
    p = HostPainter(subset)
    return p, render.DeviceRenderer(p.color_map_reduced_, colormap(), p.take_array, 19, DEV)


def _inside(array, offset):
    """the array as a device tensor that starts `offset` elements into a larger buffer (offset 1: not 16-byte aligned)"""
    a = np.ascontiguousarray(array)
    buf = torch.zeros(a.size + offset, dtype=torch.from_numpy(a).dtype, device=DEV)
    view = buf[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _inputs(shape, k, seed, s32):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    student = rng.integers(0, k, shape).astype(np.int32 if s32 else np.uint8)
    teacher = rng.integers(0, 19, shape, dtype=np.uint8)
    return frames, student, teacher


def _call(r, frames, student, teacher, outs, shape=None, k=None, dtype=None, tables=True, out_struct=True):
    """ams_render_views itself; outs: view name -> device tensor (the others NULL).  Returns the return code."""
    lib = hip.lib()
    ref = student if student is not None else teacher
    b, h, w = shape if shape is not None else tuple(ref.shape)
    if dtype is None:
        dtype = hip.DT_I32 if (student is not None and student.dtype == torch.int32) else hip.DT_U8
    o = hip.RenderOut()
    for name, t in outs.items():
        setattr(o, name, t.data_ptr())
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return lib.ams_render_views(ptr(frames), ptr(student), dtype, ptr(teacher), b, h, w, r.K if k is None else k,
                                C.c_void_p(r.tables.data_ptr()) if tables else None, C.byref(o) if out_struct else None, st)


SHAPES = {"wide_smallest_1x4x16": (1, 4, 16), "per_pixel_2x5x18": (2, 5, 18), "one_column_1x3x1": (1, 3, 1),
          "wide_shape_misaligned_3x8x48": (3, 8, 48), "two_blocks_of_rows_2x64x128": (2, 64, 128)}


@pytest.mark.parametrize("subset", sorted(SUBSETS))
@pytest.mark.parametrize("s32", [False, True], ids=["u8", "i32"])
@pytest.mark.parametrize("case", sorted(SHAPES))
def test_kernel_equals_the_host_helpers(case, s32, subset):
    shape = SHAPES[case]
    painter, r = _renderer(SUBSETS[subset])
    frames, student, teacher = _inputs(shape, r.K, seed=len(case) + 2 * s32 + r.K, s32=s32)
    want = painter.views(frames, student, teacher)
    if "misaligned" in case:
        # one element into a larger buffer: inputs and outputs off the 16-byte grid, so the wide shape takes the per-pixel path
        f, s, t = _inside(frames, 1), _inside(student, 1), _inside(teacher, 1)
        assert f.data_ptr() % 16 and s.data_ptr() % 16 and t.data_ptr() % 16
        outs = {v: _inside(np.full(shape + (3,), SENTINEL, np.uint8), 1) for v in render.VIEWS}
        assert _call(r, f, s, t, outs) == 0
        got = {v: o.cpu().numpy() for v, o in outs.items()}
    else:
        got = {v: o.cpu().numpy() for v, o in r.render(torch.from_numpy(frames).to(DEV), torch.from_numpy(student).to(DEV),
                                                         torch.from_numpy(teacher).to(DEV)).items()}
    for v in render.VIEWS:
        assert got[v].shape == want[v].shape and np.array_equal(got[v], want[v]), v
    if np.prod(shape) >= 64:                                              # the case is not hollow: all three kinds of pixel occur
        assert want["cross_mask"].any() and want["ignore_mask"].any() and not want["ignore_mask"].all()


def test_kernel_equals_the_host_helpers_at_512x1024():
    painter, r = _renderer(CI)
    frames, student, teacher = _inputs((1, 512, 1024), r.K, seed=1, s32=False)
    want = painter.views(frames, student, teacher)
    views = r.render(torch.from_numpy(frames).to(DEV), torch.from_numpy(student).to(DEV), torch.from_numpy(teacher).to(DEV))
    got = views.host()                                                   # all six in one copy
    assert list(got) == list(render.VIEWS)
    for v in render.VIEWS:
        assert np.array_equal(got[v], want[v]), v


@pytest.mark.parametrize("aligned", [True, False], ids=["wide", "per_pixel"])
def test_blend_rounds_half_to_even(aligned):
    """Every byte value 0 .. 255 under every colour of both palettes.  t = f + c is odd on a tie; t >> 1 even keeps it, t >> 1 odd rounds up."""
    painter, r = _renderer(list(range(19)))
    shape = (1, 19, 256)
    frames = np.broadcast_to(np.arange(256, dtype=np.uint8)[None, None, :, None], shape + (3,)).copy()
    teacher = np.broadcast_to(np.arange(19, dtype=np.uint8)[None, :, None], shape).copy()
    student = teacher.copy()
    t = frames.astype(np.int32) + colormap()[teacher].astype(np.int32)
    assert np.any((t & 1 == 1) & ((t >> 1) & 1 == 0)) and np.any((t & 1 == 1) & ((t >> 1) & 1 == 1)), "the input holds no tie of one kind"
    assert all(np.array_equal(np.unique(frames[0, y, :, c]), np.arange(256)) for y in range(19) for c in range(3))
    want = painter.views(frames, student, teacher)
    off = 0 if aligned else 1
    f, s, tt = _inside(frames, off), _inside(student, off), _inside(teacher, off)
    assert (f.data_ptr() % 16 == 0) == aligned
    got = r.render(f, s, tt, ("overlay_student", "overlay_teacher", "colour_teacher"))
    assert np.array_equal(got["overlay_teacher"].cpu().numpy(), want["overlay_teacher"])
    assert np.array_equal(got["overlay_student"].cpu().numpy(), want["overlay_student"])
    half = (t >> 1) + ((t & 1) & ((t >> 1) & 1))
    assert np.array_equal(got["overlay_teacher"].cpu().numpy(), half.astype(np.uint8))


@pytest.mark.parametrize("shape", [(2, 4, 32), (2, 5, 18)], ids=["wide", "per_pixel"])
def test_each_view_alone_and_nothing_else_is_written(shape):
    painter, r = _renderer(CI)
    frames, student, teacher = (torch.from_numpy(a).to(DEV) for a in _inputs(shape, r.K, seed=3, s32=False))
    every = {v: o.cpu().numpy() for v, o in r.render(frames, student, teacher).items()}
    for view in render.VIEWS:
        bufs = {v: torch.full(shape + (3,), SENTINEL, dtype=torch.uint8, device=DEV) for v in render.VIEWS}
        assert _call(r, frames, student, teacher, {view: bufs[view]}) == 0
        torch.cuda.synchronize()
        for v in render.VIEWS:
            if v == view:
                assert np.array_equal(bufs[v].cpu().numpy(), every[v]), v
            else:
                assert bool((bufs[v] == SENTINEL).all()), (view, v)


@pytest.mark.parametrize("shape", [(1, 4, 16), (1, 3, 5)], ids=["wide", "per_pixel"])
def test_labels_out_of_range_give_defined_output(shape):
    """No error and nothing read outside a table: a student label outside [0, K) paints black; a teacher id from TOTAL_CLASSES on is
    ignored (white / black) and black in colour_teacher.  The host helpers raise IndexError there."""
    painter, r = _renderer(CI)
    k = r.K
    frames, student, teacher = _inputs(shape, k, seed=4, s32=False)
    student.reshape(-1)[:3] = [k, 255, k + 1]
    teacher.reshape(-1)[4:7] = [19, 20, 255]
    with pytest.raises(IndexError):
        painter.colorize(label=student[0])
    with pytest.raises(IndexError):
        painter.cross_ignore(label_teacher=teacher[0], label_student=student[0])
    s32 = student.astype(np.int32)
    s32.reshape(-1)[:3] = [-1, k, 1 << 20]
    for st in (student, s32):
        got = {v: o.cpu().numpy().reshape(-1, 3) for v, o in r.render(frames, st, teacher).items()}
        assert not got["colour_student"][:3].any()
        assert (got["ignore_mask"][4:7] == 255).all() and not got["cross_mask"][4:7].any() and not got["colour_teacher"][4:7].any()
        # the pixels in range are the helpers'
        ok_s, ok_t = np.ones(student.size, bool), np.ones(student.size, bool)
        ok_s[:3], ok_t[4:7] = False, False
        safe_s, safe_t = np.where(ok_s.reshape(shape), st, 0), np.where(ok_t.reshape(shape), teacher, 0)
        want = {v: a.reshape(-1, 3) for v, a in painter.views(frames, safe_s, safe_t).items()}
        for v, ok in (("colour_student", ok_s), ("overlay_student", ok_s), ("colour_teacher", ok_t), ("overlay_teacher", ok_t),
                      ("ignore_mask", ok_t), ("cross_mask", ok_s & ok_t)):
            assert np.array_equal(got[v][ok], want[v][ok]), v
        # the overlay of a black pixel is the frame halved with the same rounding
        assert np.array_equal(got["overlay_student"][:3], HostPainter._overlay(frames.reshape(-1, 3)[:3], np.zeros((3, 3), np.uint8)))


REFUSED = {
    "batch_0": dict(shape=(0, 4, 16)), "height_0": dict(shape=(2, 0, 16)), "width_0": dict(shape=(2, 4, 0)), "width_negative": dict(shape=(2, 4, -16)),
    "k_0": dict(k=0), "k_33": dict(k=33), "dtype_f32": dict(dtype=hip.DT_F32), "dtype_unknown": dict(dtype=99), "no_tables": dict(tables=False),
    "no_view": dict(views=()), "no_out_struct": dict(out_struct=False),
    "colour_student_without_student": dict(views=("colour_student",), drop="s"), "cross_mask_without_student": dict(views=("cross_mask",), drop="s"),
    "cross_mask_without_teacher": dict(views=("cross_mask",), drop="t"), "ignore_mask_without_teacher": dict(views=("ignore_mask",), drop="t"),
    "colour_teacher_without_teacher": dict(views=("colour_teacher",), drop="t"), "overlay_student_without_frames": dict(views=("overlay_student",), drop="f"),
    "overlay_teacher_without_frames": dict(views=("overlay_teacher",), drop="f"),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_calls_touch_nothing(case):
    kw = dict(REFUSED[case])
    lib = hip.lib()
    painter, r = _renderer(CI)
    shape = (2, 4, 16)
    frames, student, teacher = (torch.from_numpy(a).to(DEV) for a in _inputs(shape, r.K, seed=5, s32=False))
    bufs = {v: torch.full(shape + (3,), SENTINEL, dtype=torch.uint8, device=DEV) for v in render.VIEWS}
    views = kw.pop("views", render.VIEWS)
    drop = kw.pop("drop", "")
    assert _call(r, frames, student, teacher, bufs) == 0                  # the same call, complete, is accepted
    for b in bufs.values():
        b.fill_(SENTINEL)
    rc = _call(r, None if "f" in drop else frames, None if "s" in drop else student, None if "t" in drop else teacher,
               {v: bufs[v] for v in views}, **{"shape": shape, **kw})
    msg = lib.ams_last_error()
    assert rc != 0 and msg and b"render_views" in msg
    torch.cuda.synchronize()
    assert all(bool((b == SENTINEL).all()) for b in bufs.values())


# ---------------------------------------------------------------------------------------------------- SemanticNetwork
H = 64


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(S.build_spec(), seed=0)


@pytest.fixture(scope="module")
def clip():
    return synth.SyntheticVideo(H, 3, CI, seed=5).clip()


def _edge(W0, **kw):
    return SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True, frozen_graph=FrozenGraph(W0, CI, H, 19), **kw)


@pytest.fixture(scope="module")
def edge(W0):
    net = _edge(W0, max_batch=3)
    yield net
    net.close_model()


def _host_paint(net, frames, student, teacher):
    """host painting of a batch through the network's own helpers (teacher ids the take table does not cover: ignored)"""
    p = HostPainter(CI)
    assert np.array_equal(p.take_array, net.take_array) and np.array_equal(p.color_map_reduced_, net.color_map_reduced_)
    p.colorize, p.colorize_teacher, p.cross_ignore = net.colorize, net.colorize_teacher, net.cross_ignore
    return p.views(frames, student, teacher)


def test_helpers_are_routed_by_input_type(edge, clip):
    frames, labels = clip
    frame, teacher = np.ascontiguousarray(frames[0]), np.where(labels[0] < 19, labels[0], 3).astype(np.uint8)
    student = edge.predict_input(frame[None])[0]
    f_dev, t_dev, s_dev = torch.from_numpy(frame).to(DEV), torch.from_numpy(teacher).to(DEV), torch.from_numpy(student).to(DEV)

    def same(dev, host):
        dev, host = (dev, host) if isinstance(dev, tuple) else ((dev,), (host,))
        assert len(dev) == len(host)
        for d, h in zip(dev, host):
            assert isinstance(h, np.ndarray) and isinstance(d, torch.Tensor) and d.is_cuda and d.dtype == torch.uint8
            assert tuple(d.shape) == h.shape and np.array_equal(d.cpu().numpy(), h)

    same(edge.colorize(frame=f_dev, label=s_dev), edge.colorize(frame=frame, label=student))
    same(edge.colorize(label=s_dev), edge.colorize(label=student))
    same(edge.colorize(frame=f_dev), edge.colorize(frame=frame))                     # label=None: predicted on the device
    same(edge.colorize(frame=f_dev, label=s_dev.to(torch.uint8)), edge.colorize(frame=frame, label=student))
    same(edge.colorize_teacher(t_dev, frame=f_dev), edge.colorize_teacher(teacher, frame=frame))
    same(edge.colorize_teacher(t_dev), edge.colorize_teacher(teacher))
    same(edge.cross_ignore(t_dev, label_student=s_dev), edge.cross_ignore(teacher, label_student=student))
    same(edge.cross_ignore(t_dev, frame_student=f_dev), edge.cross_ignore(teacher, frame_student=frame))
    with pytest.raises(AssertionError):
        edge.colorize(frame=f_dev[:-1], label=s_dev[:-1])
    with pytest.raises(AssertionError):
        edge.colorize()
    with pytest.raises(AssertionError):
        edge.cross_ignore(t_dev)


@pytest.mark.parametrize("n", [1, 3])
def test_predict_rendered_equals_the_plain_calls(edge, clip, n):
    frames, labels = clip[0][:n], clip[1][:n]
    assert (labels == 255).any()                                          # unlabelled pixels go through the metric and the pictures
    want = edge.predict_with_metric(frames, labels)
    got = edge.predict_rendered(frames, labels)
    assert len(got) == 6
    for g, w in zip(got[:5], want):
        assert type(g) is type(w) and np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
    assert got[0].dtype == want[0].dtype and got[0].shape == (n, H, 2 * H)
    views = got[5]
    assert list(views) == list(render.VIEWS)
    painted = _host_paint(edge, frames, want[0], labels)
    host = views.host()
    for v in render.VIEWS:
        assert views[v].is_cuda and tuple(views[v].shape) == (n, H, 2 * H, 3)
        assert np.array_equal(host[v], painted[v]) and np.array_equal(views[v].cpu().numpy(), painted[v]), v
    # device inputs, no teacher: predict_input's labels and the student's views
    labels_only, some = edge.predict_rendered(torch.from_numpy(frames).to(DEV), views=("colour_student", "overlay_student"))
    assert np.array_equal(labels_only, edge.predict_input(frames)) and labels_only.dtype == want[0].dtype
    assert np.array_equal(some["overlay_student"].cpu().numpy(), painted["overlay_student"]) and list(some) == ["colour_student", "overlay_student"]
    with pytest.raises(AssertionError):
        edge.predict_rendered(frames, views=("cross_mask",))


def test_pipelined_render_gives_the_same_per_frame(W0, edge, clip):
    frames, labels = clip
    piped = _edge(W0, pipeline_depth=2)
    try:
        tickets = [piped.predict_with_metric_async(frames[k:k + 1], labels[k:k + 1], **({"render": render.VIEWS} if k != 1 else {})) for k in range(3)]
        results = [piped.collect(t) for t in tickets]                     # the third frame's pass overwrites the label view of the first two
        for k in range(3):
            want = edge.predict_with_metric(frames[k:k + 1], labels[k:k + 1])
            assert len(results[k]) == 5
            for g, w in zip(results[k], want):
                assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
            if k == 1:
                with pytest.raises(AssertionError):
                    piped.take_rendered(tickets[k])
                continue
            views = piped.take_rendered(tickets[k])
            painted = _host_paint(edge, frames[k:k + 1], want[0], labels[k:k + 1])
            for v in render.VIEWS:
                assert np.array_equal(views[v].cpu().numpy(), painted[v]), (k, v)
        # views taken before the frame is collected: the queued frame is launched for them
        t = piped.predict_with_metric_async(frames[:1], labels[:1], render=("cross_mask",))
        early = piped.take_rendered(t)
        assert np.array_equal(early["cross_mask"].cpu().numpy(), _host_paint(edge, frames[:1], results[0][0], labels[:1])["cross_mask"])
        assert np.array_equal(piped.collect(t)[0], results[0][0])
    finally:
        piped.close_model()


# ---------------------------------------------------------------------------------------------------- scheduler
ARGS = ["--input_video", "synthetic:25-synth:seconds=3:fps=3", "--student_checkpoint", "synthetic:0", "--gpu", "0", "--mode", "simple", "--height", "64",
        "--batch_size", "2", "--iter", "1", "--send_period", "3", "--train_period", "2", "--first_train_time", "2", "--memory_len", "4", "--save_pic"]


def _scheduler(out, extra):
    """`python -m ams_amd.run` hands its arguments to run.main: called here with the same arguments, in this process"""
    np.random.seed(13)
    random.seed(13)
    summary = R.main(ARGS + ["--output_dir", out] + extra)
    assert summary["frames"] == 9
    return out


@pytest.fixture(scope="module")
def host_painted_run(tmp_path_factory):
    return _scheduler(str(tmp_path_factory.mktemp("host")) + "/", [])


@pytest.mark.parametrize("extra", [["--device_render"], ["--edge_pipeline", "2"], ["--device_render", "--edge_pipeline", "2"],
                                   ["--device_render", "--gpu_ingest"]], ids=lambda e: "+".join(x.strip("-") for x in e))
def test_scheduler_writes_the_same_directory(tmp_path, host_painted_run, extra):
    """--save_pic with the host helpers and one frame per pass is the yardstick; --device_render and --edge_pipeline 2, alone and together,
    write the same directory: PNGs byte for byte, everything else as tests/test_gpu_replay.py compares it (`_train_ms.npy` holds wall-clock
    times, the header of `_mask.dat.gz` the time it was written)."""
    a_dir, b_dir = host_painted_run, _scheduler(str(tmp_path / "other") + "/", extra)
    names = sorted(os.path.basename(p) for p in glob.glob(a_dir + "*"))
    assert names == sorted(os.path.basename(p) for p in glob.glob(b_dir + "*"))
    pngs = [n for n in names if n.endswith(".png")]
    assert len(pngs) == 4 * 8 and len([n for n in pngs if n.endswith("_overlay_student.png")]) == 4
    differ = []
    for name in names:
        a, b = a_dir + name, b_dir + name
        if name.endswith("_train_ms.npy"):
            assert np.load(a).shape == np.load(b).shape
        elif name.endswith(".gz"):
            with gzip.open(a, "rb") as fa, gzip.open(b, "rb") as fb:
                same = fa.read() == fb.read() and os.path.getsize(a) == os.path.getsize(b)
            if not same:
                differ.append(name)
        elif not filecmp.cmp(a, b, shallow=False):
            differ.append(name)
    assert differ == [], differ
