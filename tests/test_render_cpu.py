"""The host side of the picture path: the PNG writer (ams_amd/png.py), the table block of the render kernel (ams_amd/render.py:
build_tables) and `run.py --save_pic` with the CPU stand-in network behind the SemanticNetwork boundary."""
import glob
import os
import random
import struct
import zlib

import numpy as np
import pytest

from ams_amd import exp_configs, png, render
from ams_amd.semantic_network import SemanticNetwork
from ams_amd.utils import colormap
from oracle.oracle_network import OracleSemanticNetwork
from sched_cases import _main

SUBSETS = {"six": [0, 1, 2, 10, 11, 13], "all19": list(range(19)), "without_class_0": [5, 7, 18]}


def decode_png(data):
    """A decoder for what the writer may produce: 8-bit grey or RGB, one or more IDAT chunks, filter type 0 on every row.  Checks the
    signature and every chunk's CRC; returns (array, chunk names)."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks, idat, header = 8, [], b"", None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(kind + body) & 0xFFFFFFFF, kind
        chunks.append(kind)
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert pos == len(data) and chunks[0] == b"IHDR" and chunks[-1] == b"IEND" and b"IDAT" in chunks
    w, h, depth, colour, compression, filt, interlace = header
    assert depth == 8 and colour in (0, 2) and (compression, filt, interlace) == (0, 0, 0)
    channels = 1 if colour == 0 else 3
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + w * channels)
    assert not rows[:, 0].any(), "filter type 0 on every row"
    image = rows[:, 1:]
    return (image.reshape(h, w) if colour == 0 else image.reshape(h, w, 3)), chunks


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (64, 128)])
@pytest.mark.parametrize("rgb", [False, True])
def test_png_round_trip(tmp_path, shape, rgb):
    rng = np.random.default_rng(shape[0] * 7 + int(rgb))
    image = rng.integers(0, 256, shape + ((3,) if rgb else ()), dtype=np.uint8)
    data = png.encode(image)
    got, chunks = decode_png(data)
    assert chunks == [b"IHDR", b"IDAT", b"IEND"]
    assert got.dtype == np.uint8 and got.shape == image.shape and np.array_equal(got, image)
    assert png.encode(image.copy()) == data                               # the bytes depend on the image alone
    png.write(str(tmp_path / "a.png"), image)
    png.write(str(tmp_path / "b.png"), image)
    assert open(tmp_path / "a.png", "rb").read() == open(tmp_path / "b.png", "rb").read() == data
    with pytest.raises(AssertionError):
        png.encode(image.astype(np.int32))


def _network_tables(subset, total=19):
    """color_map_reduced_ / take_array exactly as SemanticNetwork.__init__ forms them"""
    cw = np.zeros((total, 1))
    cw[subset] = 1
    reduced = np.take(colormap(), np.where(cw == 1)[0], axis=0)
    ranks = np.cumsum(cw).reshape(total) * cw.reshape(total)
    take = np.where(ranks != 0, ranks - 1, ranks).astype(int)
    return reduced, take


@pytest.mark.parametrize("name", sorted(SUBSETS))
def test_table_block_holds_the_three_tables(name):
    subset = SUBSETS[name]
    reduced, take = _network_tables(subset)
    block = render.build_tables(reduced, colormap(), take, 19)
    assert block.dtype == np.uint8 and block.shape == (render.TABLE_BYTES,) and render.TABLE_BYTES == 256 * 3 + 32 * 3 + 256
    assert np.array_equal(block[:768].reshape(256, 3), colormap())
    k = len(subset)
    assert np.array_equal(block[768:768 + 3 * k].reshape(k, 3), reduced) and not block[768 + 3 * k:864].any()
    assert np.array_equal(block[864:864 + 19], take) and not block[864 + 19:].any()          # entries from TOTAL_CLASSES on are zero
    # the take table is the inverse of the subset, with 0 for every class outside it: index 0 is a real class AND "ignored"
    for c in range(19):
        assert block[864 + c] == (subset.index(c) if c in subset else 0)
    if name == "without_class_0":
        assert block[864 + 5] == 0 and block[864 + 0] == 0
    assert np.array_equal(render.build_tables(reduced, colormap(), take), block)           # total_classes defaults to len(take_array)
    with pytest.raises(AssertionError):
        render.build_tables(reduced[:1], colormap(), take, 19)                               # take_array points past the reduced palette


class PaintingOracleNetwork(OracleSemanticNetwork):
    """The CPU stand-in with the product class's NumPy painting helpers (it has none of its own), logging every per-frame call."""
    WHITE, BLACK = SemanticNetwork.WHITE, SemanticNetwork.BLACK
    CALLS = []
    _check_hw = SemanticNetwork._check_hw
    _on_device = staticmethod(SemanticNetwork._on_device)
    _overlay = staticmethod(SemanticNetwork._overlay)
    _paint = SemanticNetwork._paint
    colorize = SemanticNetwork.colorize
    colorize_teacher = SemanticNetwork.colorize_teacher
    cross_ignore = SemanticNetwork.cross_ignore

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        self.color_map_reduced_, self.take_array = _network_tables(list(self.class_indices), self.TOTAL_CLASSES)

    def predict_with_metric(self, frames, labels_teacher):
        res = super().predict_with_metric(frames, labels_teacher)
        if self.frozen:
            self.CALLS.append((np.array(frames[0]), np.array(labels_teacher[0]), np.array(res[0][0])))
        return res


def _run(out, extra):
    np.random.seed(5)
    random.seed(5)
    PaintingOracleNetwork.CALLS = []
    s = _main(PaintingOracleNetwork, ["--input_video", "synthetic:25-synth:seconds=3:fps=3", "--student_checkpoint", "synthetic:0", "--output_dir", out,
                                      "--gpu", "0", "--mode", "simple", "--height", "64", "--batch_size", "2", "--iter", "1", "--send_period", "3",
                                      "--train_period", "2", "--first_train_time", "2", "--memory_len", "4"] + extra)
    assert s["frames"] == 9
    return list(PaintingOracleNetwork.CALLS)


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("plain")) + "/"
    _run(out, [])
    return out


@pytest.mark.parametrize("depth", [1, 2])
def test_save_pic_writes_the_surviving_frames(tmp_path, plain_run, depth):
    """3 s at 3 frames per second: `i` runs 1 .. 9 after its increment, the label is i // fps, and the last frame of each label survives:
    i = 2, 5, 8 (labels 0, 1, 2) and i = 9 (the clip's last frame, label 3).  Eight files each, holding what the helpers paint."""
    out = str(tmp_path / "pics") + "/"
    calls = _run(out, ["--save_pic"] + (["--edge_pipeline", "2"] if depth == 2 else []))
    assert len(calls) == 9
    files = sorted(glob.glob(out + "*.png"))
    stem = glob.glob(out + "*_results*_mious.npy")[0][:-len("_mious.npy")]
    want = sorted("%s_%d_%s.png" % (stem, label, name) for label in (0, 1, 2, 3)
                  for name in ("cross_mask", "ignore_mask", "overlay_teacher", "output_teacher", "output_student", "overlay_student", "frame",
                               "label_student"))
    assert files == want
    net = PaintingOracleNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=64, frozen=True,
                                frozen_graph=_frozen(sorted(glob.glob(out + "*_final.pb"))[0]))
    for label, i_next in ((0, 2), (1, 5), (2, 8), (3, 9)):
        frame, gt, student = calls[i_next - 1]
        frame = frame.astype(np.uint8)
        # the clip marks unlabelled pixels with 255, which the helper's take table does not cover: ignored (white / black), like the metric
        known = gt < 19
        assert not known.all() and known.any()
        cross, ignore = net.cross_ignore(label_teacher=np.where(known, gt, 0), label_student=student)
        cross[~known], ignore[~known] = 0, 255
        colour_t, overlay_t = net.colorize_teacher(label=gt, frame=frame)
        colour_s, overlay_s = net.colorize(label=student, frame=frame)
        expect = {"cross_mask": cross, "ignore_mask": ignore, "overlay_teacher": overlay_t, "output_teacher": colour_t, "output_student": colour_s,
                  "overlay_student": overlay_s, "frame": frame, "label_student": student.astype(np.uint8)}
        for name, image in expect.items():
            got, _ = decode_png(open("%s_%d_%s.png" % (stem, label, name), "rb").read())
            assert got.shape == image.shape and np.array_equal(got, image), (label, name)
        assert overlay_s.any() and not np.array_equal(overlay_s, colour_s)           # the overlay_* files hold overlays, not the bare colours
    # every other output of the run is the run's without the flag
    _same_npy(plain_run, out)


def _frozen(path):
    from ams_amd.semantic_network import FrozenGraph
    with open(path, "rb") as f:
        return FrozenGraph.ParseFromString(f.read())


def _same_npy(a_dir, b_dir):
    names = sorted(os.path.basename(p) for p in glob.glob(a_dir + "*.npy"))
    assert names == sorted(os.path.basename(p) for p in glob.glob(b_dir + "*.npy")) and len(names) >= 9
    for name in names:
        a, b = np.load(a_dir + name), np.load(b_dir + name)
        if name.endswith("_train_ms.npy"):                                 # wall-clock times
            assert a.shape == b.shape
        else:
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), name


def test_without_save_pic_nothing_changes(tmp_path, plain_run):
    """No PNG without the flag, and the .npy files do not depend on it (the loop itself is pinned by tests/test_scheduler_cpu.py and
    tests/golden/scheduler_oracle_run.json, which this change leaves as they are)."""
    assert glob.glob(plain_run + "*.png") == []
    again = str(tmp_path / "again") + "/"
    _run(again, [])
    _same_npy(plain_run, again)
    with pytest.raises(AssertionError):
        _run(str(tmp_path / "bad") + "/", ["--device_render"])              # the flag paints --save_pic's pictures: it needs it
