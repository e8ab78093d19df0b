"""Host side of the labels derived from teacher logits, without a GPU: the refusals of ``ams_teacher_labels_from_logits`` (they come before
anything is launched, so the library answers them on a host without a device), the synthetic teacher logits, the frame sources' logits
channel and the scheduler's flag rules."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from ams_amd import hip, run as R
from ams_amd.exp_configs import class_indices
from ams_amd.synth import SyntheticVideo
from teacher_labels_ref import grid_points, labels_from_logits

E_INVALID = -1                    # AMS_E_INVALID (include/ams_hip.h)
CI6 = (0, 1, 2, 10, 11, 13)


# ---------------------------------------------------------------------------------------------------------
# the C entry's refusals
# ---------------------------------------------------------------------------------------------------------
GOOD = dict(slot=3 * 5 * 19, n=2, lh=3, lw=5, nc=19, Hs=32, Ws=64, out=32 * 64)
REFUSED = {"n_0": dict(n=0), "n_negative": dict(n=-1), "lh_0": dict(lh=0), "lh_above_Hs": dict(lh=33), "lw_0": dict(lw=0), "lw_above_Ws": dict(lw=65),
           "nc_0": dict(nc=0), "nc_256": dict(nc=256), "slot_stride_below_the_item": dict(slot=3 * 5 * 19 - 1),
           "out_stride_below_the_map": dict(out=32 * 64 - 1), "Hs_0": dict(Hs=0), "Ws_0": dict(Ws=0), "null_logits": dict(), "null_out": dict()}


@pytest.mark.parametrize("bad", sorted(REFUSED))
def test_every_refusal_of_the_c_entry_needs_no_device(bad):
    a = dict(GOOD, **REFUSED[bad])
    logits = np.zeros(2 * 3 * 5 * 19, dtype=np.float32)          # host memory: a refused call reads and launches nothing
    out = np.full(2 * 32 * 64, 0xA5, dtype=np.uint8)
    rc = hip.lib().ams_teacher_labels_from_logits(None if bad == "null_logits" else logits.ctypes.data_as(C.c_void_p), a["slot"], a["n"], a["lh"],
                                                  a["lw"], a["nc"], a["Hs"], a["Ws"],
                                                  None if bad == "null_out" else out.ctypes.data_as(C.c_void_p), a["out"], None)
    assert rc == E_INVALID
    assert b"teacher_labels_from_logits" in hip.lib().ams_last_error()
    assert (out == 0xA5).all()


# ---------------------------------------------------------------------------------------------------------
# synthetic teacher logits
# ---------------------------------------------------------------------------------------------------------
def test_frames_do_not_depend_on_calls_to_teacher_logits():
    plain, mixed = SyntheticVideo(32, 8, CI6, seed=25), SyntheticVideo(32, 8, CI6, seed=25)
    for t in (0, 3, 7, 3):
        mixed.teacher_logits(t, 3, 5)
        mixed.teacher_logits(t + 1, 5, 9)
        (fa, la), (fb, lb) = plain.frame(t), mixed.frame(t)
        assert fa.tobytes() == fb.tobytes() and la.tobytes() == lb.tobytes()
    # ... and are the frames SyntheticVideo gave before it had teacher_logits: SHA-1 of frame + label bytes, recorded then
    f, l = SyntheticVideo(32, 5, CI6, seed=25).frame(3)
    assert hashlib.sha1(f.tobytes() + l.tobytes()).hexdigest() == "814e5c20b5b1aa4d822ffa745550544896fc5470"


def test_teacher_logits_are_deterministic():
    a = SyntheticVideo(32, 8, CI6, seed=25).teacher_logits(4, 3, 5)
    v = SyntheticVideo(32, 8, CI6, seed=25)
    v.frame(2), v.teacher_logits(1, 3, 5)
    b = v.teacher_logits(4, 3, 5)
    assert a.dtype == np.float32 and a.shape == (3, 5, 19) and a.tobytes() == b.tobytes()
    assert v.teacher_logits(5, 3, 5).tobytes() != a.tobytes()
    assert SyntheticVideo(32, 8, CI6, seed=26).teacher_logits(4, 3, 5).tobytes() != a.tobytes()


@pytest.mark.parametrize("classes,num_classes,fallback", [(CI6, 19, 3), (tuple(range(19)), 19, 0)], ids=["subset", "every_class"])
@pytest.mark.parametrize("height,grid", [(32, (3, 5)), (64, (5, 9)), (32, (32, 64))])
def test_the_restated_argmax_is_the_clean_label_on_the_grid_points(height, grid, classes, num_classes, fallback):
    """margin * onehot + noise with |noise| < margin / 4: the labelled class leads every other by more than margin / 2 in the cached sample,
    and a grid point of U is that sample itself.  Between grid points nothing is promised (two samples of different classes are blended)."""
    margin = 8.0
    v = SyntheticVideo(height, 4, classes, num_classes=num_classes, seed=25)
    for t in (0, 2):
        logits = v.teacher_logits(t, *grid, margin=margin)
        ys = np.rint(np.linspace(0, v.h - 1, grid[0])).astype(np.int64)
        xs = np.rint(np.linspace(0, v.w - 1, grid[1])).astype(np.int64)
        clean = v.clean_label(t)[ys][:, xs].astype(np.int64)
        clean[clean == 255] = fallback                                     # unlabelled: the lowest class outside the subset, or class 0
        onehot = np.zeros(grid + (num_classes,), dtype=np.float32)
        np.put_along_axis(onehot, clean[..., None], np.float32(margin), axis=2)
        assert np.abs(logits - onehot).max() < margin / 4                  # by construction: the noise bound
        assert np.array_equal(np.argmax(logits, axis=-1), clean)
        on_grid, ylo, xlo = grid_points(v.h, v.w, *grid)
        assert on_grid[0, 0] and on_grid.sum() >= 1
        assert np.array_equal(labels_from_logits(logits, v.h, v.w)[on_grid], clean[ylo][:, xlo][on_grid])


def test_synthetic_source_serves_the_stride_16_grid():
    src = R.SyntheticSource(25, 32, 3, 2)
    assert src.read_logits(4).shape == (3, 5, 19) and src.read_logits(4).tobytes() == src.video.teacher_logits(4, 3, 5).tobytes()
    assert R.SyntheticSource(25, 64, 1, 1).read_logits(0).shape == (5, 9, 19)
    assert R.FrameSource().read_logits(0) is None


# ---------------------------------------------------------------------------------------------------------
# directory sources
# ---------------------------------------------------------------------------------------------------------
def test_directory_source_round_trips_logits_and_names_a_missing_file(tmp_path):
    frames, gt = tmp_path / "25-clip", tmp_path / "gt"
    frames.mkdir(), gt.mkdir()
    rng = np.random.default_rng(0)
    logits = rng.standard_normal((3, 5, 19)).astype(np.float32)
    for i in range(2):
        np.save(frames / ("frame_%06d.npy" % i), np.zeros((32, 64, 3), np.uint8))
        np.save(gt / ("gt_%06d.npy" % i), np.zeros((32, 64), np.uint8))
    np.save(gt / "logits_000000.npy", logits)
    src = R.DirectorySource(str(frames), str(gt), fps=1)
    got = src.read_logits(0)
    assert got.dtype == np.float32 and got.tobytes() == logits.tobytes()
    assert R.source_logits(src, 0).tobytes() == logits.tobytes()
    assert src.read_logits(1) is None                                      # a source without logits stays usable without --soft_teacher
    with pytest.raises(FileNotFoundError, match="logits_000001.npy") as e:
        R.source_logits(src, 1)
    assert "--soft_teacher" in str(e.value) and str(gt) in str(e.value)
    assert R.video_number(str(frames)) == 25 and R.video_number("synthetic:26-x:seconds=3") == 26


# ---------------------------------------------------------------------------------------------------------
# the scheduler's flag rules
# ---------------------------------------------------------------------------------------------------------
BASE = ["--student_checkpoint", "synthetic:0", "--output_dir", "unused", "--mode", "simple"]


def _refused(capsys, argv):
    with pytest.raises(SystemExit) as e:
        R.parse_flags(BASE + argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_the_parser_refuses_what_the_soft_path_cannot_serve(capsys):
    video = ["--input_video", "synthetic:25-synth:seconds=4:fps=1"]
    err = _refused(capsys, video + ["--labels_from_logits"])
    assert "--labels_from_logits needs --soft_teacher" in err
    err = _refused(capsys, video + ["--labels_from_logits", "--device_memory"])
    assert "--labels_from_logits needs --soft_teacher" in err
    err = _refused(capsys, video + ["--soft_teacher"])
    assert "--soft_teacher needs --device_memory" in err and "device-memory capability" in err
    err = _refused(capsys, video + ["--soft_teacher", "--labels_from_logits"])
    assert "--soft_teacher needs --device_memory" in err
    err = _refused(capsys, ["--input_video", "synthetic:26-synth:seconds=4:fps=1", "--soft_teacher", "--device_memory", "--labels_from_logits"])
    assert "COCO" in err and "experiment 26" in err
    # what is served parses, and the flags are off by default
    flags = R.parse_flags(BASE + video + ["--soft_teacher", "--device_memory", "--labels_from_logits"])
    assert flags.soft_teacher and flags.labels_from_logits
    flags = R.parse_flags(BASE + ["--input_video", "synthetic:26-synth:seconds=4:fps=1", "--soft_teacher", "--device_memory"])
    assert flags.soft_teacher and not flags.labels_from_logits              # COCO labels uploaded as before: only the derivation is refused
    flags = R.parse_flags(BASE + video)
    assert not flags.soft_teacher and not flags.labels_from_logits
    assert list(class_indices(25)) == list(CI6)
