"""run.py --compress_uplink: every sampled frame reaches the server through the uplink frame codec.  One short synthetic run in simple mode at
the smallest height the scheduler tests use, with and without --gpu_ingest.  The frames the loop hands to the lossy leg are recorded (a
wrapper around run._through_uplink) and taken through the NumPy oracle here: resize to twice the network size, the rate rule at the upload's
budget, decode, resize back.  _bw_uplink.npy counts the oracle's payload bytes, _uplink_quality.npy its qualities, and the replay memory the
fine-tune phases see holds the oracle's frames.  Without the flag the uplink accounting is the parent's zlib stand-in."""
import glob
import zlib

import numpy as np
import pytest

from ams_amd import run as R
from ams_amd.semantic_network import SemanticNetwork
from ams_amd.utils import resize_linear
import uplink_ref as U

pytestmark = pytest.mark.gpu

H, FPS, SECONDS, BW = 64, 4, 3, 100.0
SLOTS = FPS                                    # --memory_len 1 at one upload per second: the memory holds one upload
ARGS = ["--input_video", "synthetic:25-synth:seconds=%d:fps=%d" % (SECONDS, FPS), "--student_checkpoint", "synthetic:0", "--gpu", "0", "--mode", "simple",
        "--height", str(H), "--batch_size", "2", "--iter", "2", "--send_period", "1", "--train_period", "1", "--first_train_time", "1",
        "--memory_len", "1", "--sampling", "per_second"]
BUDGET = int(BW * 1000 / 8 * 1 // FPS)          # one upload per second, FPS frames in it

_oracle = {}


def through_oracle(frame):
    """(the frame the server stores, payload bytes, quality, fits), computed once per source frame"""
    key = frame.tobytes()
    if key not in _oracle:
        big = resize_linear(frame, 4 * H, 2 * H)
        payload, q, fits, _ = U.encode_to_budget(big, BUDGET)
        _oracle[key] = (resize_linear(U.decode(payload, 2 * H, 4 * H), 2 * H, H), len(payload), q, fits)
    return _oracle[key]


def _result(out, suffix):
    found = glob.glob(out + "*_results*" + suffix)
    assert len(found) == 1, (suffix, found)
    return np.load(found[0])


@pytest.fixture
def recorded(monkeypatch):
    """what went into the lossy leg and came out of it; the frame memory as every fine-tune phase found it"""
    log = {"sent": [], "memories": []}
    inner = R._through_uplink

    def through(fr, codec, budget, size, ingest=None):
        res = inner(fr, codec, budget, size, ingest)
        log["sent"].append((np.array(R._host(fr)), budget, np.array(R._host(res[0]))) + tuple(res[1:]))
        return res

    train = SemanticNetwork.train_with_deque

    def train_with_deque(self, frames, labels, *a, **k):
        log["memories"].append([np.array(f) for f in frames])
        return train(self, frames, labels, *a, **k)

    monkeypatch.setattr(R, "_through_uplink", through)
    monkeypatch.setattr(SemanticNetwork, "train_with_deque", train_with_deque)
    return log


@pytest.mark.parametrize("ingest", [False, True], ids=["host_resize", "gpu_ingest"])
def test_server_trains_on_what_the_decoder_gives_back(tmp_path, recorded, ingest):
    out = str(tmp_path / "out") + "/"
    np.random.seed(3)
    summary = R.main(ARGS + ["--output_dir", out, "--compress_uplink", "--uplink_bw", str(BW)] + (["--gpu_ingest"] if ingest else []))
    assert summary["frames"] == FPS * SECONDS
    sent = recorded["sent"]
    assert len(sent) == FPS * SECONDS and [s[1] for s in sent] == [BUDGET] * len(sent)
    want = [through_oracle(s[0]) for s in sent]
    for (src, _, got, nbytes, q, fits), (frame, size, want_q, want_fits) in zip(sent, want):
        assert src.shape == (H, 2 * H, 3) and (nbytes, q, fits) == (size, want_q, want_fits)
        assert np.array_equal(got, frame)
    assert all(w[3] for w in want) and all(1 < w[2] < 100 for w in want)          # the budget binds
    uploads = [want[i:i + FPS] for i in range(0, len(want), FPS)]
    assert np.array_equal(_result(out, "_bw_uplink.npy"), [sum(w[1] / 1024 for w in up) * 8 for up in uploads])
    rows = [(sec + 1, FPS, sum(w[1] for w in up), BUDGET, min(w[2] for w in up), np.mean([w[2] for w in up]), sum(not w[3] for w in up))
            for sec, up in enumerate(uploads)]
    assert np.array_equal(_result(out, "_uplink_quality.npy"), np.asarray(rows, np.float64))
    # the memory of memory_len / send_period * fps frames at each phase (seconds 1 and 2): the newest decoded frames, oldest first
    assert len(recorded["memories"]) == SECONDS - 1
    for k, memory in enumerate(recorded["memories"]):
        upto = [w[0] for w in want[:(k + 1) * FPS]][-SLOTS:]
        assert len(memory) == len(upto) and all(np.array_equal(a, b) for a, b in zip(memory, upto)), k
    assert np.array_equal(_result(out, "_fps_client.npy"), [FPS] * SECONDS)


def test_without_the_flag_the_uplink_accounting_is_unchanged(tmp_path, recorded):
    out = str(tmp_path / "out") + "/"
    np.random.seed(3)
    R.main(ARGS + ["--output_dir", out])
    assert recorded["sent"] == [] and glob.glob(out + "*_uplink_quality.npy") == []
    src = R.SyntheticSource(25, H, SECONDS, FPS)
    frames = [src.read(i)[0] for i in range(FPS * SECONDS)]
    want = [sum(len(zlib.compress(f.tobytes(), 6)) / 1024 for f in frames[i:i + FPS]) * 8 for i in range(0, len(frames), FPS)]
    assert np.array_equal(_result(out, "_bw_uplink.npy"), want)
    last = frames[:(SECONDS - 1) * FPS][-SLOTS:]                 # the last phase runs at second SECONDS - 1
    assert len(recorded["memories"][-1]) == len(last) and all(np.array_equal(a, b) for a, b in zip(recorded["memories"][-1], last))


def test_flag_is_refused_in_words_where_it_cannot_run(capsys):
    with pytest.raises(SystemExit):
        R.parse_flags(ARGS[:10] + ["--height", "60", "--output_dir", "unused", "--compress_uplink"])
    assert "multiple of 8" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        R.parse_flags(ARGS + ["--output_dir", "unused", "--compress_uplink", "--uplink_bw", "0"])
    assert "--uplink_bw" in capsys.readouterr().err
