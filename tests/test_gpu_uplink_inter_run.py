"""run.py --uplink_gop: within one upload, frames after the first may travel predicted from the decoded frame in front of them.  One short
synthetic run at the smallest height the scheduler tests use, as tests/test_gpu_uplink_run.py does it: the frames the loop hands to the lossy
leg are recorded (a wrapper around run._through_uplink) and taken through the NumPy oracles here as one closed-loop chain per upload, with the
budget that passes what a frame saved on to the next.  The replay memory holds the oracle chain's frames, _bw_uplink.npy its bytes,
_uplink_kinds.npy its kinds and zero-length slices.  Without the new flag the run writes what it wrote before."""
import glob

import numpy as np
import pytest

from ams_amd import run as R
from ams_amd.semantic_network import SemanticNetwork
from ams_amd.utils import resize_linear
import uplink_ref as U
import uplink_inter_ref as P
import test_gpu_uplink_run as T

pytestmark = pytest.mark.gpu

H, FPS, SECONDS, BW, GOP = T.H, T.FPS, T.SECONDS, 40.0, 4
UPLOAD = int(BW * 1000 / 8)                    # bytes of one upload: one per second


def oracle_upload(frames, gop=GOP):
    """one upload through the oracle chain -> per frame (the frame the server stores, bytes, q, fits, kind, zero-length slices, slices)"""
    out, spent, prev = [], 0, None
    for k, frame in enumerate(frames):
        big = resize_linear(frame, 4 * H, 2 * H)
        if k % gop == 0:
            prev = None
        budget = (UPLOAD - spent) // (len(frames) - k)
        payload, q, fits, kind = P.encode_to_budget(big, budget, prev)
        prev = P.decode(payload, prev) if kind == P.INTER else U.decode(payload, 2 * H, 4 * H)
        n = P.slice_count(2 * H, 4 * H) if kind == P.INTER else sum(U.slice_counts(2 * H, 4 * H))
        zeros = int((np.frombuffer(payload[16:16 + 2 * n], "<u2") == 0).sum())
        spent += len(payload)
        out.append((resize_linear(prev, 2 * H, H), len(payload), q, fits, kind, zeros, n, budget))
    return out


@pytest.fixture
def recorded(monkeypatch):
    log = {"sent": [], "memories": []}
    inner = R._through_uplink

    def through(fr, codec, budget, size, ingest=None, chain=None):
        res = inner(fr, codec, budget, size, ingest, chain)
        log["sent"].append((np.array(R._host(fr)), budget, np.array(R._host(res[0]))) + tuple(res[1:]))
        return res

    train = SemanticNetwork.train_with_deque

    def train_with_deque(self, frames, labels, *a, **k):
        log["memories"].append([np.array(f) for f in frames])
        return train(self, frames, labels, *a, **k)

    monkeypatch.setattr(R, "_through_uplink", through)
    monkeypatch.setattr(SemanticNetwork, "train_with_deque", train_with_deque)
    return log


def test_server_trains_on_the_oracle_chain(tmp_path, recorded):
    out = str(tmp_path / "out") + "/"
    np.random.seed(3)
    summary = R.main(T.ARGS + ["--output_dir", out, "--compress_uplink", "--uplink_bw", str(BW), "--uplink_gop", str(GOP)])
    assert summary["frames"] == FPS * SECONDS
    sent = recorded["sent"]
    assert len(sent) == FPS * SECONDS
    uploads = [oracle_upload([s[0] for s in sent[i:i + FPS]]) for i in range(0, len(sent), FPS)]
    want = [w for up in uploads for w in up]
    for k, ((src, budget, got, nbytes, q, fits), w) in enumerate(zip(sent, want)):
        assert (budget, nbytes, q, fits) == (w[7], w[1], w[2], w[3]), k
        assert np.array_equal(got, w[0]), k
    kinds = [[w[4] for w in up] for up in uploads]
    assert all(k[0] == P.INTRA for k in kinds) and any(P.INTER in k for k in kinds)          # prediction is used, and never across uploads
    assert all(sum(w[1] for w in up) <= UPLOAD for up in uploads)
    assert np.array_equal(T._result(out, "_bw_uplink.npy"), [sum(w[1] / 1024 for w in up) * 8 for up in uploads])
    rows = [(sec + 1, sum(w[4] == P.INTRA for w in up), sum(w[4] == P.INTER for w in up), sum(w[5] for w in up), sum(w[6] for w in up))
            for sec, up in enumerate(uploads)]
    assert np.array_equal(T._result(out, "_uplink_kinds.npy"), np.asarray(rows, np.float64))
    quality = T._result(out, "_uplink_quality.npy")
    assert quality.shape == (SECONDS, 7) and np.array_equal(quality[:, 2], [sum(w[1] for w in up) for up in uploads])
    assert np.array_equal(quality[:, 4], [min(w[2] for w in up) for up in uploads])
    assert len(recorded["memories"]) == SECONDS - 1
    for k, memory in enumerate(recorded["memories"]):
        upto = [w[0] for w in want[:(k + 1) * FPS]][-T.SLOTS:]
        assert len(memory) == len(upto) and all(np.array_equal(a, b) for a, b in zip(memory, upto)), k


def test_without_the_new_flag_the_run_is_the_intra_run(tmp_path, recorded):
    """--uplink_gop 1 is the default: the intra oracle's bytes and qualities, frame by frame, and no _uplink_kinds.npy"""
    out = str(tmp_path / "out") + "/"
    np.random.seed(3)
    R.main(T.ARGS + ["--output_dir", out, "--compress_uplink", "--uplink_bw", str(T.BW)])
    sent = recorded["sent"]
    assert [s[1] for s in sent] == [T.BUDGET] * len(sent) and glob.glob(out + "*_uplink_kinds.npy") == []
    want = [T.through_oracle(s[0]) for s in sent]
    uploads = [want[i:i + FPS] for i in range(0, len(want), FPS)]
    assert np.array_equal(T._result(out, "_bw_uplink.npy"), [sum(w[1] / 1024 for w in up) * 8 for up in uploads])
    rows = [(sec + 1, FPS, sum(w[1] for w in up), T.BUDGET, min(w[2] for w in up), np.mean([w[2] for w in up]), sum(not w[3] for w in up))
            for sec, up in enumerate(uploads)]
    assert np.array_equal(T._result(out, "_uplink_quality.npy"), np.asarray(rows, np.float64))


def test_the_flag_is_refused_in_words_without_the_codec(capsys):
    with pytest.raises(SystemExit):
        R.parse_flags(T.ARGS + ["--output_dir", "unused", "--uplink_gop", "4"])
    assert "--uplink_gop needs --compress_uplink" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        R.parse_flags(T.ARGS + ["--output_dir", "unused", "--compress_uplink", "--uplink_gop", "0"])
    assert "--uplink_gop" in capsys.readouterr().err
