"""run.py --edge_from_delta: the edge scores the model the downlink payload produces.  Each event's _delta.bin is the payload the server
counted (its _mask.dat, written under the previous event's label); the edge's confusion matrices equal those of a fresh frozen network
built from the initial model plus that payload, decoded in NumPy."""
import glob
import os

import numpy as np
import pytest

from ams_amd import delta as D, exp_configs, run as R, spec as S, synth, weights as Wt
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
from test_delta_layout_cpu import decode

pytestmark = pytest.mark.gpu

ARGS = ["--input_video", "synthetic:25-synth:seconds=8:fps=8", "--student_checkpoint", "synthetic:0", "--gpu", "0", "--mode", "simple",
        "--height", "256", "--batch_size", "4", "--iter", "3", "--send_period", "1", "--train_period", "2", "--first_train_time", "2",
        "--memory_len", "4", "--sampling", "per_second"]


def _by_second(out, suffix):
    """{second: path} of the files <...>_<second><suffix> (the run label is '0__8_tp2_f1')"""
    found = {}
    for f in glob.glob(out + "*" + suffix):
        tag = os.path.basename(f)[:-len(suffix)]
        found[int(tag.split("0__8_tp2_f1_")[1].split("_")[0])] = f
    return found


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_edge_scores_the_model_the_payload_produces(tmp_path, strategy):
    out = str(tmp_path / "out") + "/"
    summary = R.main(ARGS + ["--output_dir", out, "--train_strategy", strategy, "--edge_from_delta"])
    assert summary["edge_updates"] == 3 and summary["edge_update_ms"] > 0
    deltas = _by_second(out, "_delta.bin")
    masks = _by_second(out, "_mask.dat")
    assert sorted(deltas) == [2, 4, 6] and sorted(masks) == [0, 2, 4]
    for prev, sec in zip([0, 2, 4], [2, 4, 6]):
        assert open(deltas[sec], "rb").read() == open(masks[prev], "rb").read(), sec

    spec = S.build_spec()
    W0 = FrozenGraph.ParseFromString(open(_by_second(out, "_final.pb")[0], "rb").read()).variables
    assert all(np.array_equal(W0[k], v) for k, v in Wt.synthetic_weights(spec, 0).items())
    p0, s0 = Wt.pack_trainable(spec, W0), Wt.pack_stats(spec, W0)
    L = D.delta_layout(spec, strategy)
    cats = np.load(glob.glob(out + "*_results*_mioucats.npy")[0])
    assert cats.shape == (64, 6, 6)
    src = R.SyntheticSource(25, 256, 8, 8)
    cw = exp_configs.class_weights(25)
    ci = list(np.where(cw.reshape(-1) == 1)[0])
    for sec, (f0, f1) in ((0, (0, 16)), (2, (16, 32)), (4, (32, 48)), (6, (48, 64))):
        if sec == 0:
            W = W0
        else:
            p, s = decode(open(deltas[sec], "rb").read(), L, p0, s0)
            W = Wt.unpack(spec, p, s)
        net = SemanticNetwork("unused", class_weights_exp=cw, height=256, frozen=True, frozen_graph=FrozenGraph(W, ci, 256, 19))
        for i in range(f0, f1):
            frame, label = src.read(i)
            _, conf, _, _, _ = net.predict_with_metric(frame[None], label[None])
            assert np.array_equal(conf, cats[i]), (sec, i)
        net.close_model()


def test_without_the_flag_no_delta_is_written(tmp_path):
    out = str(tmp_path / "out") + "/"
    summary = R.main(ARGS + ["--output_dir", out, "--train_strategy", "coord_desc_rand"])
    assert "edge_updates" not in summary
    assert glob.glob(out + "*_delta.bin") == [] and len(glob.glob(out + "*_mask.dat")) == 3
