"""run.py --delta_format q8 with --edge_from_delta: the downlink carries int8 codes of the change, the edge decodes them on the device.  Each
event's _delta.bin is the payload the server counted (its _mask.dat, written under the previous event's label) and has the q8 size; the
edge's confusion matrices equal those of a fresh frozen network built from the NumPy oracle's decode of that payload — onto the initial
model, or under --no_restore onto the previous decode; _bw_downlink.npy is 8 x the gzipped size of those bytes."""
import glob
import gzip
import os

import numpy as np
import pytest

from ams_amd import delta as D, exp_configs, run as R, spec as S, weights as Wt
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
import delta_q8_ref as Q
from test_gpu_edge_delta_run import ARGS, _by_second

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("strategy,no_restore", [("coord_desc_rand", False), ("full_model", False), ("coord_desc_rand", True)])
def test_edge_scores_the_model_the_q8_payload_produces(tmp_path, strategy, no_restore):
    out = str(tmp_path / "out") + "/"
    summary = R.main(ARGS + ["--output_dir", out, "--train_strategy", strategy, "--edge_from_delta", "--delta_format", "q8"]
                     + (["--no_restore"] if no_restore else []))
    assert summary["edge_updates"] == 3 and summary["edge_update_ms"] > 0 and summary["delta_format"] == "q8"
    deltas = _by_second(out, "_delta.bin")
    masks = _by_second(out, "_mask.dat")
    zipped = _by_second(out, "_mask.dat.gz")
    assert sorted(deltas) == [2, 4, 6] and sorted(masks) == [0, 2, 4] == sorted(zipped)
    spec = S.build_spec()
    L = D.delta_layout(spec, strategy)
    for prev, sec in zip([0, 2, 4], [2, 4, 6]):
        payload = open(deltas[sec], "rb").read()
        assert payload == open(masks[prev], "rb").read() == gzip.open(zipped[prev], "rb").read(), sec
        bits = np.unpackbits(np.frombuffer(payload, np.uint8)[:L.mask_bytes])
        assert len(payload) == L.mask_bytes + 4 * len(L.entries) + int(bits.sum()), sec
    bw = np.load(glob.glob(out + "*_results*_bw_downlink.npy")[0])
    assert [int(b) for b in bw] == [8 * os.path.getsize(zipped[s]) for s in (0, 2, 4)]

    W0 = FrozenGraph.ParseFromString(open(_by_second(out, "_final.pb")[0], "rb").read()).variables
    assert all(np.array_equal(W0[k], v) for k, v in Wt.synthetic_weights(spec, 0).items())
    p, s = Wt.pack_trainable(spec, W0), Wt.pack_stats(spec, W0)
    cats = np.load(glob.glob(out + "*_results*_mioucats.npy")[0])
    assert cats.shape == (64, 6, 6)
    src = R.SyntheticSource(25, 256, 8, 8)
    cw = exp_configs.class_weights(25)
    ci = list(np.where(cw.reshape(-1) == 1)[0])
    for sec, (f0, f1) in ((0, (0, 16)), (2, (16, 32)), (4, (32, 48)), (6, (48, 64))):
        if sec == 0:
            W = W0
        else:
            base = (p, s) if no_restore else (Wt.pack_trainable(spec, W0), Wt.pack_stats(spec, W0))          # chained / from the initial model
            p, s = Q.decode_q8(open(deltas[sec], "rb").read(), L, *base)
            W = Wt.unpack(spec, p, s)
        net = SemanticNetwork("unused", class_weights_exp=cw, height=256, frozen=True, frozen_graph=FrozenGraph(W, ci, 256, 19))
        for i in range(f0, f1):
            frame, label = src.read(i)
            _, conf, _, _, _ = net.predict_with_metric(frame[None], label[None])
            assert np.array_equal(conf, cats[i]), (sec, i)
        net.close_model()


def test_without_the_flag_the_format_is_fp16(tmp_path):
    out = str(tmp_path / "out") + "/"
    summary = R.main(ARGS + ["--output_dir", out, "--train_strategy", "coord_desc_rand", "--edge_from_delta"])
    assert summary["delta_format"] == "fp16"
    spec = S.build_spec()
    L = D.delta_layout(spec, "coord_desc_rand")
    for f in glob.glob(out + "*_delta.bin"):
        payload = open(f, "rb").read()
        bits = np.unpackbits(np.frombuffer(payload, np.uint8)[:L.mask_bytes])
        assert len(payload) == L.mask_bytes + 2 * int(bits.sum())
