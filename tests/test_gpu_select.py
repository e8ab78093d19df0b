"""Server-side model updates on the device (k_select.hip; StudentEngine.select_changed / encode_delta; SemanticNetwork(device_masks=True);
run.py --device_masks).  Every comparison is bit for bit: the device path has to produce the masks, parameters and payload bytes of the
host path, which stays the default.

  4. the selection and apply kernels, through the C ABI, against the NumPy formulas of the host path;
  5. the encode against the reference's writer and the host delta_payload, and its round trip through the edge's decoder;
  6. two networks from the same weights and seeds, one with device_masks=True: same masks, parameters, losses, variables, payload;
  7. run.py with and without --device_masks: same files and numbers;
  8. a device_masks phase that never reads curr_mask / train_params copies no model to the host.

6 and 7 rely on the fine-tune step being run-to-run identical, as tests/test_gpu_soft_teacher.py does.
"""
import ctypes as C
import glob
import os
import random
from collections import deque

import numpy as np
import pytest
import torch

from ams_amd import coord_masks, delta as D, exp_configs, hip, run as R, spec as S, synth, weights as Wt
from ams_amd.coord_masks import percentile_cut, percentile_rank
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork
from test_delta_layout_cpu import encode, layout_vars
from test_gpu_delta import masks_for, server_values
from test_select_cpu import change_cases, host_formulas, order_statistics, same_bits

pytestmark = pytest.mark.gpu

CI = [0, 1, 2, 10, 11, 13]
SPEC = S.build_spec()
CW = exp_configs.class_weights(25)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def W0():
    return Wt.synthetic_weights(SPEC, seed=0)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- 4. kernels through the C ABI ----------------------------------------------------------------------------------------------------------------
def _select_on_device(lib, after, before, k, cut_of, offset):
    """-> (a, b, nan_count, mask, params, kept); offset: every array is a view one element into its buffer"""
    n = after.size
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def up(x):
        buf = torch.zeros(n + offset, dtype=torch.float32, device=DEV)
        buf[offset:].copy_(torch.from_numpy(x))
        return buf[offset:]

    a_dev, b_dev = up(after), up(before)
    mask = torch.full((n + offset + 8,), 7, dtype=torch.uint8, device=DEV)
    result = torch.zeros(2, dtype=torch.int64, device=DEV)
    kept = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    scratch = torch.empty(int(lib.ams_select_changed_scratch(n)), dtype=torch.int64, device=DEV)
    hip.check(lib.ams_select_changed(_ptr(a_dev), _ptr(b_dev), n, k, _ptr(result), _ptr(scratch), scratch.numel(), stream), "ams_select_changed")
    w = result.cpu().numpy()
    a, b = w[:1].view(np.float32)
    cut = cut_of(a, b, int(w[1]))
    hip.check(lib.ams_select_apply(_ptr(a_dev), _ptr(b_dev), n, float(cut), _ptr(mask[offset:]), _ptr(kept), stream), "ams_select_apply")
    m = mask.cpu().numpy()
    assert (m[:offset] == 7).all() and (m[offset + n:] == 7).all(), "mask written outside its n entries"
    assert np.array_equal(b_dev.cpu().numpy().view(np.uint32), before.view(np.uint32)), "before was written"
    return a, b, int(w[1]), m[offset:offset + n], a_dev.cpu().numpy(), int(kept.item())


def _pairs(n):
    """name -> (after, before): the changes of test_select_cpu.change_cases plus after == before and a change of +inf"""
    rng = np.random.default_rng(n)
    out = {}
    for name, x in change_cases(n).items():
        before = (rng.integers(-2048, 2048, n) / 1024).astype(np.float32)
        out[name] = (before + x, before)
    before = rng.standard_normal(n).astype(np.float32)
    out["unchanged"] = (before.copy(), before)
    after = (before + (rng.standard_normal(n) * 1e-3).astype(np.float32)).astype(np.float32)
    after[n // 3] = np.float32(np.inf)
    out["inf_change"] = (after, before)
    return out


@pytest.mark.parametrize("n", (1, 63, 64, 65, 4097, 2113043))
def test_selection_and_apply_equal_the_host_formulas(n):
    lib = hip.lib()
    for name, (after, before) in _pairs(n).items():
        with np.errstate(invalid="ignore"):
            changes = np.abs(after - before)
        for f in (0.1, 0.37) if n > 100000 else (0.1, 0.05, 0.2, 0.01, 0.37):
            q = 100 * (1 - f)
            k = percentile_rank(n, q)
            wa, wb, wn = order_statistics(changes, k)
            wcut, wm, wp, wk = host_formulas(after, before, q)
            runs = []
            for offset in (0, 1, 0):
                a, b, nans, mask, params, kept = _select_on_device(lib, after, before, k, lambda a, b, c: percentile_cut(a, b, n, q, c), offset)
                where = (name, n, f, offset)
                assert nans == wn, where
                assert (same_bits(a, wa) or np.isnan(wa)) and (same_bits(b, wb) or np.isnan(wb)), where + (a, wa, b, wb)
                assert set(np.unique(mask)) <= {0, 1} and np.array_equal(mask.astype(bool), wm), where
                assert np.array_equal(params.view(np.uint32), wp.view(np.uint32)), where
                assert kept == wk, where
                runs.append((np.float32(a).tobytes(), np.float32(b).tobytes(), mask.tobytes(), params.tobytes()))
            assert runs[0] == runs[2], "two runs differ"


def test_a_nan_cut_keeps_nothing():
    lib = hip.lib()
    n = 4097
    after, before = _pairs(n)["random"]
    _, _, _, mask, params, kept = _select_on_device(lib, after, before, 5, lambda a, b, c: np.float32(np.nan), 0)
    assert kept == 0 and not mask.any() and np.array_equal(params.view(np.uint32), before.view(np.uint32))


# ---- 5. encode -----------------------------------------------------------------------------------------------------------------------------------
def _server(W0, H=32, **kw):
    return SemanticNetwork("unused", class_weights_exp=CW, height=H, scale=[1], mini_batch_size=2, lr=1e-3, coord_frac=kw.pop("coord_frac", 0.1),
                           initial_variables=W0, **kw)


def _frozen(W, H=32):
    return SemanticNetwork("unused", class_weights_exp=CW, height=H, frozen=True, frozen_graph=FrozenGraph(W, CI, H, 19))


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_encode_equals_the_reference_writer_and_the_host_payload(strategy, W0):
    rng = np.random.default_rng(5)
    L = D.delta_layout(SPEC, strategy)
    odd = next(i for i, e in enumerate(L.entries) if e.count % 8)
    net = _server(W0)                                               # host path: its delta_payload is the loop the encode replaces
    eng = net.engine
    sp, ss = server_values(L, rng)
    eng.params.copy_(torch.from_numpy(sp))
    eng.stats.copy_(torch.from_numpy(ss))
    vals = layout_vars(SPEC, L, sp, ss)
    for density in ("zero", "one", "tenth", "all"):
        masks = masks_for(L, density, rng)
        if density != "zero":
            for m in masks[:2]:
                m[:12] = True                                       # the fp16 edge values are always sent
            masks[odd][-1] = True                                   # ... and the last element of a variable of 8 j + r elements
        with np.errstate(over="ignore"):
            want = encode(vals, masks)
        net.curr_mask = [m.reshape(np.shape(W0[e.name])) for m, e in zip(masks, L.entries)]
        net.train_params = [v.reshape(np.shape(W0[e.name])) for v, e in zip(vals, L.entries)]
        with np.errstate(over="ignore"):
            assert net.delta_payload() == want
        flat = torch.from_numpy(np.concatenate(masks).astype(np.uint8)).to(eng.device)
        got = eng.encode_delta(L, flat)
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want, (strategy, density)
        assert eng.encode_delta(L, flat).cpu().numpy().tobytes() == want                  # a second run is identical
        if density == "all":
            assert eng.encode_delta(L, None).cpu().numpy().tobytes() == want              # NULL = every bit set
        # a buffer that is too small: an error, and not one byte written
        for cap in [L.mask_bytes - 1] + ([len(want) - 1] if len(want) > L.mask_bytes else []):
            with pytest.raises(hip.AmsHipError):
                eng.encode_delta(L, flat, cap=cap)
        if len(want) > L.mask_bytes:
            cap = len(want) - 2
            table = L.table()
            out = torch.full((len(want) + 64,), 0xAB, dtype=torch.uint8, device=eng.device)
            size = torch.zeros(1, dtype=torch.int64, device=eng.device)
            scratch = torch.empty(int(eng.lib.ams_student_encode_delta_scratch(table, len(table))), dtype=torch.int64, device=eng.device)
            hip.check(eng.lib.ams_student_encode_delta(eng._h, _ptr(flat), table, len(table), _ptr(out), cap, _ptr(size), _ptr(scratch),
                                                       scratch.numel(), eng._stream()), "ams_student_encode_delta")
            assert int(size.item()) == len(want) > cap
            assert (out.cpu().numpy() == 0xAB).all(), "bytes written although the payload does not fit"
    net.close_model()


@pytest.mark.parametrize("strategy", ["coord_desc_rand", "full_model"])
def test_device_payload_round_trips_through_the_edge(strategy, W0):
    H = 32
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=2).clip()
    server = _server(W0, device_masks=True, masked_gradients=strategy != "full_model")
    np.random.seed(3)
    random.seed(3)
    server.train_with_deque(deque(frames), deque(labels), 2, strategy)
    dev = server.delta_payload(device=True)
    host = server.delta_payload()
    assert isinstance(dev, torch.Tensor) and dev.dtype == torch.uint8 and dev.cpu().numpy().tobytes() == host
    with np.errstate(over="ignore"):
        assert host == encode(server.train_params, server.curr_mask)
    server.close_model()
    edges = [_frozen(W0), _frozen(W0)]
    assert edges[0].apply_delta(dev, strategy) == edges[1].apply_delta(host, strategy) > 0
    a, b = edges[0].engine.get_variables(), edges[1].engine.get_variables()
    for name in SPEC.all_variable_names():
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), name
    for e in edges:
        e.close_model()


# ---- 6. network level ----------------------------------------------------------------------------------------------------------------------------
def _same_list(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8) if x.dtype == bool else x.view(np.uint32), y.view(np.uint8) if y.dtype == bool else y.view(np.uint32))


def _compare_phase(host, dev, strategy):
    assert host.last_losses == dev.last_losses or np.array_equal(np.asarray(host.last_losses), np.asarray(dev.last_losses), equal_nan=True)
    assert host.delta_payload() == dev.delta_payload()
    _same_list(host.curr_mask, dev.curr_mask)
    _same_list(host.train_params, dev.train_params)
    if host.mask is None:
        assert dev.mask is None
    else:
        assert list(host.mask) == list(dev.mask)
        _same_list([np.asarray(v) for v in host.mask.values()], list(dev.mask.values()))
    hv, dv = host.get_vars(), dev.get_vars()
    assert list(hv) == list(dv)
    for k in hv:
        assert np.asarray(hv[k]).tobytes() == np.asarray(dv[k]).tobytes(), k
    assert host.engine.adam_step == dev.engine.adam_step


def _two_phases(W0, H, frac, strategy, monkeypatch=None):
    frames, labels = synth.SyntheticVideo(H, 6, CI, seed=H).clip()
    nets = [_server(W0, H, coord_frac=frac, masked_gradients=strategy != "full_model", device_masks=on) for on in (False, True)]
    for keep in (False, True):
        if monkeypatch is not None:
            # _train draws a table / Bernoulli mask from the global NumPy generator while the sampler thread is already drawing batches from
            # it, on either path: which of the two comes first is a race.  The phase's mask is therefore drawn here, by the same function,
            # before any thread runs, and handed to both networks; the generator then feeds the sampler alone.
            np.random.seed(99 + keep)
            drawn = coord_masks.build_mask(strategy, frac, {v.name: v.shape for v in SPEC.trainable})
            monkeypatch.setattr(coord_masks, "build_mask", lambda *a, _m=drawn: {k: v.copy() for k, v in _m.items()})
        for net in nets:
            np.random.seed(17 + keep)
            random.seed(17 + keep)
            net.train_with_deque(deque(frames), deque(labels), 3, strategy, keep_mask=keep)
        if monkeypatch is not None:
            monkeypatch.undo()
        _compare_phase(nets[0], nets[1], strategy)
    return nets


@pytest.mark.parametrize("H", (32, 64))
@pytest.mark.parametrize("frac", (0.1, 0.01))
def test_coord_desc_auto_on_the_device_equals_the_host_path(H, frac, W0):
    nets = _two_phases(W0, H, frac, "coord_desc_auto")
    kept = sum(int(m.sum()) for m in nets[1].curr_mask)
    assert 0 < kept <= SPEC.n_trainable * frac * 1.5 + 1
    for net in nets:
        net.close_model()


@pytest.mark.parametrize("strategy", ("coord_desc_rand", "coord_desc_last", "full_model"))
@pytest.mark.parametrize("H,frac", ((32, 0.1), (64, 0.01)))
def test_other_strategies_with_device_held_masks_equal_the_host_path(strategy, H, frac, W0, monkeypatch):
    nets = _two_phases(W0, H, frac, strategy, monkeypatch if strategy != "full_model" else None)
    assert len(nets[1].curr_mask) == (272 if strategy == "full_model" else 164)
    for net in nets:
        net.close_model()


# ---- 7. scheduler level --------------------------------------------------------------------------------------------------------------------------
ARGS = ["--input_video", "synthetic:25-synth:seconds=8:fps=8", "--student_checkpoint", "synthetic:0", "--gpu", "0", "--mode", "simple",
        "--height", "64", "--batch_size", "4", "--iter", "3", "--send_period", "1", "--train_period", "2", "--first_train_time", "2",
        "--memory_len", "4", "--sampling", "per_second", "--train_strategy", "coord_desc_auto", "--edge_from_delta"]


def test_run_with_device_masks_writes_the_same_files(tmp_path, capsys):
    outs, summaries, logs = [], [], []
    for flag in ([], ["--device_masks"]):
        out = str(tmp_path / ("dev" if flag else "host")) + "/"
        np.random.seed(5)
        random.seed(5)
        summaries.append(R.main(ARGS + ["--output_dir", out] + flag))
        outs.append(out)
        text = capsys.readouterr().out
        logs.append([l.replace(out, "") for l in text.splitlines() if " took " not in l and "ms each" not in l and "Done!!!" not in l])
    assert logs[0] == logs[1]                                        # every logged number, timings aside
    names = [sorted(os.path.basename(f) for f in glob.glob(o + "*")) for o in outs]
    assert names[0] == names[1] and sum(n.endswith("_mask.dat") for n in names[0]) == 3 and sum(n.endswith("_delta.bin") for n in names[0]) == 3
    for name in names[0]:
        a, b = open(outs[0] + name, "rb").read(), open(outs[1] + name, "rb").read()
        if name.endswith(("_mask.dat", "_delta.bin", "_update.txt")):
            assert a == b, name
        elif name.endswith(".npy") and "_train_ms" not in name:
            assert np.array_equal(np.load(outs[0] + name), np.load(outs[1] + name), equal_nan=True), name
        elif name.endswith(".pb"):
            va, vb = FrozenGraph.ParseFromString(a).variables, FrozenGraph.ParseFromString(b).variables
            assert all(np.array_equal(va[k].view(np.uint32), vb[k].view(np.uint32)) for k in va), name
    for key in ("frames", "mean_miou", "edge_updates"):
        assert summaries[0][key] == summaries[1][key], key


# ---- 8. no model copy to the host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ("coord_desc_auto", "coord_desc_rand", "full_model"))
def test_a_device_phase_copies_no_model_to_the_host(strategy, W0, monkeypatch):
    H = 32
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=9).clip()
    for on in (True, False):
        net = _server(W0, H, device_masks=on, masked_gradients=strategy != "full_model")
        calls = {"get_variables": 0, "params.cpu": 0}
        eng = net.engine
        real_get, real_cpu = eng.get_variables, torch.Tensor.cpu

        def counted_get():
            calls["get_variables"] += 1
            return real_get()

        def counted_cpu(t, *a, **kw):
            if t.dtype == torch.float32 and t.numel() >= SPEC.n_stats:      # params, stats, Adam moments or a copy of them
                calls["params.cpu"] += 1
            return real_cpu(t, *a, **kw)

        eng.get_variables = counted_get
        monkeypatch.setattr(torch.Tensor, "cpu", counted_cpu)
        np.random.seed(1)
        random.seed(1)
        net.train_with_deque(deque(frames), deque(labels), 3, strategy)
        payload = net.delta_payload()
        monkeypatch.undo()
        if on:
            assert calls == {"get_variables": 0, "params.cpu": 0}, calls
            masks = net.curr_mask                                        # the first read materialises them
            assert len(payload) == D.delta_layout(SPEC, strategy).mask_bytes + 2 * sum(int(m.sum()) for m in masks)
        else:
            assert calls["get_variables"] >= 1 and calls["params.cpu"] >= 1   # the wrappers do see the host path's copies
        net.close_model()
