"""Time the server side of a model update at 512 x 1024, coord_desc_auto with coord_frac 0.1: the host path (the default) against the device
path (SemanticNetwork(device_masks=True), k_select.hip), in one process on one GPU.

Two quantities on the host clock, each the median of --reps events after --warmup:

  select_ms   everything between the end of the phase's first step and the point where the second step can be enqueued: fetch the model,
              np.percentile, masks, roll-back, mask upload (host path) / select_changed (device path).  The stream is drained before the clock
              starts, so the first step is not in it.
  payload_ms  phase end -> payload bytes in host memory: what _train does after its last step (the host path fetches the model for
              train_params there) plus delta_payload().

Beside them, HIP-event times of the device path's kernels alone: ams_select_changed (memset + 8 launches), ams_select_apply,
ams_student_encode_delta (table upload + 3 launches).  Writes one JSON (--out) and prints it.

    python tools/time_server_update.py [--reps 50] [--warmup 5] [--out out/time_server_update.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ams_amd import delta as D, exp_configs, spec as S, synth, weights as Wt  # noqa: E402
from ams_amd.coord_masks import percentile_rank  # noqa: E402
from ams_amd.semantic_network import SemanticNetwork  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]
STRATEGY = "coord_desc_auto"


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90))}


def host_select(net, before):
    """the host path's selection, as in SemanticNetwork._train (it == 0)"""
    after = net._model_vars()
    names = [v.name for v in net.engine.spec.trainable]
    changes = np.concatenate([np.abs(after[k] - before[k]).reshape(-1) for k in names], axis=0)
    cut = np.percentile(changes, 100 * (1 - net.coord_frac))
    mask, combine = {}, {}
    for k in names:
        mask[k] = np.abs(after[k] - before[k]) > cut
        combine[k] = np.where(mask[k], after[k], before[k])
    net._restore_dict(combine)
    return mask, net._mask_to_device(mask)


def host_phase_end(net, mask):
    names = [v.name for v in net.engine.spec.trainable]
    after = net._model_vars()
    net.curr_mask = [np.asarray(mask[k]) for k in names]
    net.train_params = [after[k] for k in names]
    return net.delta_payload()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--frac", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="out/time_server_update.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_server_update needs the GPU"
    spec = S.build_spec()
    W0 = Wt.synthetic_weights(spec, seed=0)
    frames, labels = synth.SyntheticVideo(a.height, a.batch, CI, seed=3).clip()
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=a.height, scale=[1], mini_batch_size=a.batch,
                          lr=1e-3, coord_frac=a.frac, masked_gradients=True, initial_variables=W0, device_masks=True)
    eng = net.engine
    dev = eng.device
    L = D.delta_layout(spec, STRATEGY)
    n = spec.n_trainable
    ones = torch.ones(n, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)
    t = {k: [] for k in ("host_select_ms", "device_select_ms", "host_payload_ms", "device_payload_ms", "select_kernels_us", "apply_kernel_us",
                         "encode_kernels_us")}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    payloads = None
    for r in range(a.warmup + a.reps):
        keep = r >= a.warmup
        # ---- host path
        net.restore_initial()
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.adam_step = 0          # both paths start from the same optimiser state
        before_host = {k: v for k, v in net._model_vars().items() if k in {x.name for x in spec.trainable}}
        eng.train_step(frames, labels, net.lr, ones)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        mask_host, mask_dev_h = host_select(net, before_host)
        torch.cuda.synchronize(dev)                       # the uploads the second step waits for
        t1 = time.perf_counter()
        eng.train_step(frames, labels, net.lr, mask_dev_h)
        torch.cuda.synchronize(dev)
        net.__dict__.pop("_held", None)
        t2 = time.perf_counter()
        payload_h = host_phase_end(net, mask_host)
        t3 = time.perf_counter()
        # ---- device path, from the same weights and batch
        net.restore_initial()
        eng.adam_m.zero_()
        eng.adam_v.zero_()
        eng.adam_step = 0
        before_dev = eng.snapshot_params()
        eng.train_step(frames, labels, net.lr, ones)
        torch.cuda.synchronize(dev)
        t4 = time.perf_counter()
        mask_dev, _kept = eng.select_changed(before_dev, net.coord_frac)
        t5 = time.perf_counter()                          # both kernels are enqueued; the second step can follow on the stream
        eng.train_step(frames, labels, net.lr, mask_dev)
        torch.cuda.synchronize(dev)
        t6 = time.perf_counter()
        net._hold_phase(STRATEGY, mask_dev)
        payload_d = net.delta_payload()
        t7 = time.perf_counter()
        assert payload_d == payload_h, "the two paths disagree"
        # ---- the kernels alone, HIP events
        net.restore_initial()
        before_dev = eng.snapshot_params()
        eng.train_step(frames, labels, net.lr, ones)
        words = eng._select_words
        k = percentile_rank(n, 100 * (1 - net.coord_frac))
        out = torch.empty(L.max_payload_bytes, dtype=torch.uint8, device=dev)
        table = L.table()
        torch.cuda.synchronize(dev)
        ev[0].record(st)
        rc = eng.lib.ams_select_changed(C.c_void_p(eng.params.data_ptr()), C.c_void_p(before_dev.data_ptr()), n, k, C.c_void_p(words.data_ptr()),
                                        C.c_void_p(eng._select_scratch.data_ptr()), eng._select_scratch.numel(), eng._stream())
        ev[1].record(st)
        rc |= eng.lib.ams_select_apply(C.c_void_p(eng.params.data_ptr()), C.c_void_p(before_dev.data_ptr()), n, 1e-4, C.c_void_p(mask_dev.data_ptr()),
                                       C.c_void_p(words.data_ptr() + 16), eng._stream())
        ev[2].record(st)
        rc |= eng.lib.ams_student_encode_delta(eng._h, C.c_void_p(mask_dev.data_ptr()), table, len(table), C.c_void_p(out.data_ptr()), out.numel(),
                                               C.c_void_p(words.data_ptr() + 24), C.c_void_p(eng._encode_scratch.data_ptr()),
                                               eng._encode_scratch.numel(), eng._stream())
        ev[3].record(st)
        torch.cuda.synchronize(dev)
        assert rc == 0, eng.lib.ams_last_error()
        if keep:
            t["host_select_ms"].append((t1 - t0) * 1e3)
            t["host_payload_ms"].append((t3 - t2) * 1e3)
            t["device_select_ms"].append((t5 - t4) * 1e3)
            t["device_payload_ms"].append((t7 - t6) * 1e3)
            t["select_kernels_us"].append(ev[0].elapsed_time(ev[1]) * 1e3)
            t["apply_kernel_us"].append(ev[1].elapsed_time(ev[2]) * 1e3)
            t["encode_kernels_us"].append(ev[2].elapsed_time(ev[3]) * 1e3)
            payloads = len(payload_d)
    result = {"height": a.height, "width": 2 * a.height, "batch": a.batch, "coord_frac": a.frac, "reps": a.reps, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(dev), "n_trainable": n, "payload_bytes": payloads}
    result.update({k: stats(v) for k, v in t.items()})
    result["select_host_over_device"] = result["host_select_ms"]["median"] / result["device_select_ms"]["median"]
    result["payload_host_over_device"] = result["host_payload_ms"]["median"] / result["device_payload_ms"]["median"]
    result["note"] = ("select_ms: first step drained -> second step can be enqueued (host path: incl. the mask upload's completion; device "
                      "path: incl. its one 16-byte read-back); payload_ms: phase end -> payload bytes in host memory; *_us: HIP events "
                      "around the C ABI calls of the device path, stream otherwise idle")
    net.close_model()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
