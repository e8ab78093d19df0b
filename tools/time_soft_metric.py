"""Time the soft-teacher evaluation (k_soft_metric.hip) beside the calls it rides behind, alternating in one process on one GPU, at 512 x 1024,
six classes, 1 and 32 frames.

Medians of --reps after --warmup, p10 / p90 beside them:

  a  predict_with_metric, host frames and labels in, host results out (host clock, stream drained before and after)
  b  predict_with_soft_metric: the same results plus the SoftMetric, with teacher logits at the label size and on a 33 x 65 grid (device
     tensors, as a replay memory holds them)
  c  the launches alone on the logits of a finished pass (HIP events, stream otherwise idle): the existing head launch (labels + confusion
     matrix + loss) for comparison, and the soft-metric launch into preallocated buffers with the statistics alone and with both maps, for
     both teacher grids

    python tools/time_soft_metric.py [--reps 100] [--warmup 10] [--out profiles/soft_metric_512x1024.json]
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

from ams_amd import exp_configs, hip, spec as S, synth, weights as Wt  # noqa: E402
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]
NC = 19


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": int(xs.size)}


def time_calls(net, frames, labels, grids, reps, warmup):
    dev = net.engine.device
    calls = {"predict_with_metric": lambda: net.predict_with_metric(frames, labels)}
    for name, t in grids.items():
        calls["predict_with_soft_metric_" + name] = lambda t=t: net.predict_with_soft_metric(frames, labels, t)
    ms = {k: [] for k in calls}
    for k in range(warmup + reps):
        for name, fn in calls.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            if k >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {k + "_ms": stats(v) for k, v in ms.items()}
    for name in grids:
        out["extra_%s_ms" % name] = out["predict_with_soft_metric_%s_ms" % name]["median"] - out["predict_with_metric_ms"]["median"]
    return out


def time_launches(net, frames, labels, grids, reps, warmup):
    eng = net.engine
    dev = eng.device
    st = torch.cuda.current_stream(dev)
    n = len(frames)
    eng.predict_frames(frames, labels, hip.MODE_FROZEN, u8=True)
    teacher = eng.last_inputs()[1]
    h, w = eng.lowres
    K = len(CI)
    ci = (C.c_int32 * K)(*CI)
    labels_dev = torch.empty((n, eng.height, eng.width), dtype=torch.int32, device=dev)
    cm = torch.empty(K * K, dtype=torch.int64, device=dev)
    loss = torch.empty(2, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sp = C.c_void_p(st.cuda_stream)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rows = torch.empty((n, int(eng.lib.ams_soft_metric_stats_len(K))), dtype=torch.int64, device=dev)
    p = torch.empty((n, eng.height, eng.width, K), dtype=torch.float32, device=dev)
    ce = torch.empty((n, eng.height, eng.width), dtype=torch.float32, device=dev)
    us = {"head": []}
    for name in grids:
        us["soft_metric_stats_only_" + name] = []
        us["soft_metric_stats_and_maps_" + name] = []
    for k in range(warmup + reps):
        for name in us:
            torch.cuda.synchronize(dev)
            e0.record(st)
            if name == "head":
                hip.check(eng.lib.ams_k_upsample_argmax(ptr(eng.logits_lowres), n, h, w, 32, ci, K, eng.height, eng.width, ptr(teacher), ptr(labels_dev),
                                                        ptr(cm), ptr(loss), sp))
            else:
                t = grids[name.rsplit("_", 1)[1]]
                maps = "_maps_" in name
                hip.check(eng.lib.ams_student_soft_metric(eng._h, n, ptr(teacher), ptr(t), int(t.shape[1]), int(t.shape[2]), ptr(rows),
                                                          ptr(p) if maps else None, ptr(ce) if maps else None, sp))
            e1.record(st)
            torch.cuda.synchronize(dev)
            if k >= warmup:
                us[name].append(e0.elapsed_time(e1) * 1e3)
    return {k + "_us": stats(v) for k, v in us.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="profiles/soft_metric_512x1024.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_soft_metric needs the GPU"
    H = a.height
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=3).clip()
    frames, labels = np.ascontiguousarray(frames), np.ascontiguousarray(labels)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True,
                          frozen_graph=FrozenGraph(W0, CI, H, 19), max_batch=32)
    dev = net.engine.device
    result = {"height": H, "width": 2 * H, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev)}
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (1, 32):
        f, l = np.concatenate([frames] * 8)[:n], np.concatenate([labels] * 8)[:n]
        grids = {"full": torch.randn((n, H, 2 * H, NC), generator=gen, device=dev) * 3, "33x65": torch.randn((n, 33, 65, NC), generator=gen, device=dev) * 3}
        key = "%d_frame%s" % (n, "s" if n > 1 else "")
        result["calls_" + key] = time_calls(net, f, l, grids, a.reps, a.warmup)
        result["launch_" + key] = time_launches(net, f, l, grids, a.reps, a.warmup)
        del grids
    result["note"] = ("*_ms: host clock, stream drained before and after, the calls alternating; *_us: HIP events around the launch (with its "
                      "memset), stream otherwise idle; the events add a few us of their own")
    net.close_model()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
