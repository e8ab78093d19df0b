"""Time the edge confidence (k_confidence.hip) beside the calls it rides behind, alternating in one process on one GPU, at 512 x 1024.

Medians of --reps after --warmup, p10 / p90 beside them:

  a  one-frame predict_with_metric, host arrays in and out (host clock, stream drained before and after)
  b  one-frame predict_with_confidence: the same results plus the statistics row on the host, the uint8 map left on the device
  c  the launches alone on the logits of a finished pass, at 1 and at 32 frames (HIP events, stream otherwise idle): the confidence kernel
     with its three outputs and teacher labels (through StudentEngine.confidence, which allocates them), the existing head launch (labels
     + confusion matrix + loss) for comparison, and the confidence launch part by part into preallocated buffers: the uint8 map alone,
     the statistics alone without and with teacher labels, the map and the statistics with teacher labels (what the edge loop runs)

    python tools/time_confidence.py [--reps 100] [--warmup 10] [--out profiles/confidence_512x1024.json]
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


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": int(xs.size)}


def time_calls(net, frames, labels, reps, warmup):
    dev = net.engine.device
    ms = {"predict_with_metric": [], "predict_with_confidence": []}
    for k in range(warmup + reps):
        for name in ms:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            getattr(net, name)(frames, labels)
            torch.cuda.synchronize(dev)
            if k >= warmup:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    out = {k + "_ms": stats(v) for k, v in ms.items()}
    out["extra_ms"] = out["predict_with_confidence_ms"]["median"] - out["predict_with_metric_ms"]["median"]
    return out


def time_launches(net, frames, labels, reps, warmup):
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
    n_stats = int(eng.lib.ams_confidence_stats_len())
    u8 = torch.empty((n, eng.height, eng.width), dtype=torch.uint8, device=dev)
    rows = torch.empty((n, n_stats), dtype=torch.int64, device=dev)
    # the parts of the confidence launch: (teacher, map, statistics) given or NULL
    parts = {"confidence_u8_only_no_teacher": (False, True, False), "confidence_stats_only_no_teacher": (False, False, True),
             "confidence_stats_only_teacher": (True, False, True), "confidence_u8_stats_teacher": (True, True, True)}
    us = {"confidence": [], "head": [], **{k: [] for k in parts}}
    for k in range(warmup + reps):
        for name in us:
            torch.cuda.synchronize(dev)
            e0.record(st)
            if name == "confidence":
                eng.confidence(teacher, f32=True, batch=n)
            elif name == "head":
                hip.check(eng.lib.ams_k_upsample_argmax(ptr(eng.logits_lowres), n, h, w, 32, ci, K, eng.height, eng.width, ptr(teacher), ptr(labels_dev),
                                                        ptr(cm), ptr(loss), sp))
            else:
                with_teacher, with_map, with_stats = parts[name]
                hip.check(eng.lib.ams_student_confidence(eng._h, n, ptr(teacher) if with_teacher else None, ptr(u8) if with_map else None, None,
                                                         ptr(rows) if with_stats else None, sp))
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
    ap.add_argument("--out", default="profiles/confidence_512x1024.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_confidence needs the GPU"
    H = a.height
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=3).clip()
    frames, labels = np.ascontiguousarray(frames), np.ascontiguousarray(labels)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True,
                          frozen_graph=FrozenGraph(W0, CI, H, 19), max_batch=32)
    result = {"height": H, "width": 2 * H, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(net.engine.device)}
    result["one_frame_calls"] = time_calls(net, frames[:1], labels[:1], a.reps, a.warmup)
    for n in (1, 32):
        result["launch_%d_frame%s" % (n, "s" if n > 1 else "")] = time_launches(net, np.concatenate([frames] * 8)[:n], np.concatenate([labels] * 8)[:n],
                                                                               a.reps, a.warmup)
    result["note"] = ("*_ms: host clock, stream drained before and after, the two calls alternating; *_us: HIP events around the launch (with its "
                      "memset and, for `confidence`, the allocation of its outputs), stream otherwise idle; the events add a few us of their own")
    net.close_model()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
