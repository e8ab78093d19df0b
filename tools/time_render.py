"""Time the picture path on the host (the NumPy helpers of SemanticNetwork: colorize, colorize_teacher, cross_ignore) against the same
pictures painted on the device (ams_amd/render.py, k_render.hip), alternating in one process on one GPU.

Medians of --reps after --warmup, p10 / p90 beside them, at 512 x 1024:

  a  the six views of one frame from device-resident inputs: the host helpers, including the copy of the labels and the frame they need,
     (host clock, stream drained before and after) against the render launch alone (HIP events, stream otherwise idle)
  b  predict_with_metric + host painting against predict_rendered, at 1 and 4 frames per pass (host clock; the views stay on the device)
  c  the same with the views brought back to the host (RenderedViews.host(): one copy)

The baseline of every ratio is the host path timed in the same run.  Writes one JSON (--out) and prints it.

    python tools/time_render.py [--cases a,b,c] [--reps 50] [--warmup 5] [--out profiles/render_512x1024.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ams_amd import exp_configs, render, spec as S, synth, weights as Wt  # noqa: E402
from ams_amd.semantic_network import FrozenGraph, SemanticNetwork  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": int(xs.size)}


def host_paint(net, frame, student, teacher):
    """the six views of one frame through the host helpers (teacher ids the take table does not cover are ignored, as run.py paints them)"""
    known = teacher < net.TOTAL_CLASSES
    cross, ignore = net.cross_ignore(label_teacher=np.where(known, teacher, 0), label_student=student)
    ignore[~known] = 255
    cross[~known] = 0
    return (cross, ignore) + tuple(net.colorize_teacher(label=teacher, frame=frame)) + tuple(net.colorize(label=student, frame=frame))


def time_views(net, frame_dev, student_dev, teacher_dev, reps, warmup):
    dev = net.engine.device
    st = torch.cuda.current_stream(dev)
    r = net._get_renderer()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host_ms, launch_us = [], []
    for k in range(warmup + reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        host_paint(net, frame_dev[0].cpu().numpy(), student_dev[0].cpu().numpy(), teacher_dev[0].cpu().numpy())
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize(dev)
        e0.record(st)
        r.render(frame_dev, student_dev, teacher_dev)
        e1.record(st)
        torch.cuda.synchronize(dev)
        if k >= warmup:
            host_ms.append(ms)
            launch_us.append(e0.elapsed_time(e1) * 1e3)
    out = {"host_helpers_ms": stats(host_ms), "render_launch_us": stats(launch_us)}
    out["host_over_device"] = out["host_helpers_ms"]["median"] * 1e3 / out["render_launch_us"]["median"]
    return out


def time_calls(net, frames, labels, reps, warmup, to_host):
    dev = net.engine.device
    host_ms, dev_ms = [], []
    for k in range(warmup + reps):
        for path in ("host", "device"):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if path == "host":
                res = net.predict_with_metric(frames, labels)
                for j in range(len(frames)):
                    host_paint(net, frames[j], res[0][j], labels[j])
            else:
                res = net.predict_rendered(frames, labels)
                if to_host:
                    res[5].host()
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3
            if k >= warmup:
                (host_ms if path == "host" else dev_ms).append(ms)
    out = {"host_ms": stats(host_ms), "device_ms": stats(dev_ms)}
    out["host_over_device"] = out["host_ms"]["median"] / out["device_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--out", default="profiles/render_512x1024.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_render needs the GPU"
    cases = a.cases.split(",")
    H = a.height
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, 4, CI, seed=3).clip()
    frames, labels = np.ascontiguousarray(frames), np.ascontiguousarray(labels)
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, frozen=True,
                          frozen_graph=FrozenGraph(W0, CI, H, 19), max_batch=4)
    dev = net.engine.device
    result = {"height": H, "width": 2 * H, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(dev),
              "views": list(render.VIEWS), "bytes_per_frame_six_views": H * 2 * H * (3 + 1 + 1 + 6 * 3)}
    if "a" in cases:
        student = torch.from_numpy(net.predict_input(frames[:1]).astype(np.uint8)).to(dev)
        result["a_six_views_one_frame"] = time_views(net, torch.from_numpy(frames[:1]).to(dev), student, torch.from_numpy(labels[:1]).to(dev),
                                                     a.reps, a.warmup)
    for case, to_host in (("b", False), ("c", True)):
        if case in cases:
            for n in (1, 4):
                result["%s_%d_frame%s%s" % (case, n, "s" if n > 1 else "", "_views_to_host" if to_host else "")] = \
                    time_calls(net, frames[:n], labels[:n], a.reps, a.warmup, to_host)
    result["note"] = ("*_ms: host clock, stream drained before and after, host path and device path alternating; render_launch_us: HIP events "
                      "around the one launch, stream otherwise idle; host_helpers_ms includes the device -> host copy of frame and labels")
    net.close_model()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
