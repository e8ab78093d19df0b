"""Time a training phase fed from the host replay memory (two deques, sampler and stager threads, pinned staging: the default) against the
same phase fed from a DeviceReplayMemory (ams_amd/replay.py, k_replay.hip), alternating in one process on one GPU.

Host clock around ``train_with_deque`` (which ends with the read-back of the losses, so the stream is drained), medians of --reps phases after
--warmup, p10 / p90 beside them, at 512 x 1024, batch 8, 20 iterations:

  a  hard labels, scale [1]                       (what run.py runs)
  b  soft_teacher with teacher logits at the label size
  c  scale [1, 1.25, 1.5]                         (the host path falls to utils.mini_batch)
  d  soft_teacher, logits at the frame size, scale [1, 1.25, 1.5], flip   (device path only: the host path refuses the combination)
  e  case d on a memory that caches every class against one that caches the six selected (logits_select), alternating
  f  case d on a memory with logits at the frame size against one with a 33 x 65 cache and logits_upsample, alternating
  g  one append of a frame with a 33 x 65 x 19 grid: the label derived on the device (append(frame, None, logits)) against the label map
     uploaded from the host (512 KB), alternating

Both paths start every phase from the same seeds, so they train on the same draws.  The baseline of every ratio is the host path timed in
the same run.  Case d has no host path to compare against and no threshold: its phase time is recorded next to HIP-event times of the logits
gather alone (ams_replay_gather_logits, one launch per mini-batch).  Beside them: HIP-event times of the gather launch alone (copy case, bilinear case; stream otherwise idle), and the ASR event
with 10 label pairs as the loop over calc_cross_miou against one cross_miou_pairs call (host clock).  Case e compares the two logit layouts of
the same build in the same run, never a number of an earlier run: the phase (host clock), the logits gather alone (HIP events, equal
descriptors) and one ``append`` of a frame whose logits are a device tensor (HIP events: the copy against the pack kernel) or a NumPy
array (host clock, synchronised: 19 against 6 channels uploaded).  Case f likewise compares two memories of the same build in the same run:
the frame-size cache (ams_replay_gather_logits) against the low-resolution one (ams_replay_gather_logits_lowres), equal seeds and descriptors,
the phase on the host clock, the logits gather alone in HIP events, ``nbytes`` of both.  Case g times one ``append`` of host arrays into a
memory as run.py --soft_teacher builds it (33 x 65 cache, logits_upsample, the six selected channels): HIP events around the append alone,
the form with a host label map (what the parent of this case offers: 512 KB of labels and 6 channels of logits uploaded) against label=None
(19 channels uploaded, ams_teacher_labels_from_logits, the pack kernel), alternating; beside it the label kernel alone on device logits.
Writes one JSON (--out) and prints it.
Cases b and c are slow on the host path (seconds per phase): --reps_b / --reps_c set their own counts, recorded in the JSON.

    python tools/time_replay.py [--cases a,b,c,d,e,f,g,gather,asr] [--reps 50] [--warmup 5] [--out out/time_replay.json]
"""
import argparse
import json
import os
import random
import sys
import time
from collections import deque

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ams_amd import exp_configs, spec as S, synth, weights as Wt  # noqa: E402
from ams_amd.replay import DeviceReplayMemory, draw_samples  # noqa: E402
from ams_amd.semantic_network import SemanticNetwork  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": int(xs.size)}


def seed(k):
    np.random.seed(k)
    random.seed(k)


def time_phases(net, host_args, mem, iters, reps, warmup):
    """host path and device path alternate; returns their per-phase wall times in ms"""
    dev = net.engine.device
    host_ms, dev_ms = [], []
    for r in range(warmup + reps):
        for path in ("host", "device"):
            seed(100 + r)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            if path == "host":
                net.train_with_deque(host_args[0], host_args[1], iters, "full_model", teacher_logits_deque=host_args[2])
            else:
                net.train_with_deque(mem, None, iters, "full_model")
            torch.cuda.synchronize(dev)
            ms = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                (host_ms if path == "host" else dev_ms).append(ms)
    out = {"host_ms": stats(host_ms), "device_ms": stats(dev_ms)}
    out["host_over_device"] = out["host_ms"]["median"] / out["device_ms"]["median"]
    return out


def time_gather(mem, H, scale, batch, reps, warmup):
    dev = mem.device
    st = torch.cuda.current_stream(dev)
    seed(7)
    plan = mem.plan(draw_samples(len(mem), (mem.src_h, mem.src_w), [H, 2 * H], scale, batch, warmup + reps), H, 2 * H)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = []
    for r in range(warmup + reps):
        torch.cuda.synchronize(dev)
        e0.record(st)
        plan.batch(r)
        e1.record(st)
        torch.cuda.synchronize(dev)
        if r >= warmup:
            us.append(e0.elapsed_time(e1) * 1e3)
    return stats(us)


def alternating_phases(net, mems, iters, reps, warmup):
    """``mems`` = {name: memory}: within every repetition one device-path phase from each in turn, equal seeds; per-phase wall times in ms
    by name"""
    dev = net.engine.device
    ms = {k: [] for k in mems}
    for r in range(warmup + reps):
        for k, mem in mems.items():
            seed(100 + r)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            net.train_with_deque(mem, None, iters, "full_model")
            torch.cuda.synchronize(dev)
            if r >= warmup:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return ms


def alternating_logits_gathers(mems, H, scale, flip, batch, reps, warmup):
    """``mems`` = {name: memory} of equal frame size: HIP events around the logits gather of a mini-batch alone (the frames' gather is not in
    the window), equal descriptors, the memories in turn within every repetition; times in us by name"""
    first = next(iter(mems.values()))
    dev = first.device
    st = torch.cuda.current_stream(dev)
    seed(7)
    samples = draw_samples(len(first), (first.src_h, first.src_w), [H, 2 * H], scale, batch, warmup + reps, flip=flip)
    plans = {k: mem.plan(samples, H, 2 * H) for k, mem in mems.items()}
    assert not any(p.whole_frames for p in plans.values())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {k: [] for k in mems}
    for r in range(warmup + reps):
        for k, mem in mems.items():
            plan = plans[k]
            torch.cuda.synchronize(dev)
            e0.record(st)
            mem._gather_logits(plan.table_host[r], plan.table_dev[r], plan.logits, (H, 2 * H))
            e1.record(st)
            torch.cuda.synchronize(dev)
            if r >= warmup:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    return us


def time_device_phases(net, mem, iters, reps, warmup):
    """the device path alone; per-phase wall times in ms"""
    return stats(alternating_phases(net, {"device": mem}, iters, reps, warmup)["device"])


def time_logits_gather(mem, H, scale, flip, batch, reps, warmup):
    """HIP events around the logits gather of a mini-batch alone, one memory"""
    return stats(alternating_logits_gathers({"device": mem}, H, scale, flip, batch, reps, warmup)["device"])


def time_layouts(net, mems, H, scale, flip, batch, iters, reps, warmup):
    """case e: ``mems`` = {"full": memory, "selected": memory} with equal contents; the layouts alternate within every repetition, first the
    phases, then the logits gather alone, then one append"""
    dev = net.engine.device
    st = torch.cuda.current_stream(dev)
    phase_ms = alternating_phases(net, mems, iters, reps, warmup)
    gather_us = alternating_logits_gathers(mems, H, scale, flip, batch, reps, warmup)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    # one append: the frame and the label are device tensors in both forms, so that the window holds the logits' way in
    f_dev, l_dev, t_dev = (x.clone() for x in mems["full"][0])
    t_host = t_dev.cpu().numpy()
    append_dev_us, append_np_ms = {k: [] for k in mems}, {k: [] for k in mems}
    for r in range(warmup + reps):
        for k, mem in mems.items():
            torch.cuda.synchronize(dev)
            e0.record(st)
            mem.append(f_dev, l_dev, t_dev)
            e1.record(st)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            mem.append(f_dev, l_dev, t_host)
            torch.cuda.synchronize(dev)
            if r >= warmup:
                append_dev_us[k].append(e0.elapsed_time(e1) * 1e3)
                append_np_ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, mem in mems.items():
        ch = mem.logits_cached_shape[2]
        out[k] = {"channels": ch, "memory_bytes": mem.nbytes, "slot_bytes": mem.nbytes // mem.capacity,
                  "logits_bytes_written": batch * H * 2 * H * ch * 4, "device_ms": stats(phase_ms[k]),
                  "step_ms": float(np.median(phase_ms[k])) / iters, "logits_gather_us": stats(gather_us[k]),
                  "append_device_tensor_us": stats(append_dev_us[k]), "append_numpy_ms": stats(append_np_ms[k])}
    for q in ("device_ms", "logits_gather_us", "append_device_tensor_us", "append_numpy_ms"):
        out["full_over_selected_" + q] = out["full"][q]["median"] / out["selected"][q]["median"]
    return out


def time_lowres(net, mems, H, scale, flip, batch, iters, reps, warmup):
    """case f: ``mems`` = {"full_size": memory, "lowres": memory}, frames and labels equal, the small cache standing for its upsample; the two
    alternate within every repetition, first the phases, then the logits gather alone"""
    phase_ms = alternating_phases(net, mems, iters, reps, warmup)
    gather_us = alternating_logits_gathers(mems, H, scale, flip, batch, reps, warmup)
    out = {}
    for k, mem in mems.items():
        out[k] = {"logits_cached_shape": list(mem.logits_cached_shape), "memory_bytes": mem.nbytes, "slot_bytes": mem.nbytes // mem.capacity,
                  "logits_bytes_written": batch * H * 2 * H * mem.logits_cached_shape[2] * 4, "device_ms": stats(phase_ms[k]),
                  "step_ms": float(np.median(phase_ms[k])) / iters, "logits_gather_us": stats(gather_us[k])}
    for q in ("device_ms", "logits_gather_us"):
        out["lowres_over_full_size_" + q] = out["lowres"][q]["median"] / out["full_size"][q]["median"]
    out["full_size_over_lowres_memory_bytes"] = out["full_size"]["memory_bytes"] / out["lowres"]["memory_bytes"]
    return out


def time_append_labels(mem, frame, label, logits, reps, warmup):
    """case g: ``mem`` caches ``logits``' grid; host arrays in both forms.  HIP events around one append (the stream is idle before, the
    window ends when the slot is complete), the two forms alternating; then the label kernel alone on logits that are on the device."""
    dev = mem.device
    st = torch.cuda.current_stream(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    us = {"label_uploaded": [], "label_derived": [], "label_kernel_alone": []}
    for r in range(warmup + reps):
        for k in ("label_uploaded", "label_derived"):
            torch.cuda.synchronize(dev)
            e0.record(st)
            mem.append(frame, label if k == "label_uploaded" else None, logits)
            e1.record(st)
            torch.cuda.synchronize(dev)
            if r >= warmup:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    logits_dev = torch.from_numpy(logits).to(dev)
    for r in range(warmup + reps):
        torch.cuda.synchronize(dev)
        e0.record(st)
        mem.labels_from_logits(logits_dev)
        e1.record(st)
        torch.cuda.synchronize(dev)
        if r >= warmup:
            us["label_kernel_alone"].append(e0.elapsed_time(e1) * 1e3)
    out = {k + "_us": stats(v) for k, v in us.items()}
    out["derived_over_uploaded"] = out["label_derived_us"]["median"] / out["label_uploaded_us"]["median"]
    k = mem.logits_cached_shape[2]
    out["bytes_uploaded"] = {"label_uploaded": frame.nbytes + label.nbytes + logits.nbytes // logits.shape[2] * k, "label_derived": frame.nbytes + logits.nbytes}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--slots", type=int, default=12)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps_b", type=int, default=None)
    ap.add_argument("--reps_c", type=int, default=None)
    ap.add_argument("--reps_d", type=int, default=None)
    ap.add_argument("--reps_e", type=int, default=None)
    ap.add_argument("--reps_f", type=int, default=None)
    ap.add_argument("--reps_g", type=int, default=None)
    ap.add_argument("--lowres", default="33,65", help="cases f and g: the cached grid of the low-resolution memory")
    ap.add_argument("--cases", default="a,b,c,d,e,f,g,gather,asr")
    ap.add_argument("--out", default="out/time_replay.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_replay needs the GPU"
    cases = a.cases.split(",")
    H = a.height
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, a.slots, CI, seed=3).clip()
    frames, labels = [np.ascontiguousarray(f) for f in frames], [np.ascontiguousarray(l) for l in labels]
    net = SemanticNetwork("unused", class_weights_exp=exp_configs.class_weights(25), height=H, scale=[1], mini_batch_size=a.batch, lr=1e-3,
                          initial_variables=W0)
    dev = net.engine.device
    mem = DeviceReplayMemory(a.slots, H, 2 * H, dev)
    for f, l in zip(frames, labels):
        mem.append(f, l)
    host = (deque(frames), deque(labels), None)
    result = {"height": H, "width": 2 * H, "batch": a.batch, "iterations": a.iters, "slots": a.slots, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(dev), "memory_bytes": mem.nbytes}
    if "a" in cases:
        net.scale = [1]
        result["a_hard_scale1"] = time_phases(net, host, mem, a.iters, a.reps, a.warmup)
    if "c" in cases:
        net.scale = [1, 1.25, 1.5]
        result["c_multi_scale"] = time_phases(net, host, mem, a.iters, a.reps_c or a.reps, a.warmup)
        net.scale = [1]
    if "gather" in cases:
        result["gather_copy_us"] = time_gather(mem, H, [1], a.batch, a.reps, a.warmup)
        result["gather_bilinear_us"] = time_gather(mem, H, [1.25], a.batch, a.reps, a.warmup)
    if "asr" in cases:
        pairs = min(10, a.slots - 1)
        loop_ms, call_ms = [], []
        for r in range(a.warmup + a.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            first = len(mem) - 1 - pairs
            want = [net.calc_cross_miou(np.array([labels[k], labels[k + 1]]))[2] for k in range(first, len(mem) - 1)]
            t1 = time.perf_counter()
            got = [x[2] for x in mem.cross_miou_pairs(net, first)]
            t2 = time.perf_counter()
            assert len(got) == pairs and np.array_equal(want, got, equal_nan=True)
            if r >= a.warmup:
                loop_ms.append((t1 - t0) * 1e3)
                call_ms.append((t2 - t1) * 1e3)
        result["asr_pairs"] = pairs
        result["asr_loop_ms"], result["asr_one_call_ms"] = stats(loop_ms), stats(call_ms)
        result["asr_loop_over_one_call"] = result["asr_loop_ms"]["median"] / result["asr_one_call_ms"]["median"]
    if "b" in cases or "d" in cases or "e" in cases or "f" in cases:
        rng = np.random.default_rng(5)
        tl = [rng.standard_normal((H, 2 * H, 19)).astype(np.float32) for _ in range(a.slots)]
        soft_mem = DeviceReplayMemory(a.slots, H, 2 * H, dev, logits_shape=(H, 2 * H, 19))
        for f, l, t in zip(frames, labels, tl):
            soft_mem.append(f, l, t)
        net.soft_teacher = True
        net.engine.set_soft_teacher(True)
    if "b" in cases:
        result["b_soft_teacher_full_size"] = time_phases(net, (host[0], host[1], deque(tl)), soft_mem, a.iters, a.reps_b or a.reps, a.warmup)
        result["b_soft_teacher_full_size"]["memory_bytes"] = soft_mem.nbytes
    if "d" in cases:
        net.scale, net.flip = [1, 1.25, 1.5], True
        reps_d = a.reps_d or a.reps
        phase = time_device_phases(net, soft_mem, a.iters, reps_d, a.warmup)
        result["d_soft_teacher_augmented"] = {
            "scale": net.scale, "flip": True, "device_ms": phase, "step_ms": phase["median"] / a.iters,
            "logits_gather_us": time_logits_gather(soft_mem, H, net.scale, True, a.batch, reps_d, a.warmup),
            "logits_bytes_written": a.batch * H * 2 * H * 19 * 4, "memory_bytes": soft_mem.nbytes}
        net.scale, net.flip = [1], False
    if "e" in cases:
        sel_mem = DeviceReplayMemory(a.slots, H, 2 * H, dev, logits_shape=(H, 2 * H, 19), logits_select=CI)
        for f, l, t in zip(frames, labels, tl):
            sel_mem.append(f, l, t)
        net.scale, net.flip = [1, 1.25, 1.5], True
        result["e_logit_layouts"] = time_layouts(net, {"full": soft_mem, "selected": sel_mem}, H, net.scale, True, a.batch, a.iters,
                                                 a.reps_e or a.reps, a.warmup)
        result["e_logit_layouts"].update({"scale": net.scale, "flip": True, "class_idx": CI})
        net.scale, net.flip = [1], False
    if "f" in cases:
        lh, lw = (int(v) for v in a.lowres.split(","))
        low_mem = DeviceReplayMemory(a.slots, H, 2 * H, dev, logits_shape=(lh, lw, 19), logits_upsample=True)
        for f, l in zip(frames, labels):
            low_mem.append(f, l, rng.standard_normal((lh, lw, 19)).astype(np.float32))
        net.scale, net.flip = [1, 1.25, 1.5], True
        result["f_lowres_logits"] = time_lowres(net, {"full_size": soft_mem, "lowres": low_mem}, H, net.scale, True, a.batch, a.iters,
                                                a.reps_f or a.reps, a.warmup)
        result["f_lowres_logits"].update({"scale": net.scale, "flip": True, "reps": a.reps_f or a.reps})
        net.scale, net.flip = [1], False
    if "g" in cases:
        lh, lw = (int(v) for v in a.lowres.split(","))
        video = synth.SyntheticVideo(H, a.slots, CI, seed=3)
        grid_mem = DeviceReplayMemory(a.slots, H, 2 * H, dev, logits_shape=(lh, lw, 19), logits_upsample=True, logits_select=CI)
        result["g_append_labels_from_logits"] = time_append_labels(grid_mem, frames[0], labels[0], video.teacher_logits(0, lh, lw), a.reps_g or a.reps,
                                                                   a.warmup)
        result["g_append_labels_from_logits"].update({"logits_shape": [lh, lw, 19], "class_idx": CI, "reps": a.reps_g or a.reps})
    result["note"] = ("*_ms: host clock around train_with_deque, stream drained before and after, host path and device path alternating with equal "
                      "seeds; gather_*_us: HIP events around the one launch, stream otherwise idle; asr_*: host clock, results compared; "
                      "d_*: device path only, logits_gather_us = HIP events around ams_replay_gather_logits alone; e_*: the full and the "
                      "selected layout alternating with equal seeds and descriptors, append_* = one append of a frame with its logits; f_*: a memory "
                      "with logits at the frame size and one with a low-resolution cache (logits_upsample) alternating with equal seeds and "
                      "descriptors, logits_gather_us = HIP events around ams_replay_gather_logits / ams_replay_gather_logits_lowres alone; g_*: HIP events "
                      "around one append of host arrays (frame, 33 x 65 x 19 logits) with the label map uploaded or derived on the device, "
                      "alternating, and around ams_teacher_labels_from_logits alone")
    net.close_model()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
