"""Timing of the uplink frame codec on a synthetic clip frame at the upload size of --height H (2H x 4H).

    python tools/uplink_bench.py --height 512 --out out/uplink.json              # HIP events around each C entry: median, p10 - p90
    rocprofv3 --kernel-trace --stats -d out/uplink_trace -- python tools/uplink_bench.py --height 512 --reps 20
    python tools/uplink_bench.py --trace out/uplink_trace --out out/uplink_kernels.json   # per kernel: median, p10 - p90 of the dispatches

The frame is encoded at a budget (--budget bytes) and at q = 50 and 90; sizes and qualities are printed with the times.

--inter times the predicted frame's entries (ams_uplink_inter_*) and kernels the same way, next to the intra ones in the same window: clip
frame 1 against clip frame 0 as the decoder gives it at the budget's quality.

    python tools/uplink_bench.py --inter --height 512 --out profiles/uplink_inter_1024x2048_calls.json
    rocprofv3 --kernel-trace --stats -d out/uplink_inter_trace -- python tools/uplink_bench.py --inter --height 512 --reps 20
    python tools/uplink_bench.py --trace out/uplink_inter_trace --out profiles/uplink_inter_1024x2048_kernels.json
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def spread(v):
    v = np.asarray(v, np.float64)
    return {"median": float(np.median(v)), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "n": int(len(v))}


def trace_stats(root):
    """rocprofv3's kernel trace under `root` -> {kernel: spread of the dispatch durations in microseconds} for the codec's kernels"""
    out = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row["Kernel_Name"]
                if "uplink_" in name:
                    key = name.split("(")[0].split("::")[-1]
                    out.setdefault(key, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1000.0)
    return {k: spread(v[len(v) // 5:]) for k, v in sorted(out.items())}          # the first fifth of each kernel's dispatches is warm-up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--budget", type=int, default=25000)
    ap.add_argument("--trace", default=None)
    ap.add_argument("--inter", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trace:
        res = {"kernels_us": trace_stats(a.trace)}
    else:
        import ctypes as C
        import torch
        from ams_amd import hip, synth
        from ams_amd.ingest import FrameIngest
        from ams_amd.uplink import UplinkCodec
        assert torch.cuda.is_available(), "needs a GPU"
        H, W = 2 * a.height, 4 * a.height
        frame = FrameIngest("cuda:0").frame(synth.SyntheticVideo(a.height, 1, [0, 1, 2, 10, 11, 13], seed=3).frame(0)[0], H, W)
        codec = UplinkCodec("cuda:0")
        lib, st = codec.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        payload, q, fits = codec.encode_to_budget(frame, a.budget)
        sizes = codec.size_table(frame)
        scratch, sizes_dev, nbytes, status = codec._encoder(H, W)
        cap = codec.max_payload_bytes(H, W)
        room = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        payloads = {k: codec.encode(frame, k) for k in sorted({q, 50, 90})}
        for p in payloads.values():
            codec.decode(p, (H, W))
        dscratch, dstatus = codec._dec[(H, W)]
        out = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda:0")
        p = lambda t: C.c_void_p(t.data_ptr())
        calls = {"transform": lambda: lib.ams_uplink_transform(p(frame), H, W, p(scratch), scratch.numel(), st),
                 "size_table": lambda: lib.ams_uplink_size_table(p(scratch), scratch.numel(), H, W, p(sizes_dev), st)}
        for k, pl in payloads.items():
            calls["encode_q%d" % k] = lambda k=k: lib.ams_uplink_encode(p(scratch), scratch.numel(), H, W, k, p(room), cap, p(nbytes), p(status), st)
            calls["decode_q%d" % k] = lambda pl=pl: lib.ams_uplink_decode(p(pl), pl.numel(), H, W, p(out), p(dstatus), p(dscratch), dscratch.numel(), st)
        extra = {}
        if a.inter:
            video = synth.SyntheticVideo(a.height, 1, [0, 1, 2, 10, 11, 13], seed=3)
            ref = codec.decode(payload, (H, W))                   # frame 0 as the server has it
            cur = FrameIngest("cuda:0").frame(video.frame(1)[0], H, W)
            ppayload, pq, pfits = codec.encode_to_budget(cur, a.budget, reference=ref)
            psizes = codec.size_table(cur, reference=ref)
            pscratch, psizes_dev, pnbytes, pstatus = codec._encoder_p(H, W)
            pcap = int(lib.ams_uplink_inter_max_bytes(H, W))
            proom = torch.empty(pcap, dtype=torch.uint8, device="cuda:0")
            ppayloads = {k: codec.encode(cur, k, reference=ref) for k in sorted({pq, 50, 90})}
            for pl in ppayloads.values():
                codec.decode(pl, reference=ref)
            pdscratch, pdstatus = codec._dec_p[(H, W)]
            calls["inter_transform"] = lambda: lib.ams_uplink_inter_transform(p(cur), p(ref), H, W, p(pscratch), pscratch.numel(), st)
            calls["inter_size_table"] = lambda: lib.ams_uplink_inter_size_table(p(pscratch), pscratch.numel(), H, W, p(psizes_dev), st)
            for k, pl in ppayloads.items():
                calls["inter_encode_q%d" % k] = lambda k=k: lib.ams_uplink_inter_encode(p(pscratch), pscratch.numel(), H, W, k, p(proom), pcap,
                                                                                        p(pnbytes), p(pstatus), st)
                calls["inter_decode_q%d" % k] = lambda pl=pl: lib.ams_uplink_inter_decode(p(pl), pl.numel(), p(ref), H, W, p(out), p(pdstatus),
                                                                                          p(pdscratch), pdscratch.numel(), st)
            from ams_amd.uplink import kind_of
            extra = {"inter_budget_quality": pq, "inter_budget_kind": kind_of(ppayload), "inter_fits": pfits,
                     "inter_payload_bytes": {str(k): int(v.numel()) for k, v in ppayloads.items()},
                     "inter_sizes_q1_q50_q100": [int(psizes[0]), int(psizes[49]), int(psizes[99])]}
        times = {k: [] for k in calls}
        for rep in range(8 + a.reps):                             # the entries alternate inside one window; 8 warm-up rounds
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                hip.check(fn(), k)
                e1.record()
                e1.synchronize()
                if rep >= 8:
                    times[k].append(1000.0 * e0.elapsed_time(e1))
        res = {"frame": [H, W], "budget": a.budget, "budget_quality": q, "fits": fits, "payload_bytes": {str(k): int(v.numel()) for k, v in payloads.items()},
               "sizes_q1_q50_q100": [int(sizes[0]), int(sizes[49]), int(sizes[99])], "calls_us": {k: spread(v) for k, v in times.items()}}
        res.update(extra)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
