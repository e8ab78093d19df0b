"""Time the edge-side model update at 512 x 1024: payload host -> device, the decode kernels (k_delta.hip), the re-freeze.

Two payloads: a 10 % coord_desc_rand delta (trainable layout) and a full_model delta (all-variables layout, every value sent).  Each phase is
timed with device events over --reps repetitions after --warmup, and the whole update (StudentEngine.apply_delta from host bytes + freeze,
what SemanticNetwork.apply_delta does on a frozen edge) with the host clock.  The decode is timed from the payload already on the device
(table upload + delta_count_kernel + delta_scan_kernel + delta_apply_kernel); its bytes are the mask section read twice, the values read
once and the f32 results written.  Writes one JSON (--out) and prints it.

    python tools/time_edge_update.py [--reps 50] [--warmup 5] [--out out/time_edge_update.json]
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

from ams_amd import coord_masks, delta as D, spec as S, weights as Wt  # noqa: E402
from ams_amd.engine import StudentEngine  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]


def payload_for(spec, strategy, rng):
    L = D.delta_layout(spec, strategy)
    if strategy == "full_model":
        masks = [np.ones(e.count, bool) for e in L.entries]
    else:
        shapes = {v.name: v.shape for v in spec.trainable}
        m = coord_masks.build_mask(strategy, 0.1, shapes)
        masks = [np.asarray(m[e.name]).reshape(-1) for e in L.entries]
    out = bytearray()
    for m in masks:
        out += np.packbits(m).tobytes()
    for e, m in zip(L.entries, masks):
        out += (0.05 * rng.standard_normal(e.count)).astype(np.float32)[m].astype(np.float16).tobytes()
    return L, bytes(out), int(sum(int(m.sum()) for m in masks))


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"mean": float(xs.mean()), "median": float(np.median(xs)), "min": float(xs.min()), "max": float(xs.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="out/time_edge_update.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_edge_update needs the GPU"
    spec = S.build_spec()
    W0 = Wt.synthetic_weights(spec, seed=0)
    eng = StudentEngine(CI, a.height, 2 * a.height, max_batch=1, trainable=False)
    eng.load_variables(W0)
    eng.freeze()
    st = torch.cuda.current_stream(eng.device)
    rng = np.random.default_rng(0)
    result = {"height": a.height, "width": 2 * a.height, "reps": a.reps, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(eng.device), "payloads": {}}
    for strategy in ("coord_desc_rand", "full_model"):
        L, payload, n_values = payload_for(spec, strategy, rng)
        host = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).pin_memory()
        dev = torch.empty(len(payload), dtype=torch.uint8, device=eng.device)
        table = L.table()
        scratch = torch.empty(int(eng.lib.ams_student_apply_delta_scratch(table, len(table))), dtype=torch.int64, device=eng.device)
        words = torch.zeros(2, dtype=torch.int64, device=eng.device)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
        h2d, dec, frz, upd = [], [], [], []
        for r in range(a.warmup + a.reps):
            eng.load_variables(W0)
            torch.cuda.synchronize()
            ev[0].record(st)
            dev.copy_(host, non_blocking=True)
            ev[1].record(st)
            rc = eng.lib.ams_student_apply_delta(eng._h, C.c_void_p(dev.data_ptr()), len(payload), table, len(table),
                                                 C.c_void_p(words.data_ptr()), C.c_void_p(words.data_ptr() + 8),
                                                 C.c_void_p(scratch.data_ptr()), scratch.numel(), eng._stream())
            assert rc == 0, eng.lib.ams_last_error()
            ev[2].record(st)
            ev[3].record(st)
            eng.freeze()
            ev[4].record(st)
            torch.cuda.synchronize()
            w = words.cpu().numpy()
            assert int(w[1:].view(np.int32)[0]) == 0 and int(w[0]) == n_values
            # the whole update as a frozen edge runs it: host bytes in -> model re-frozen
            eng.load_variables(W0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assert eng.apply_delta(payload, L) == n_values
            eng.freeze()
            t1 = time.perf_counter()
            if r >= a.warmup:
                h2d.append(ev[0].elapsed_time(ev[1]) * 1e3)
                dec.append(ev[1].elapsed_time(ev[2]) * 1e3)
                frz.append(ev[3].elapsed_time(ev[4]) * 1e3)
                upd.append((t1 - t0) * 1e3)
        dec_bytes = 2 * L.mask_bytes + 2 * n_values + 4 * n_values
        result["payloads"][strategy] = {
            "layout": L.kind, "payload_bytes": len(payload), "mask_bytes": L.mask_bytes, "values": n_values,
            "h2d_us": stats(h2d), "decode_us": stats(dec), "freeze_us": stats(frz), "update_host_ms": stats(upd),
            "decode_bytes": dec_bytes, "decode_GBps_median": dec_bytes / (np.median(dec) * 1e-6) / 1e9,
            "note": "decode_us = table upload + 3 kernels, payload on the device; freeze_us includes freeze's own stream synchronisation; "
                    "update_host_ms = apply_delta(host bytes) + freeze, host clock",
        }
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
