"""Time the 8-frame 512 x 1024 fine-tune step with hard-pixel mining off and at top_k = 0.25, alternating in one process on one GPU, and
(--other-tree DIR) against another checkout of the project, alternating processes of the two trees.

  step_ms        host clock around train_step with the stream drained before and after, the variants alternating step by step; median, p10 / p90
  kernels        the engine's per-launch profiler (HIP events around every launch, a separate pass): the ordered list of kernel names of one step,
                 and the time of the three mining launches (key; select = three histogram + scan passes; relabel) and of the loss kernel
  other tree     --rounds times, each in a fresh process: `--variants off --child` run from DIR, the same from this tree, then this tree's
                 two variants: the other tree's step time and the spread between its own processes, this tree's unmined step measured the
                 same way, and whether the kernel lists of all the unmined steps are equal

    python tools/time_loss_mining.py [--reps 40] [--warmup 8] [--other-tree DIR] [--out profiles/loss_mining_512x1024.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

from ams_amd import hip, spec as S, synth, weights as Wt  # noqa: E402
from ams_amd.engine import StudentEngine  # noqa: E402

CI = [0, 1, 2, 10, 11, 13]


def stats(xs):
    xs = np.asarray(xs, np.float64)
    return {"median": float(np.median(xs)), "mean": float(xs.mean()), "min": float(xs.min()), "max": float(xs.max()),
            "p10": float(np.percentile(xs, 10)), "p90": float(np.percentile(xs, 90)), "n": int(xs.size)}


def read_profile(eng):
    need = C.c_size_t(0)
    hip.check(eng.lib.ams_student_profile_read(eng._h, None, 0, C.byref(need)))
    buf = C.create_string_buffer(need.value + 16)
    hip.check(eng.lib.ams_student_profile_read(eng._h, buf, len(buf), C.byref(need)))
    return [(line.split("\t")[0], float(line.split("\t")[2])) for line in buf.value.decode().splitlines()]


def measure(variants, H, B, reps, warmup):
    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, B, CI, seed=3).clip()
    eng = StudentEngine(CI, H, 2 * H, max_batch=B, trainable=True)
    eng.load_variables(W0)
    dev = eng.device
    fd = torch.as_tensor(np.ascontiguousarray(frames)).to(dev)
    ld = torch.as_tensor(np.ascontiguousarray(labels)).to(dev)
    top_k = {"off": 1.0, "top_k_0.25": 0.25}

    def step(v):
        if v != "off" or len(variants) > 1:
            eng.set_loss_mining(top_k[v])
        return eng.train_step(fd, ld, 1e-4)

    ms = {v: [] for v in variants}
    for k in range(warmup + reps):
        for v in variants:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            step(v)
            torch.cuda.synchronize(dev)
            if k >= warmup:
                ms[v].append((time.perf_counter() - t0) * 1e3)
    out = {"step_ms": {v: stats(x) for v, x in ms.items()}, "kernels": {}}
    for v in variants:                                  # the profiler pass: three steps, the last one's rows
        rows = []
        for _ in range(3):
            hip.check(eng.lib.ams_student_profile(eng._h, 1))
            step(v)
            torch.cuda.synchronize(dev)
            rows = read_profile(eng)
            hip.check(eng.lib.ams_student_profile(eng._h, 0))
        pick = {n: round(t * 1e3, 2) for n, t in rows if n.startswith("mining_") or n.startswith("ce_loss_grad")}
        out["kernels"][v] = {"names": [n for n, _ in rows], "launch_us": pick, "profiled_step_ms": round(sum(t for _, t in rows), 4)}
    if "top_k_0.25" in variants:
        out["mining_result"] = eng.mining_result()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--variants", default="off,top_k_0.25")
    ap.add_argument("--other-tree", default=None, help="another checkout (built) to time the unmined step of, in processes of its own")
    ap.add_argument("--rounds", type=int, default=3, help="with --other-tree: processes per tree and variant set")
    ap.add_argument("--child", action="store_true", help="print the result as one JSON line and nothing else")
    ap.add_argument("--out", default="profiles/loss_mining_512x1024.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "time_loss_mining needs the GPU"
    if a.child:
        print(json.dumps(measure(a.variants.split(","), a.height, a.batch, a.reps, a.warmup)), flush=True)
        return
    result = {"height": a.height, "width": 2 * a.height, "batch": a.batch, "reps": a.reps, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "runs": []}

    def child(tree, variants):
        tree = os.path.abspath(tree)
        cmd =[sys.executable, os.path.join(tree, "tools", "time_loss_mining.py"), "--child", "--variants", variants, "--height", str(a.height),
               "--batch", str(a.batch), "--reps", str(a.reps), "--warmup", str(a.warmup)]
        p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=400)
        if p.returncode != 0:
            raise RuntimeError("child in %s failed (%d): %s" % (tree, p.returncode, p.stderr[-2000:]))
        return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])

    # "this_off": this tree timing the unmined step alone, as the other tree's processes do (in "this" the unmined step follows a mined one)
    order = ["this"] if not a.other_tree else ["other", "this_off", "this"] * a.rounds
    for who in order:
        r = child(a.other_tree, "off") if who == "other" else child(ROOT, "off" if who == "this_off" else a.variants)
        result["runs"].append({"tree": who, **r})
        print(who, json.dumps(r["step_ms"]), flush=True)
    if a.other_tree:
        names = [r["kernels"]["off"]["names"] for r in result["runs"]]
        result["off_kernel_list_equals_other_tree"] = all(n == names[0] for n in names)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    small = {k: v for k, v in result.items() if k != "runs"}
    small["runs"] = [{"tree": r["tree"], "step_ms": r["step_ms"], "launch_us": {v: k["launch_us"] for v, k in r["kernels"].items()},
                      "mining_result": r.get("mining_result")} for r in result["runs"]]
    print(json.dumps(small, indent=1))


if __name__ == "__main__":
    main()
