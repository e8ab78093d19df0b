"""Record what the frozen forward launches and computes, so that two builds of the library can be compared byte for byte.

    AMS_HIP_LIB=<build A>/libams_hip.so python tools/plan_identity.py --out a.json
    AMS_HIP_LIB=<build B>/libams_hip.so python tools/plan_identity.py --out b.json
    cmp a.json b.json

For a fixed list of cases (matmul modes x batch sizes at defaults; from the default mode one option at a time through its values; layers
moved outside fp16's range around the stride-16 hand-overs) with seeded weights and frames, at 64 x 128 and 512 x 1024, the file holds per
case: the profile hook's rows without the time column (kernel name with template arguments, layer, bytes, flops, flops_x6), a checksum
of the low-res logits and of the label maps of that profiled call, and the same two checksums of a call with the profiler off (the profiler
forces the one-stream plan, so the multi-part plans are only covered by the second call).  At 64 x 128 it also holds the losses and a
checksum of the parameters after three seeded single-rank train_steps, twice (the two must agree for the comparison to mean anything).

One child process per frame size, each under a time limit of its own; nothing further is started after a non-zero exit.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CI = [0, 1, 2, 10, 11, 13]
MAX_BATCH = 32
BIG = 20                                    # x 2^20: weights ~ 1e5, beyond fp16's 65504


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def scaled(W, ks):
    """W with each scope of ``ks`` scaled by 2^k and its BN compensating (the same function; tests/test_gpu_f16_range.py)"""
    import numpy as np
    W = dict(W)
    for scope, k in ks.items():
        f = np.float32(2.0 ** k)
        W[scope + "/weights:0"] = W[scope + "/weights:0"] * f
        W[scope + "/BatchNorm/moving_mean:0"] = W[scope + "/BatchNorm/moving_mean:0"] * f
        W[scope + "/BatchNorm/gamma:0"] = W[scope + "/BatchNorm/gamma:0"] * np.float32(2.0 ** -k)
    return W


def cases(hip, H):
    """(name, batch, matmul mode, {option: value}, {scope: k})"""
    rows16 = (H // 16) * (2 * H // 16)
    D = hip.MATMUL_SPLIT_F16
    modes = [("f32", hip.MATMUL_F32), ("bf16x2", hip.MATMUL_SPLIT_BF16), ("bf16x3", hip.MATMUL_SPLIT_BF16_X6), ("bf16", hip.MATMUL_BF16),
             ("f16", D)]
    out = [("mode %s B%d" % (n, b), b, m, {}, {}) for n, m in modes for b in (1, 2, 8, 32)]
    B = 8
    one = [(hip.OPT_FUSE_FIRST_BLOCK, (0, 1, 2)), (hip.OPT_FUSE_BLOCK, (0, 1)), (hip.OPT_FUSE_EXPAND_DW, (0, 1, 2)),
           (hip.OPT_FUSE_EXPAND_DW_STREAM, (0, 1, 2)), (hip.OPT_FUSE_DW_PROJECT, (0, 1)), (hip.OPT_BLOCK_X6, (0, 1)),
           (hip.OPT_STREAM_MIN_ROWS, (0, B * rows16 + 1)), (hip.OPT_EMULATE_BF16_STORAGE, (1,)), (hip.OPT_OVERLAP_HEAD, (1,)),
           (hip.OPT_DUAL_STREAM, (0,))]
    for opt, values in one:
        out += [("opt %d=%d B%d" % (opt, v, B), B, D, {opt: v}, {}) for v in values]
    out += [("opt %d=%d bf16x2 B%d" % (hip.OPT_FUSE_DW_PROJECT, v, B), B, hip.MATMUL_SPLIT_BF16, {hip.OPT_FUSE_DW_PROJECT: v}, {}) for v in (0, 1)]
    out += [("late 16 B32", 32, D, {hip.OPT_LATE_SUBBATCH: 16}, {}), ("late 5 B8", 8, D, {hip.OPT_LATE_SUBBATCH: 5}, {})]
    out += [("dual forced %d parts B7" % n, 7, D, {hip.OPT_DUAL_STREAM: 2, hip.OPT_DUAL_PARTS: n}, {}) for n in (2, 3, 4)]
    # every block layer by layer, tiled and streamed wherever supported, streaming from the first row: each in every mode
    for n, m in modes:
        out.append(("layers %s B%d" % (n, B), B, m, {hip.OPT_FUSE_BLOCK: 0, hip.OPT_FUSE_EXPAND_DW: 0, hip.OPT_FUSE_EXPAND_DW_STREAM: 0}, {}))
        out.append(("stream all %s B%d" % (n, B), B, m, {hip.OPT_FUSE_BLOCK: 0, hip.OPT_FUSE_EXPAND_DW_STREAM: 2, hip.OPT_STREAM_MIN_ROWS: 0}, {}))
        out.append(("emulate %s B%d" % (n, B), B, m, {hip.OPT_EMULATE_BF16_STORAGE: 1, hip.OPT_STREAM_MIN_ROWS: 0}, {}))
    # the hand-over states: a stride-16 expand layer with Cin 64, one with Cin 160, a project layer in front of one — beyond fp16's range
    e64, e160, pj = "MobilenetV2/expanded_conv_8/expand", "MobilenetV2/expanded_conv_15/expand", "MobilenetV2/expanded_conv_10/project"
    for label, scopes in (("expand Cin 64", [e64]), ("expand Cin 160", [e160]), ("project", [pj]), ("all three", [e64, e160, pj]),
                          ("expand + its project", ["MobilenetV2/expanded_conv_14/expand", "MobilenetV2/expanded_conv_14/project"])):
        ks = {s: BIG for s in scopes}
        out.append(("range %s B%d" % (label, B), B, D, {}, ks))
        out.append(("range %s rows 0 B%d" % (label, 2), 2, D, {hip.OPT_STREAM_MIN_ROWS: 0}, ks))
        out.append(("range %s dual B%d" % (label, 7), 7, D, {hip.OPT_DUAL_STREAM: 2, hip.OPT_DUAL_PARTS: 3, hip.OPT_STREAM_MIN_ROWS: 0}, ks))
    return out


def child(H, out_path):
    import torch
    from ams_amd import hip, spec as S, synth, weights as Wt
    from ams_amd.engine import StudentEngine

    W0 = Wt.synthetic_weights(S.build_spec(), seed=0)
    frames, labels = synth.SyntheticVideo(H, MAX_BATCH, CI, seed=5).clip()
    defaults = {hip.OPT_FUSE_FIRST_BLOCK: 1, hip.OPT_FUSE_BLOCK: 1, hip.OPT_FUSE_EXPAND_DW: 1, hip.OPT_FUSE_EXPAND_DW_STREAM: 1,
                hip.OPT_FUSE_DW_PROJECT: 0, hip.OPT_BLOCK_X6: 1, hip.OPT_STREAM_MIN_ROWS: 4096, hip.OPT_EMULATE_BF16_STORAGE: 0,
                hip.OPT_OVERLAP_HEAD: 0, hip.OPT_LATE_SUBBATCH: 0, hip.OPT_DUAL_STREAM: 1, hip.OPT_DUAL_PARTS: 2, hip.OPT_DUAL_AUTOTUNE: 0}
    eng = StudentEngine(CI, H, 2 * H, max_batch=MAX_BATCH, trainable=False)
    h, w = eng.lowres
    result = {"height": H, "cases": []}
    n_launches = 0

    def sums(fr):
        lab = eng.predict(fr)
        torch.cuda.synchronize()
        return {"logits": sha(eng.logits_lowres.view(-1, h, w, 32)[:len(fr)]), "labels": sha(lab)}

    state = None
    for name, B, mode, opts, ks in cases(hip, H):
        for opt, v in {**defaults, **opts}.items():
            hip.check(eng.lib.ams_student_set_option(eng._h, opt, int(v)))
        if state != (mode, tuple(sorted(ks))):
            eng.set_matmul_mode(mode)
            eng.load_variables(scaled(W0, ks) if ks else W0)
            eng.freeze()
            state = (mode, tuple(sorted(ks)))
        fr = frames[:B]
        hip.check(eng.lib.ams_student_profile(eng._h, 1))
        try:
            profiled = sums(fr)
            need = C.c_size_t(0)
            hip.check(eng.lib.ams_student_profile_read(eng._h, None, 0, C.byref(need)))
            buf = C.create_string_buffer(need.value + 16)
            hip.check(eng.lib.ams_student_profile_read(eng._h, buf, len(buf), C.byref(need)))
        finally:
            hip.check(eng.lib.ams_student_profile(eng._h, 0))
        rows = []
        for line in buf.value.decode().splitlines():
            f = line.split("\t")
            rows.append([f[0], int(f[1])] + f[3:])              # without the time column
        n_launches += len(rows)
        result["cases"].append({"name": name, "fallback_layers": eng.f16_fallback_layers(), "rows": rows, "profiled": profiled, "plain": sums(fr)})
        print("%4d  %-40s %3d launches" % (H, name, len(rows)), flush=True)
    eng.close()
    result["n_cases"], result["n_launches"] = len(result["cases"]), n_launches

    if H == 64:
        # item: three seeded fine-tune steps, single rank, on a fresh engine — twice
        result["train"] = []
        for run in range(2):
            eng = StudentEngine(CI, H, 2 * H, max_batch=4, trainable=True)
            eng.load_variables(W0)
            losses = []
            for step in range(3):
                ls = eng.train_step(frames[4 * step:4 * step + 4], labels[4 * step:4 * step + 4], 1e-3)
                losses.append(ls.cpu().numpy().tobytes().hex())
            torch.cuda.synchronize()
            result["train"].append({"losses": losses, "params": sha(eng.params), "stats": sha(eng.stats)})
            eng.close()
        print("train steps: runs agree: %s" % (result["train"][0] == result["train"][1]), flush=True)
    Path(out_path).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", required=True, help="JSON file to write")
    ap.add_argument("--heights", default="64,512", help="frame heights (width = 2 x height), one child process each")
    ap.add_argument("--timeout", type=int, default=420, help="seconds per child process")
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child, args.out)
        return 0
    parts = []
    for H in [int(x) for x in args.heights.split(",")]:
        part = "%s.%d.part" % (args.out, H)
        rc = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", str(H),
                             "--out", part]).returncode
        if rc != 0:
            print("frame height %d: exit status %d — nothing further is started" % (H, rc), file=sys.stderr)
            return rc
        parts.append(json.loads(Path(part).read_text()))
        os.remove(part)
    Path(args.out).write_text(json.dumps(parts, indent=1, sort_keys=True) + "\n")
    print("%s: %d cases, %d launches" % (args.out, sum(p["n_cases"] for p in parts), sum(p["n_launches"] for p in parts)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
