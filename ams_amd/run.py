"""Edge/server scheduler around the hot path — the *intended* semantics of the reference's run.py.

Same flags (run.py:18-69), same call order on ``SemanticNetwork`` (construct -> save initial frozen model; per
training event: [phi-score / ASR / ATR] -> ``restore_initial`` -> ``train_with_deque`` -> delta accounting ->
``save_to_frozen_graph``; edge: reload at every event time, ``predict_with_metric`` per frame), same output files
(``*_fps_client.npy``, ``*_bw_uplink.npy``, ``*_bw_downlink.npy``, ``*_model_update_times.npy``, ``*_update.txt``,
``*_loss.npy``, ``*_mioucats.npy``, ``*_mious.npy``, ``*_mioumems.npy``).  The reference file does not run as
committed; the defects listed in SURVEY.md Appendix D are resolved towards their evident intent:
  * sampling and training fire ONCE per matching second (reference: once per frame of that second);
  * ``label_memory.append`` (reference ``extend`` pushes rows);
  * first training at ceil(100 / train_period) * train_period seconds, then every ``train_period`` (int range);
  * uplink sampling follows the reference by default (``--sampling reference``): ``send_rate = sampling_period / fps``
    (run.py:115; 1.0 at the defaults 30 / 30) is handed to ``choose_frames`` as the FRACTION of the bucket (run.py:175), so at
    the defaults every bucketed frame is uploaded and the replay memory of ``memory_len / sampling_period * fps`` entries
    spans a few seconds; ASR moves it inside [0.1, 1] (run.py:287-288).  ``--sampling per_second`` is the evident intent of
    the flag names instead: ``send_rate`` counts frames per SECOND (``fps / sampling_period`` at the start, started inside
    ASR's [0.1, 1] when ASR is on), ``choose_frames`` receives ``send_rate / fps``, and the replay memory spans
    ``memory_len`` seconds.  ``*_fps_client.npy``, the uplink byte counts, ``*_update.txt`` totals and the replay-memory
    contents (hence the fine-tuned models) differ between the two settings; INTEGRATION.md lists them;
  * samples are uploaded every ``train_period`` seconds (the reference's last ``train_model`` argument, run.py:600-601);
  * a training event that finds the replay memory empty still publishes the current model for that time, so that the edge
    has a model to load (the reference would fail inside ``mini_batch``);
  * ``--save_pic`` (run.py:441-454): the reference unpacks the ``(colour, overlay)`` pair of ``colorize`` / ``colorize_teacher`` into swapped
    names, so its ``overlay_*.png`` files hold the bare colour maps and its ``output_*.png`` files the overlays; here the ``overlay_*`` files
    hold the overlays.  The reference rewrites ``<results>_<second>_*.png`` at every frame (``second = i / fps`` after ``i`` advanced), so only
    the last frame of each label survives; here only those frames are painted and written.  ``cross_ignore`` raises IndexError on a teacher id
    from the class count on (255 = unlabelled in the synthetic clips); the pictures count such a pixel as ignored, as the metric does.
  * ``--compress_uplink`` (run.py:177-266 there: sampled frames at twice the network size through ffmpeg/libx264 at a bitrate the flag
    ``uplink_bw`` is read for but never defined): there is no ffmpeg here, so the lossy leg is an intra-frame transform codec of the project's own
    (``ams_amd.uplink``, format AUC1), encoded and decoded on the device.  A sampled frame is resized to 2H x 4H, encoded at the largest of the
    100 qualities whose payload fits the frame's budget, decoded, resized to H x 2H and only then stored: the server trains on what the decoder
    gives back, and ``*_bw_uplink.npy`` counts the payload bytes.  Budget rule: with ``--uplink_bw`` in kbit/s (added flag, default 200: a
    choice, not a measurement) an upload of n frames gives each floor(uplink_bw * 1000 / 8 * period / n) bytes, period = the upload period of
    the loop in seconds.  The byte counts are this codec's, NOT H.264's: no byte parity, and no inter-frame prediction unless
    ``--uplink_gop`` asks for it.
    ``<results>_uplink_quality.npy`` has one row per upload: second, frames, bytes, budget per frame, min q, mean q, frames that did not fit;
    ``--uplink_gop N`` (added flag, default 1 = all of the above unchanged): the frames of one upload travel as the reference's one clip per
    upload does, frame k with k % N != 0 predicted from the decoded frame k - 1 where that is the better payload (format AUP1, motion search
    on the device; the choice per frame is exact, from the sizes of both kinds), frame k of n at (upload bytes - spent) // (n - k) bytes; the
    budget column stays the even split; ``<results>_uplink_kinds.npy``: per upload second, intra frames, inter frames, zero-length slices,
    all slices;
Out of scope (networking emulation / reporting): H.264 byte parity of the uplink, PNG-exact uplink byte counts without
``--compress_uplink`` (zlib-deflated frame size is logged instead), the matplotlib plots.
Video comes from a ``FrameSource``: there is no OpenCV here (pictures are written by ``ams_amd.png``), so ``--input_video`` is either
``synthetic:<NUM>-<name>[:seconds=S][:fps=F]`` (procedural clip) or a directory holding
``frame_%06d.npy`` (RGB uint8) and ``gt_%06d.npy`` files, with ``--soft_teacher`` also ``logits_%06d.npy`` (the teacher's logits, f32
[lh, lw, classes] on its own grid) beside the gt files.
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys
import time
import zlib
from collections import deque
from typing import List, Optional, Tuple

import numpy as np

from . import png
from .confidence import NB as CONFIDENCE_BINS
from .delta import delta_layout
from .exp_configs import class_weights, coco_class_converter, is_coco, test_length
from .semantic_network import FrozenGraph, SemanticNetwork
from .synth import SyntheticVideo
from .utils import (balanced_class_weights, calculate_miou, choose_frames, label_class_counts, loss_knobs_problem, resize_linear,
                    resize_nearest, string_class_iou)


# ----------------------------------------------------------------------------------------------------------- flags
def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="AMS edge/server emulation on MI355X")
    req = dict(required=True)
    p.add_argument("--input_video", **req, help="synthetic:<NUM>-<name>[:seconds=S][:fps=F] or a frame directory NUM-NAME")
    p.add_argument("--gt_video", default="", help="directory of gt_%%06d.npy labels (unused for synthetic input)")
    p.add_argument("--student_checkpoint", **req, help="path prefix of <prefix>.npy, or 'synthetic[:seed]'")
    p.add_argument("--output_dir", **req)
    p.add_argument("--gpu", default="0")
    p.add_argument("--initial_fill", action="store_true")
    p.add_argument("--memory_len", type=int, default=250)
    p.add_argument("--batch_size", type=int, default=10)
    p.add_argument("--iter", type=int, default=200)
    p.add_argument("--height", type=int, default=256)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--send_period", type=int, default=30)
    p.add_argument("--train_period", type=int, default=10)
    p.add_argument("--only_results", action="store_true")
    p.add_argument("--compress_uplink", action="store_true",
                   help="uplink: sampled frames travel at twice the network size through the lossy frame codec of ams_amd.uplink at the byte "
                        "budget --uplink_bw gives (needs a GPU and --height a multiple of 8); the server trains on the decoded frames and the "
                        "uplink is counted in payload bytes.  The reference's H.264 leg in mechanism, not in byte counts")
    p.add_argument("--uplink_gop", type=int, default=1,
                   help="--compress_uplink: within one upload, frame k with k %% N != 0 may travel predicted from the decoded frame k - 1 "
                        "(format AUP1: motion search and residual on the device), chosen per frame against intra from the exact sizes; frame k "
                        "of n gets (upload bytes - spent) // (n - k).  1 = every frame intra.  <results>_uplink_kinds.npy: per upload second, "
                        "intra frames, inter frames, zero-length slices, all slices")
    p.add_argument("--uplink_bw", type=float, default=200.0,
                   help="--compress_uplink: the uplink's rate in kbit/s (extra flag; the reference reads an undefined flag of this name); an "
                        "upload of n frames gives each floor(uplink_bw * 1000 / 8 * upload period / n) bytes")
    p.add_argument("--no_restore", action="store_true")
    p.add_argument("--save_pic", action="store_true")
    p.add_argument("--gpu_ingest", action="store_true",
                   help="resize / BGR->RGB of frames and labels on the GPU (extra flag; reference: cv2 on the host)")
    p.add_argument("--enable_ASR", action="store_true")
    p.add_argument("--enable_ATR", action="store_true")
    p.add_argument("--train_strategy", default="full_model",
                   choices=["full_model", "coord_desc_auto", "coord_desc_last", "coord_desc_first", "coord_desc_both",
                            "coord_desc_rand"])
    p.add_argument("--coord_fraction", default="0.1", choices=["0.1", "0.05", "0.2", "0.01"])
    p.add_argument("--mode", **req, choices=["simple", "pretrained", "horizon", "early"])
    p.add_argument("--early_cutoff_time", type=int, default=60)
    # additions (not in the reference): make short synthetic runs possible
    p.add_argument("--length", type=int, default=None, help="override exp_configs.test_length (seconds)")
    p.add_argument("--first_train_time", type=int, default=None, help="override ceil(100/train_period)*train_period")
    p.add_argument("--edge_pipeline", type=int, default=1, choices=[1, 2, 3, 4],
                   help="edge: frames per inference pass (extra flag; 1 = the reference's synchronous per-frame call).  With n >= 2 the edge "
                        "holds n frames and labels them in ONE pass (a one-frame pass leaves most of the chip idle), while the previous pass's "
                        "results are being consumed; per-frame outputs are identical")
    p.add_argument("--sampling", default="reference", choices=["reference", "per_second"],
                   help="uplink sampling: 'reference' = run.py:115/175 (send_rate = send_period / fps is the fraction of the bucket "
                        "that is uploaded), 'per_second' = send_rate counts frames per second (fps / send_period)")
    p.add_argument("--edge_from_delta", action="store_true",
                   help="score the edge model the downlink payload produces (extra flag): the server also writes each event's raw payload "
                        "(<label>_<second>_delta.bin), and the edge keeps its network and applies that payload to the initial model "
                        "(--no_restore: to its previous model) on the device instead of reloading the server's full f32 model")
    p.add_argument("--delta_format", default="fp16", choices=["fp16", "q8"],
                   help="what the downlink payload carries behind its mask bits (extra flag): fp16 = the masked values as fp16 (the reference's "
                        "format), q8 = one f32 scale per variable and one int8 code per masked element of the CHANGE against the model both ends "
                        "hold (the initial model; with --no_restore the edge's previous model, which the server tracks).  _mask.dat, _mask.dat.gz, "
                        "_delta.bin and the downlink accounting carry the chosen format; --edge_from_delta decodes it")
    p.add_argument("--device_masks", action="store_true",
                   help="server: choose coord_desc_auto's coordinates, keep the masks and encode the downlink payload on the device (extra "
                        "flag; same files and numbers)")
    p.add_argument("--device_memory", action="store_true",
                   help="server: keep the replay memory on the device and sample mini-batches from it there (extra flag; needs a GPU; composes "
                        "with --gpu_ingest and --device_masks; same files and numbers)")
    p.add_argument("--device_render", action="store_true",
                   help="edge: paint the --save_pic views on the device right behind the inference pass and copy them to the host once per "
                        "written frame (extra flag; needs --save_pic and a GPU; composes with --gpu_ingest, --edge_pipeline and "
                        "--edge_from_delta; same files)")
    p.add_argument("--edge_confidence", action="store_true",
                   help="edge: also compute the student's own certainty (per-pixel softmax maximum) right behind every inference pass and log it "
                        "(extra flag; needs a GPU network): <results>_confidence.npy [frames, 3] = mean confidence, share of pixels below 0.5, "
                        "expected calibration error against the teacher; <results>_reliability.npy [frames, 3, 32] = valid pixels, hits and "
                        "summed confidence (x 2^20) per confidence bin; with --save_pic one grey confidence.png per pictured frame.  Every other "
                        "file is unchanged; composes with --gpu_ingest, --edge_pipeline, --edge_from_delta and --device_render")
    p.add_argument("--soft_teacher", action="store_true",
                   help="server: fine-tune against the teacher's distribution (extra flag; needs --device_memory): the source also serves each "
                        "sampled frame's teacher logits (a directory: logits_%%06d.npy beside the gt files, f32 [lh, lw, classes]; a synthetic "
                        "clip: a H/16+1 x W/16+1 grid), the replay memory caches the student's channels of that grid and the soft loss reads its "
                        "align-corners upsample.  Also writes <results>_soft_eval.npy: per training event the second, the soft loss over the "
                        "memory after the phase, the probabilistic mIoU and the K per-class values; every other file keeps its name and format")
    p.add_argument("--labels_from_logits", action="store_true",
                   help="server: derive the hard labels of the replay memory from the teacher logits on the device instead of resizing and "
                        "uploading the source's label map (extra flag; needs --soft_teacher; not for the experiments whose labels arrive in "
                        "COCO numbering).  The edge keeps scoring against the source's labels")
    p.add_argument("--kd_temperature", type=float, default=None,
                   help="server: temperature T of the soft-teacher loss (extra flag; needs --soft_teacher; finite and > 0, default 1): both logit "
                        "sets are divided by T and the soft term carries the factor T^2.  Evaluation (<results>_soft_eval.npy) keeps the T = 1 loss")
    p.add_argument("--kd_alpha", type=float, default=None,
                   help="server: weight of the soft term in the soft-teacher loss (extra flag; needs --soft_teacher; in [0, 1], default 1); the "
                        "hard-label cross-entropy takes 1 - kd_alpha")
    p.add_argument("--loss_class_weights", default=None,
                   help="server: per-class weights of the fine-tune loss with a weighted mean (extra flag): K comma-separated floats in the order "
                        "of the experiment's classes, each 0 or in [2^-6, 16], or 'balanced' = N / (P n_k) capped to that range, recomputed at the "
                        "start of every training phase from the labels then in the replay memory.  Also writes <results>_loss_weights.npy "
                        "[phases, K]; evaluation stays unweighted and every other file keeps its name and format")
    p.add_argument("--kd_conf_gamma", type=float, default=None,
                   help="server: weight every pixel of the soft-teacher loss by the teacher's confidence (largest target probability) to this power "
                        "(extra flag; needs --soft_teacher; in [0, 8], default 0)")
    p.add_argument("--loss_top_k", type=float, default=None,
                   help="server: hard-pixel mining (extra flag; DeepLab's top_k_percent_pixels): every fine-tune step takes its loss over the hardest "
                        "fraction F in (0, 1] of the valid pixels, chosen on the device.  Also writes <results>_mining.npy, one row (threshold, kept, "
                        "valid) per training event from the phase's last iteration; evaluation stays unmined and every other file keeps its name")
    p.add_argument("--loss_top_k_warmup", type=int, default=None,
                   help="server: ease the mining in over the first N iterations of every phase (extra flag; needs --loss_top_k < 1; DeepLab's "
                        "hard_example_mining_step): iteration it keeps min(1, it / N) F + (1 - min(1, it / N)), so iteration 0 is unmined")
    p.add_argument("--horizon_k1s",default="16,32,64,128,256,512", help="horizon mode: training-window lengths in seconds (reference: hard-coded)")
    p.add_argument("--horizon_k2", type=int, default=256, help="horizon mode: evaluation window in seconds (reference: 256)")
    p.add_argument("--horizon_points", type=int, default=3, help="horizon mode: number of evaluation points (reference: 3)")
    return p


# ----------------------------------------------------------------------------------------------------------- video
class FrameSource:
    """fps, number of frames, and (RGB uint8 frame, uint8 teacher label) by absolute frame index."""
    fps: int

    def __len__(self) -> int:  # pragma: no cover
        raise NotImplementedError

    def read(self, i: int) -> Tuple[np.ndarray, np.ndarray]:  # pragma: no cover
        raise NotImplementedError

    def read_logits(self, i: int) -> Optional[np.ndarray]:
        """The teacher's logits for frame ``i``, f32 [lh, lw, classes] on the teacher's own grid, or None where the source has none."""
        return None


class SyntheticSource(FrameSource):
    def __init__(self, exp_num: int, height: int, seconds: int, fps: int):
        self.fps = fps
        cw = class_weights(exp_num)
        self.video = SyntheticVideo(height, seconds * fps, np.where(cw.reshape(-1) == 1)[0], num_classes=cw.shape[0], seed=exp_num)
        self.n = seconds * fps

    def __len__(self):
        return self.n

    def read(self, i):
        return self.video.frame(i)

    def read_logits(self, i):
        return self.video.teacher_logits(i, self.video.h // 16 + 1, self.video.w // 16 + 1)          # the grid of an output-stride-16 teacher


class DirectorySource(FrameSource):
    def __init__(self, frames_dir: str, gt_dir: str, fps: int = 30):
        self.frames_dir, self.gt_dir, self.fps = frames_dir, gt_dir or frames_dir, fps
        self.n = len([f for f in os.listdir(frames_dir) if f.startswith("frame_") and f.endswith(".npy")])

    def __len__(self):
        return self.n

    def read(self, i):
        return (np.load(os.path.join(self.frames_dir, "frame_%06d.npy" % i)),
                np.load(os.path.join(self.gt_dir, "gt_%06d.npy" % i)))

    def read_logits(self, i):
        path = os.path.join(self.gt_dir, "logits_%06d.npy" % i)
        return np.load(path).astype(np.float32, copy=False) if os.path.exists(path) else None


def video_number(spec: str) -> int:
    """The experiment number an --input_video names: synthetic:<NUM>-<name>... or a directory <NUM>-<name>."""
    if spec.startswith("synthetic:"):
        return int(spec.split(":")[1].split("-")[0])
    return int(os.path.basename(spec.rstrip("/")).split("-")[0])


def source_logits(source: FrameSource, i: int) -> np.ndarray:
    """--soft_teacher: frame ``i``'s teacher logits, or an error that names what is missing."""
    logits = source.read_logits(i)
    if logits is None:
        missing = os.path.join(source.gt_dir, "logits_%06d.npy" % i) if isinstance(source, DirectorySource) else "read_logits(%d)" % i
        raise FileNotFoundError("--soft_teacher needs the teacher logits of every sampled frame: %s is missing (f32 [lh, lw, classes], the "
                                "teacher's own output grid, beside the gt_%%06d.npy files)" % missing)
    return logits


def open_source(flags) -> Tuple[FrameSource, int]:
    spec = flags.input_video
    if spec.startswith("synthetic:"):
        parts = spec.split(":")
        vid_num = video_number(spec)
        opts = dict(kv.split("=") for kv in parts[2:])
        seconds = int(opts.get("seconds", flags.length or test_length(vid_num)))
        return SyntheticSource(vid_num, flags.height, seconds, int(opts.get("fps", 30))), vid_num
    return DirectorySource(spec, flags.gt_video), video_number(spec)


def _frame_to_size(frame: np.ndarray, size: List[int], ingest=None):
    """The frame half of ``_to_size``."""
    if frame.shape[:2] != (size[0], size[1]):
        frame = ingest.frame(frame, size[0], size[1]) if ingest is not None else resize_linear(frame, size[1], size[0])
    return frame


def _to_size(frame: np.ndarray, label: np.ndarray, size: List[int], ingest=None):
    """cv2.resize(frame, (2H, H)) [bilinear] and cv2.resize(label, ..., INTER_NEAREST) (run.py:179-183, :415-421).

    ``ingest`` (an ``ams_amd.ingest.FrameIngest``, flag ``--gpu_ingest``) does both on the device: the raw uint8 frame is
    what crosses PCIe and the results stay there (``SemanticNetwork`` takes device tensors); frames that already have the
    network's size pass through untouched either way."""
    frame = _frame_to_size(frame, size, ingest)
    if label.shape[:2] != (size[0], size[1]):
        label = ingest.label(label, size[0], size[1]) if ingest is not None else resize_nearest(label, size[1], size[0])
    return frame, label


def uplink_budget(uplink_bw: float, period: int, n: int) -> int:
    """--compress_uplink: the bytes each of the ``n`` frames of an upload may take, ``period`` seconds after the previous upload."""
    return int(uplink_bw * 1000 / 8 * period // n)


def uplink_upload_bytes(uplink_bw: float, period: int) -> int:
    """--uplink_gop > 1: the bytes of one upload, ``period`` seconds after the previous one; frame k of n gets (these - spent) // (n - k)."""
    return int(uplink_bw * 1000 / 8 * period)


def _through_uplink(fr, codec, budget: int, size: List[int], ingest=None, chain=None):
    """--compress_uplink: the sampled frame as the server receives it.  Resized to twice the network size, encoded at the budget and decoded on
    the device, resized to the network size by the same rule (both on the device with ``ingest``, else ``resize_linear`` on the host)
    -> (frame, payload bytes, quality, fits).

    ``chain`` (--uplink_gop > 1) is the upload's state: under "reference" the decoded frame in front of this one, or None where this frame
    must be intra; the call offers it to the encoder, leaves its own decoded frame there and appends (kind, zero-length slices, slices)
    to "frames"."""
    H2, W2 = 2 * size[0], 2 * size[1]
    if fr.shape[:2] != (H2, W2):
        fr = ingest.frame(fr, H2, W2) if ingest is not None else resize_linear(_host(fr), W2, H2)
    if chain is not None:
        from .uplink import INTER, kind_of, table_lengths
        reference = chain["reference"]
        payload, quality, fits = codec.encode_to_budget(fr, budget, reference=reference)
        kind = kind_of(payload)
        decoded = codec.decode(payload, reference=reference) if kind == INTER else codec.decode(payload, (H2, W2))
        lens = table_lengths(payload, H2, W2)
        chain["reference"] = decoded
        chain["frames"].append((kind, int((lens == 0).sum()), len(lens)))
        fr = ingest.frame(decoded, size[0], size[1]) if ingest is not None else resize_linear(_host(decoded), size[1], size[0])
        return fr, int(payload.numel()), quality, fits
    payload, quality, fits = codec.encode_to_budget(fr, budget)
    decoded = codec.decode(payload, (H2, W2))
    fr = ingest.frame(decoded, size[0], size[1]) if ingest is not None else resize_linear(_host(decoded), size[1], size[0])
    return fr, int(payload.numel()), quality, fits


def _batch1(x):
    """np.expand_dims(x, 0) for host arrays and device tensors alike."""
    return x.unsqueeze(0) if hasattr(x, "unsqueeze") else np.expand_dims(x, axis=0)


def _host(x) -> np.ndarray:
    return x.cpu().numpy() if hasattr(x, "cpu") else x


class Context:
    def __init__(self, flags, network_cls=None):
        self.flags = flags
        # the class behind the SemanticNetwork boundary: the HIP-backed one unless a caller injects another with the same
        # surface (tests/golden/make_scheduler_fixture.py pins this loop with a CPU stand-in)
        self.network_cls = network_cls or SemanticNetwork
        self.size = [flags.height, flags.height * 2]
        self.source, self.vid_num = open_source(flags)
        self.length = flags.length or (len(self.source) // self.source.fps)
        self.ingest = None
        if getattr(flags, "gpu_ingest", False):
            from .ingest import FrameIngest
            self.ingest = FrameIngest("cuda:%s" % flags.gpu)
        ck = flags.student_checkpoint
        self.initial_variables = None
        if ck.startswith("synthetic"):
            from .spec import build_spec
            from .weights import synthetic_weights
            seed = int(ck.split(":")[1]) if ":" in ck else 0
            self.initial_variables = synthetic_weights(build_spec(class_weights(self.vid_num).shape[0]), seed)

    def save_dir(self, prepend: str) -> str:
        video = self.flags.input_video.replace(":", "_").split("/")[-1]
        ck = self.flags.student_checkpoint.replace(":", "_").split("/")
        return os.path.join(self.flags.output_dir, "%s_%s_%s_%d" % (prepend, video, ck[-2] if len(ck) > 1 else ck[-1],
                                                                    self.flags.height))


PICTURES = ("cross_mask", "ignore_mask", "overlay_teacher", "output_teacher", "output_student", "overlay_student", "frame", "label_student")


def write_pictures(prefix: str, semantic_network, frame, gt_frame, label_student, views=None) -> None:
    """The eight files of reference run.py:443-454 under ``prefix`` (RGB in the file, as cv2.imwrite leaves it after RGB2BGR).  ``views``: host
    arrays [1,H,W,3] by view name, painted on the device (--device_render); None: the host helpers paint."""
    frame, gt_frame = _host(frame), _host(gt_frame)
    if views is not None:
        v = {k: a[0] for k, a in views.items()}
        cross_mask, ignore_mask = v["cross_mask"], v["ignore_mask"]
        output_teacher, overlay_teacher = v["colour_teacher"], v["overlay_teacher"]
        output_student, overlay_student = v["colour_student"], v["overlay_student"]
    else:
        # cross_ignore indexes its take table with the teacher ids and raises on one from the class count on (255 = unlabelled): such a pixel
        # is ignored (white / black), as the metric and the device path count it; the helper sees a valid id there and its answer is replaced
        known = gt_frame < len(semantic_network.take_array)
        cross_mask, ignore_mask = semantic_network.cross_ignore(label_teacher=np.where(known, gt_frame, 0), label_student=label_student)
        ignore_mask[~known] = 255
        cross_mask[~known] = 0
        output_teacher, overlay_teacher = semantic_network.colorize_teacher(label=gt_frame, frame=frame)
        output_student, overlay_student = semantic_network.colorize(label=label_student, frame=frame)
    images = (cross_mask, ignore_mask, overlay_teacher, output_teacher, output_student, overlay_student, frame,
              np.asarray(label_student).astype(np.uint8))
    for name, image in zip(PICTURES, images):
        png.write(prefix + name + ".png", image)


def print_process(str_log, curr_time):
    print("Process [current time: %d]: " % curr_time, str_log)


# ----------------------------------------------------------------------------------------------------------- server
def train_model(ctx: Context, train_start, train_end, sampling_period, gpu_id, run_label, gt_path, exp_num, save_range,
                sample_send_period):
    """Server side: collect sampled frames in [train_start, train_end), fine-tune at the times in save_range and publish
    a frozen model after each (reference run.py:78-361)."""
    FLAGS = ctx.flags
    assert train_end - train_start != 0, "There should be at least one set of data points"
    uplink_codec = None
    if getattr(FLAGS, "compress_uplink", False):
        from .uplink import UplinkCodec
        uplink_codec = UplinkCodec("cuda:%s" % gpu_id)
    uplink_log = []           # --compress_uplink, per upload: (second, frames, bytes, budget per frame, min q, mean q, frames that did not fit)
    uplink_gop = getattr(FLAGS, "uplink_gop", 1)
    uplink_kinds = []         # --uplink_gop > 1, per upload: (second, intra frames, inter frames, zero-length slices, all slices)
    save_range = list(save_range)
    fps = ctx.source.fps
    train_end_frame = min(train_end * fps, len(ctx.source))
    i = train_start * fps
    update_count = 0
    per_second = getattr(FLAGS, "sampling", "reference") == "per_second"
    if per_second:
        send_rate = min(float(fps), fps / float(sampling_period))  # frames per second uploaded (module docstring)
        if FLAGS.enable_ASR:
            send_rate = float(np.clip(send_rate, 0.1, 1))          # start inside ASR's range: its first update must not jump
    else:
        send_rate = sampling_period / fps                          # reference run.py:115: the fraction of the bucket
    sample_per_period, up_bw_per_period, down_bw_per_period = [], [], []
    frame_label_bucket = []
    num_unseen_frames = 0
    model_save_times = [0]
    train_period_reset = train_period_current = (save_range[2] - save_range[1]) if len(save_range) > 2 else FLAGS.train_period
    send_rate_deq = deque(maxlen=5)
    hibernate = False
    map_coco = coco_class_converter() if is_coco(exp_num) else None
    mem = max(1, int(FLAGS.memory_len / sampling_period * fps))
    frame_memory, label_memory = deque(maxlen=mem), deque(maxlen=mem)
    device_memory = None
    soft_teacher = bool(getattr(FLAGS, "soft_teacher", False))
    labels_from_logits = bool(getattr(FLAGS, "labels_from_logits", False))
    assert not soft_teacher or getattr(FLAGS, "device_memory", False), "--soft_teacher needs --device_memory"
    assert not labels_from_logits or (soft_teacher and map_coco is None), "--labels_from_logits needs --soft_teacher and labels in the logits' numbering"
    if getattr(FLAGS, "device_memory", False):
        from .replay import DeviceReplayMemory
        memory_kw = {}
        if soft_teacher:
            # the teacher's grid as the first frame's logits give it; a slot keeps the student's channels of it, and the grid stands for its
            # align-corners upsample to the frame size wherever a batch is resampled
            cw = class_weights(exp_num)
            lh, lw, nc = source_logits(ctx.source, i).shape
            assert nc == cw.shape[0], "teacher logits of %d classes for experiment %d, which has %d" % (nc, exp_num, cw.shape[0])
            memory_kw = dict(logits_shape=(lh, lw, nc), logits_upsample=True, logits_select=np.where(cw.reshape(-1) == 1)[0].tolist())
        device_memory = DeviceReplayMemory(mem, ctx.size[0], ctx.size[1], "cuda:%s" % gpu_id, **memory_kw)

    # --loss_class_weights: K fixed weights, or 'balanced' = recomputed per phase from the memory's labels (the scene changes)
    weights_flag = getattr(FLAGS, "loss_class_weights", None)
    balanced = weights_flag == "balanced"
    fixed_weights = None if weights_flag is None or balanced else parse_loss_class_weights(weights_flag, int(class_weights(exp_num).sum()))
    conf_gamma = float(getattr(FLAGS, "kd_conf_gamma", None) or 0.0)
    loss_weights_log = []     # --loss_class_weights, per training phase: the K weights it ran under
    mining_flag = getattr(FLAGS, "loss_top_k", None)
    mining_log = []           # --loss_top_k, per training phase: (threshold, kept, valid) of its last iteration
    semantic_network = ctx.network_cls(meta_dir=FLAGS.student_checkpoint, class_weights_exp=class_weights(exp_num),
                                       height=FLAGS.height, gpu_id=gpu_id, scale=[1], mini_batch_size=FLAGS.batch_size,
                                       lr=FLAGS.lr, mem_frac=1, coord_frac=float(FLAGS.coord_fraction),
                                       train_biases_only=False, regularize=False,
                                       masked_gradients=FLAGS.train_strategy not in ['full_model'],
                                       cross_miou_compat=FLAGS.enable_ASR, initial_variables=ctx.initial_variables,
                                       **({"device_masks": True} if getattr(FLAGS, "device_masks", False) else {}),
                                       **({"soft_teacher": True} if soft_teacher else {}),
                                       **{k: float(getattr(FLAGS, k)) for k in ("kd_temperature", "kd_alpha", "kd_conf_gamma")
                                          if getattr(FLAGS, k, None) is not None},
                                       **({"loss_class_weights": fixed_weights} if fixed_weights is not None else {}),
                                       **{k: getattr(FLAGS, k) for k in ("loss_top_k", "loss_top_k_warmup") if getattr(FLAGS, k, None) is not None})
    save_dir = ctx.save_dir(run_label + "_%d" % train_start)
    semantic_network.save_to_frozen_graph(save_dir + "_final")
    print_process("Saved model to %s_final.pb" % save_dir, 0)
    train_ms = []
    control_log = []          # per training event: (second, mean phi-score or nan, send_rate, train_period_current, hibernating)
    soft_eval = []            # --soft_teacher, per training event: (second, soft loss, probabilistic mIoU, its K per-class values)

    while i < train_end_frame:
        frame, gt = ctx.source.read(i)
        # --soft_teacher: a bucketed label carries its frame index, so that only the frames choose_frames picks have their logits read
        frame_label_bucket.append((frame, (gt, i)) if soft_teacher else (frame, gt))
        i += 1
        if i % fps != 0:
            continue                                   # events are evaluated once per elapsed second
        second = i // fps
        if second % (5) == 0:
            print_process("%d seconds elapsed" % second, second)

        if second % sample_send_period == 0:
            frames_chosen, labels_chosen = choose_frames(frame_label_bucket, min(1.0, send_rate / fps if per_second else send_rate))
            size_images = 0.0
            budget = uplink_budget(FLAGS.uplink_bw, sample_send_period, len(frames_chosen)) if uplink_codec is not None and frames_chosen else 0
            sent = []         # --compress_uplink: (bytes, quality, fits) per frame of this upload
            # --uplink_gop N > 1: within this upload frame k with k % N != 0 is offered the decoded frame k - 1; no reference crosses uploads
            chain = dict(reference=None, frames=[]) if uplink_codec is not None and uplink_gop > 1 else None
            upload_bytes = uplink_upload_bytes(FLAGS.uplink_bw, sample_send_period) if chain is not None else 0
            for k, (fr, label) in enumerate(zip(frames_chosen, labels_chosen)):
                logits = None
                if soft_teacher:
                    label, index = label
                    logits = source_logits(ctx.source, index)
                if chain is not None:
                    if k % uplink_gop == 0:
                        chain["reference"] = None
                    # what prediction saved so far goes to the frames that follow
                    fr, *info = _through_uplink(fr, uplink_codec, (upload_bytes - sum(n for n, _, _ in sent)) // (len(frames_chosen) - k), ctx.size,
                                                ctx.ingest, chain)
                    sent.append(info)
                elif uplink_codec is not None:
                    # the frame goes through the lossy leg before anything else sees it; its label does not travel (the teacher is the server's)
                    fr, *info = _through_uplink(fr, uplink_codec, budget, ctx.size, ctx.ingest)
                    sent.append(info)
                if labels_from_logits:
                    # the server never touches the source's label map: no resize, no upload; the slot's labels are the argmax of the
                    # logits' upsample, formed on the device
                    fr, label_resized = _frame_to_size(fr, ctx.size, ctx.ingest), None
                else:
                    fr, label_resized = _to_size(fr, label, ctx.size, ctx.ingest)
                if device_memory is not None:
                    # the replay memory lives on the device: what --gpu_ingest produced there stays there; the host copy of the frame below
                    # is emulation accounting only
                    if map_coco is not None:
                        label_resized = map_coco[_host(label_resized)]
                    device_memory.append(fr, label_resized, logits)
                    fr = _host(fr)
                else:
                    fr, label_resized = _host(fr), _host(label_resized)       # the replay memory lives on the host
                    if map_coco is not None:
                        label_resized = map_coco[label_resized]
                    frame_memory.append(fr)
                    label_memory.append(label_resized)
                if uplink_codec is not None:
                    size_images += sent[-1][0] / 1024                         # the payload that travelled
                else:
                    size_images += len(zlib.compress(fr.tobytes(), 6)) / 1024     # stand-in for the PNG size
            frame_label_bucket.clear()
            sample_per_period.append(len(frames_chosen))
            num_unseen_frames += len(frames_chosen)
            up_bw_per_period.append(size_images * 8)
            if uplink_codec is not None:
                qs = [q for _, q, _ in sent]
                uplink_log.append((second, len(sent), sum(n for n, _, _ in sent), budget, min(qs) if qs else np.nan,
                                   float(np.mean(qs)) if qs else np.nan, sum(1 for _, _, fits in sent if not fits)))
            if chain is not None:
                inter = sum(1 for kind, _, _ in chain["frames"] if kind == "AUP1")
                uplink_kinds.append((second, len(chain["frames"]) - inter, inter, sum(z for _, z, _ in chain["frames"]),
                                     sum(n for _, _, n in chain["frames"])))

        n_memory = len(device_memory) if device_memory is not None else len(frame_memory)
        if second in save_range and n_memory == 0:
            # nothing has been uploaded yet (e.g. a horizon window shorter than the upload period): the model of this event
            # time is the current one, published unchanged
            print_process("No samples in memory at %d s: publishing the current model unchanged" % second, second)
            save_dir = ctx.save_dir(run_label + "_%d" % second)
            semantic_network.save_to_frozen_graph(save_dir + "_final")
            model_save_times.append(float(second))
        elif second in save_range:
            phi = float("nan")
            if FLAGS.enable_ASR and n_memory > 1:
                # phi-score over the frames that arrived since the last update -> sampling rate (run.py:279-290)
                i_start = max(0, n_memory - num_unseen_frames - 1)
                if device_memory is not None:
                    cross = [r[2] for r in device_memory.cross_miou_pairs(semantic_network, i_start)]       # one launch, one copy
                else:
                    cross = [semantic_network.calc_cross_miou(np.array([label_memory[k], label_memory[k + 1]]))[2]
                             for k in range(i_start, len(label_memory) - 1)]
                if cross:
                    phi = float(np.mean(cross))
                    send_rate = float(np.clip(send_rate - 0.2 * np.tanh((np.mean(cross) - 0.6) * 20), 0.1, 1))
                    send_rate_deq.append(send_rate)
                    print_process("Send rate updated to %.2f" % send_rate, second)
                num_unseen_frames = 0
            if FLAGS.enable_ATR and len(send_rate_deq) > 0:
                if np.mean(list(send_rate_deq)) < 0.25:
                    hibernate = True
                if np.mean(list(send_rate_deq)) > 0.35 and hibernate:
                    hibernate = False
                    train_period_current = train_period_reset
                if hibernate:
                    train_period_current = min(train_period_current + 2, 6 * train_period_reset)
                idx = save_range.index(second)
                save_range = save_range[:idx] + list(range(second, train_end, train_period_current))
            control_log.append((second, phi, send_rate, train_period_current, int(hibernate)))

            if not FLAGS.no_restore:
                semantic_network.restore_initial()
            if balanced:
                # the same integer histogram on either memory, so the same weights bit for bit
                counts = device_memory.class_counts(semantic_network) if device_memory is not None \
                    else label_class_counts(label_memory, semantic_network.class_indices_graph)
                semantic_network.set_loss_weights(balanced_class_weights(counts), conf_gamma)
            if weights_flag is not None:
                loss_weights_log.append(np.asarray(semantic_network.loss_class_weights, dtype=np.float32))
            t1 = time.time()
            if device_memory is not None:
                semantic_network.train_with_deque(device_memory, None, FLAGS.iter, FLAGS.train_strategy)
            else:
                semantic_network.train_with_deque(frame_memory, label_memory, FLAGS.iter, FLAGS.train_strategy)
            train_ms.append(1000 * (time.time() - t1))
            print("Training for %d iterations took %d ms!!!" % (FLAGS.iter, train_ms[-1]))
            if mining_flag is not None:
                m = getattr(semantic_network, "last_mining", None)        # None: the phase's last iteration was unmined (a warm-up not yet over)
                mining_log.append((m["threshold"], m["kept"], m["valid"]) if m else (np.nan, np.nan, np.nan))
            if soft_teacher:
                # what the phase left: the soft loss and the probabilistic IoU of the model about to be published, over the whole memory
                metric, _conf = semantic_network.evaluate_memory(device_memory)
                soft_eval.append([float(second), metric.loss_soft, metric.soft_miou] + [float(v) for v in metric.soft_iou])
                print_process("Soft-teacher loss over the memory %.4f, probabilistic mIoU %.1f%%" % (metric.loss_soft, 100 * metric.soft_miou), second)
            # model delta on the downlink: packed mask bits + masked parameters as fp16, gzip -9 (run.py:316-336)
            if getattr(FLAGS, "delta_format", "fp16") == "q8":  # int8 codes of the change; continual training follows the edge's model
                payload = semantic_network.delta_payload(fmt="q8", track_edge=bool(FLAGS.no_restore))
            else:
                payload = semantic_network.delta_payload()      # value part gathered + cast to fp16 on the device
            if getattr(FLAGS, "device_masks", False):          # the same number from the layout: curr_mask stays on the device
                full_size = delta_layout(semantic_network.engine.spec, FLAGS.train_strategy).n_elements
            else:
                full_size = sum(val.size for val in semantic_network.curr_mask)
            with open(save_dir + '_mask.dat', 'wb') as f:
                f.write(payload)
            with gzip.open(save_dir + '_mask.dat.gz', 'wb', compresslevel=9) as f:
                f.write(payload)
            if getattr(FLAGS, "edge_from_delta", False):
                # _mask.dat above carries the PREVIOUS event's label (as in the reference): the edge finds this event's payload by its own time
                with open(ctx.save_dir(run_label + "_%d" % second) + "_delta.bin", 'wb') as f:
                    f.write(payload)
            curr_update = os.path.getsize(save_dir + '_mask.dat.gz') * 8
            down_bw_per_period.append(curr_update)
            update_count += 1
            print("Full size of model is %d; update is %.1f Kbit" % (full_size, curr_update / 1024))
            save_dir = ctx.save_dir(run_label + "_%d" % second)
            semantic_network.save_to_frozen_graph(save_dir + "_final")
            print_process("Saved model to %s_final.pb" % save_dir, second)
            model_save_times.append(float(second))

    semantic_network.close_model()
    final_save_dir = ctx.save_dir(run_label + "_results")
    np.save(final_save_dir + '_fps_client.npy', sample_per_period)
    np.save(final_save_dir + '_bw_uplink.npy', up_bw_per_period)
    np.save(final_save_dir + '_bw_downlink.npy', down_bw_per_period)
    np.save(final_save_dir + '_model_update_times.npy', model_save_times)
    np.save(final_save_dir + '_train_ms.npy', train_ms)
    np.save(final_save_dir + '_control.npy', np.asarray(control_log, dtype=np.float64).reshape(-1, 5))
    if uplink_codec is not None:
        np.save(final_save_dir + '_uplink_quality.npy', np.asarray(uplink_log, dtype=np.float64).reshape(-1, 7))
        if uplink_gop > 1:
            np.save(final_save_dir + '_uplink_kinds.npy', np.asarray(uplink_kinds, dtype=np.float64).reshape(-1, 5))
    if weights_flag is not None:
        np.save(final_save_dir + '_loss_weights.npy', np.asarray(loss_weights_log, dtype=np.float32).reshape(-1, int(class_weights(exp_num).sum())))
    if mining_flag is not None:
        np.save(final_save_dir + '_mining.npy', np.asarray(mining_log, dtype=np.float64).reshape(-1, 3))
    if soft_teacher:
        k = int(class_weights(exp_num).sum())
        np.save(final_save_dir + '_soft_eval.npy', np.asarray(soft_eval, dtype=np.float64).reshape(-1, 3 + k))
    with open(final_save_dir + '_update.txt', 'w') as f:
        f.write("%d\n%d\n%d\n%d\n%d" % (sum(down_bw_per_period), sum(up_bw_per_period), update_count,
                                        train_end - train_start, sum(sample_per_period)))
    return model_save_times


# ----------------------------------------------------------------------------------------------------------- edge
def infer_output(ctx: Context, inf_start, inf_end, gpu_id, run_label, gt_path, exp_num, load_range):
    """Edge side: label every frame in [inf_start, inf_end) with the newest published model (run.py:364-461)."""
    FLAGS = ctx.flags
    assert inf_end - inf_start != 0, "There should be at least one set of data points"
    fps = ctx.source.fps
    inf_end_frame = min(inf_end * fps, len(ctx.source))
    i = inf_start * fps
    semantic_network = None
    confusion_matrix_memory = deque(maxlen=10 * fps)
    loss_s, miou_cats, miou_s, miou_mem_s = [], [], [], []
    final_save_dir = ctx.save_dir(run_label + "_results")
    load_times = set(float(t) for t in load_range)
    t_infer = 0.0
    depth = int(getattr(FLAGS, "edge_pipeline", 1))
    in_flight = deque()               # tickets of submitted frames (depth >= 2), oldest first
    from_delta = bool(getattr(FLAGS, "edge_from_delta", False))
    base_variables = None             # --edge_from_delta: the model the edge loaded first (what the server restores before each event)
    update_s = []                     # --edge_from_delta: host wall time of each edge update (payload in -> model re-frozen)
    save_pic = bool(getattr(FLAGS, "save_pic", False))
    device_render = bool(getattr(FLAGS, "device_render", False))
    views = None
    if device_render:
        from .render import VIEWS as views
    edge_confidence = bool(getattr(FLAGS, "edge_confidence", False))
    conf_rows, reliability = [], []   # --edge_confidence: per frame (mean, low_fraction(0.5), ECE) and (hist_valid, hist_hit, bin_sum)
    held = {}                         # --save_pic, depth >= 2: ticket -> (advanced frame index, frame, label) of the frames that get pictures

    def pictured(i_next):
        """--save_pic: does the frame after which ``i`` became ``i_next`` keep its files?  (the last frame of each label ``i_next // fps``)"""
        return save_pic and ((i_next + 1) % fps == 0 or i_next == inf_end_frame)

    def pictures(i_next, frame, gt_frame, result, rendered, confidence=None):
        write_pictures(final_save_dir + "_%d_" % (i_next // fps), semantic_network, frame, gt_frame, result[0][0],
                       rendered.host() if rendered is not None else None)
        if confidence is not None:                     # after the reference's eight: the certainty map, grey (255 = sure)
            png.write(final_save_dir + "_%d_confidence.png" % (i_next // fps), confidence.host()[0])

    def log_confidence(confidence):
        st = confidence.stats[0]
        conf_rows.append((st.mean, st.low_fraction(0.5), st.ece))
        reliability.append(np.stack([st.hist_valid, st.hist_hit, st.bin_sum]))

    def predict_with_extras(frame, gt_frame, want_views):
        """One synchronous pass with the views and / or the confidence behind it: (predict_with_metric's 5-tuple, views or None, confidence or None)."""
        if want_views:
            out = semantic_network.predict_rendered(_batch1(frame), _batch1(gt_frame), views, confidence=edge_confidence)
            return out[:5], out[5], out[6] if edge_confidence else None
        out = semantic_network.predict_with_confidence(_batch1(frame), _batch1(gt_frame))
        return out[:5], None, out[5]

    def collect(ticket):
        res = semantic_network.collect(ticket)
        confidence = None
        if edge_confidence:
            confidence = semantic_network.take_confidence(ticket)
            log_confidence(confidence)
        if ticket in held:
            pictures(*held.pop(ticket), res, semantic_network.take_rendered(ticket) if device_render else None, confidence)
        return res

    def record(result, n_done):
        _labels, conf_mat_, _, miou_, loss_ = result
        loss_s.append(loss_)
        miou_cats.append(np.array(conf_mat_))
        miou_s.append(miou_)
        confusion_matrix_memory.append(conf_mat_)
        miou_mem_s.append(np.nanmean(calculate_miou(np.sum(list(confusion_matrix_memory), axis=0), nan=True)))
        if n_done % fps == 0:
            miou = np.nanmean(calculate_miou(np.sum(miou_cats[-fps:], axis=0), nan=True))
            print_process("miou at %03d secs: %.1f%%" % (n_done / fps, float(miou) * 100), n_done / fps)

    done = inf_start * fps
    while i < inf_end_frame:
        if i / fps in load_times:
            while in_flight:                           # the frames still in flight belong to the model that is about to be replaced
                t0 = time.time()
                res = collect(in_flight.popleft())
                t_infer += time.time() - t0
                done += 1
                record(res, done)
            save_dir = ctx.save_dir(run_label + "_%d" % (i // fps))
            if from_delta and semantic_network is not None:
                # the edge keeps its network and applies what the downlink carried; an event that published the current model unchanged
                # (empty replay memory) sent no payload, and the edge keeps its model
                if os.path.exists(save_dir + "_delta.bin"):
                    with open(save_dir + "_delta.bin", "rb") as f:
                        payload = f.read()
                    t0 = time.time()
                    semantic_network.apply_delta(payload, FLAGS.train_strategy, None if FLAGS.no_restore else base_variables,
                                                 **({"fmt": "q8"} if getattr(FLAGS, "delta_format", "fp16") == "q8" else {}))
                    update_s.append(time.time() - t0)
            else:
                if semantic_network is not None:
                    semantic_network.close_model()
                kw = {"pipeline_depth": depth} if depth > 1 else {}
                if from_delta:
                    with open(save_dir + "_final.pb", "rb") as f:
                        kw["frozen_graph"] = FrozenGraph.ParseFromString(f.read())
                    base_variables = kw["frozen_graph"].variables
                semantic_network = ctx.network_cls(meta_dir=save_dir + "_final", class_weights_exp=class_weights(exp_num),
                                                   height=FLAGS.height, gpu_id=gpu_id, mem_frac=1, frozen=True, **kw)
        frame, gt_frame = _to_size(*ctx.source.read(i), ctx.size, ctx.ingest)
        t0 = time.time()
        rendered = confidence = None
        if depth > 1:
            more_kw = {"confidence": True} if edge_confidence else {}
            if pictured(i + 1):
                render_kw = {"render": views} if device_render else {}
                in_flight.append(semantic_network.predict_with_metric_async(_batch1(frame), _batch1(gt_frame), **render_kw, **more_kw))
                held[in_flight[-1]] = (i + 1, frame, gt_frame)
            else:
                in_flight.append(semantic_network.predict_with_metric_async(_batch1(frame), _batch1(gt_frame), **more_kw))
            # up to two passes of `depth` frames in flight: the one on the GPU and the one being filled
            res = collect(in_flight.popleft()) if len(in_flight) >= 2 * depth else None
        elif edge_confidence or (device_render and pictured(i + 1)):
            res, rendered, confidence = predict_with_extras(frame, gt_frame, device_render and pictured(i + 1))
        else:                                          # the reference's surface: all a CPU stand-in has
            res = semantic_network.predict_with_metric(_batch1(frame), _batch1(gt_frame))
        t_infer += time.time() - t0
        i += 1
        if confidence is not None:
            log_confidence(confidence)
        if depth == 1 and pictured(i):
            pictures(i, frame, gt_frame, res, rendered, confidence)
        if res is not None:
            done += 1
            record(res, done)
    while in_flight:
        t0 = time.time()
        res = collect(in_flight.popleft())
        t_infer += time.time() - t0
        done += 1
        record(res, done)
    np.save('%s_loss.npy' % final_save_dir, loss_s)
    np.save('%s_mioucats.npy' % final_save_dir, miou_cats)
    np.save('%s_mious.npy' % final_save_dir, miou_s)
    np.save('%s_mioumems.npy' % final_save_dir, miou_mem_s)
    if edge_confidence:
        np.save('%s_confidence.npy' % final_save_dir, np.asarray(conf_rows, dtype=np.float64).reshape(-1, 3))
        np.save('%s_reliability.npy' % final_save_dir, np.asarray(reliability, dtype=np.int64).reshape(-1, 3, CONFIDENCE_BINS))
    if semantic_network is not None:
        semantic_network.close_model()
    n = max(1, inf_end_frame - inf_start * fps)
    summary = {"frames": n, "frames_per_sec": n / max(t_infer, 1e-9), "mean_miou": float(np.nanmean(miou_s)),
               "delta_format": getattr(FLAGS, "delta_format", "fp16")}
    if from_delta:
        summary["edge_updates"] = len(update_s)
        summary["edge_update_ms"] = 1000.0 * float(np.mean(update_s)) if update_s else float("nan")
        print_process("%d edge updates from the downlink payload, %.2f ms each (mean host wall time)"
                      % (summary["edge_updates"], summary["edge_update_ms"]), inf_end / 1.0)
    return summary


def event_times(flags, length: int) -> List[int]:
    """[0] + first training at ceil(100/train_period)*train_period, then every train_period (run.py:594-598)."""
    first = flags.first_train_time if flags.first_train_time is not None else int(np.ceil(100 / flags.train_period) * flags.train_period)
    return [0] + [t for t in range(first, length, flags.train_period)
                  if t == 0 or t >= flags.memory_len or not flags.initial_fill]


def parse_loss_class_weights(text: str, k: int) -> np.ndarray:
    """--loss_class_weights as K comma-separated floats: f32 [K], or a ValueError that names what is wrong."""
    try:
        cw = np.asarray([float(t) for t in text.split(",")], dtype=np.float32)
    except ValueError:
        raise ValueError("--loss_class_weights must be 'balanced' or %d comma-separated floats (got %r)" % (k, text))
    problem = loss_knobs_problem(True, loss_class_weights=cw, class_count=k, dash="--")
    if problem:
        raise ValueError(problem)
    return cw


def parse_flags(argv: Optional[List[str]] = None):
    """The flags, with the combinations the soft-teacher path cannot serve refused in words."""
    parser = build_parser()
    flags = parser.parse_args(argv)
    if flags.soft_teacher and not flags.device_memory:
        parser.error("--soft_teacher needs --device_memory: augmented and low-resolution soft batches are a device-memory capability (the host "
                     "deques carry no teacher logits)")
    if flags.labels_from_logits and not flags.soft_teacher:
        parser.error("--labels_from_logits needs --soft_teacher: the labels are derived from the teacher logits that flag caches")
    for name in ("kd_temperature", "kd_alpha", "kd_conf_gamma"):
        if getattr(flags, name) is not None and not flags.soft_teacher:
            parser.error("--%s needs --soft_teacher: it shapes the loss against the teacher logits that flag caches" % name)
    problem = loss_knobs_problem(flags.soft_teacher, dash="--", **{name: getattr(flags, name) for name in ("kd_temperature", "kd_alpha", "kd_conf_gamma")
                                                                   if getattr(flags, name) is not None})
    if problem:
        parser.error(problem)
    if flags.uplink_gop < 1:
        parser.error("--uplink_gop must be at least 1 (got %d)" % flags.uplink_gop)
    if flags.uplink_gop > 1 and not flags.compress_uplink:
        parser.error("--uplink_gop needs --compress_uplink: predicted frames are a payload kind of the uplink frame codec")
    if flags.compress_uplink:
        import torch
        if not torch.cuda.is_available():
            parser.error("--compress_uplink needs a GPU: the uplink frame codec runs on the device and has no host fallback")
        if flags.height < 8 or flags.height % 8 != 0:
            parser.error("--compress_uplink needs --height to be a multiple of 8 (got %d): the codec takes frames of 2 x height by 4 x height "
                         "in macroblocks of 16 x 16" % flags.height)
        if flags.height > 1024:
            parser.error("--compress_uplink takes --height up to 1024 (got %d): the codec's frames are at most 4096 wide" % flags.height)
        if not (np.isfinite(flags.uplink_bw) and flags.uplink_bw > 0):
            parser.error("--uplink_bw must be finite and > 0 kbit/s (got %r)" % flags.uplink_bw)
    if flags.loss_top_k_warmup is not None and flags.loss_top_k is None:
        parser.error("--loss_top_k_warmup needs --loss_top_k: it eases the mining in")
    problem = loss_knobs_problem(True, dash="--", **{name: getattr(flags, name) for name in ("loss_top_k", "loss_top_k_warmup")
                                                     if getattr(flags, name) is not None})
    if problem:
        parser.error(problem)
    if flags.loss_class_weights is not None and flags.loss_class_weights != "balanced":
        try:
            parse_loss_class_weights(flags.loss_class_weights, int(class_weights(video_number(flags.input_video)).sum()))
        except ValueError as e:
            parser.error(str(e))
    if flags.labels_from_logits and is_coco(video_number(flags.input_video)):
        parser.error("--labels_from_logits does not go with experiment %d: its teacher labels arrive in COCO numbering and are converted on the "
                     "way into the memory (map_coco), which an argmax over the logits' own classes cannot stand for"
                     % video_number(flags.input_video))
    return flags


def main(argv: Optional[List[str]] = None, network_cls=None):
    flags = parse_flags(argv)
    assert not flags.enable_ATR or flags.enable_ASR, 'ASR must be enabled for ATR to work'
    assert not flags.enable_ASR or flags.mode == 'simple', 'ASR can only be used in simple mode'
    assert not flags.enable_ATR or flags.mode == 'simple', 'ATR can only be used in simple mode'
    assert not flags.edge_from_delta or flags.mode in ('simple', 'early', 'pretrained'), \
        '--edge_from_delta needs an edge that starts from the server\'s initial model (simple, early or pretrained mode)'
    assert not flags.device_render or flags.save_pic, '--device_render paints the pictures of --save_pic: pass both'
    assert not flags.edge_confidence or hasattr(network_cls or SemanticNetwork, "predict_with_confidence"), \
        '--edge_confidence needs a network that computes the student\'s confidence on the GPU (predict_with_confidence): %s has none' \
        % (network_cls or SemanticNetwork).__name__
    os.makedirs(flags.output_dir, exist_ok=True)
    ctx = Context(flags, network_cls)
    vid_num, length = ctx.vid_num, ctx.length
    summary = None
    if flags.mode == 'simple':
        run_label = "%d__%d_tp%d_f%d" % (0, length, flags.train_period, flags.send_period)
        events = event_times(flags, length)
        if not flags.only_results:
            events = train_model(ctx, 0, length, flags.send_period, flags.gpu, run_label, flags.gt_video, vid_num, events,
                                 flags.train_period)          # the times at which a model was actually published
            summary = infer_output(ctx, 0, length, flags.gpu, run_label, flags.gt_video, vid_num, events)
    elif flags.mode == 'early':
        run_label = "early%d_f%d" % (flags.early_cutoff_time, flags.send_period)
        events = [0, flags.early_cutoff_time]
        if not flags.only_results:
            events = train_model(ctx, 0, flags.early_cutoff_time, flags.send_period, flags.gpu, run_label, flags.gt_video,
                                 vid_num, events, flags.train_period)
            summary = infer_output(ctx, 0, length, flags.gpu, run_label, flags.gt_video, vid_num, events)
    elif flags.mode == 'pretrained':
        run_label = "pretrained"
        train_model(ctx, 0, 1, flags.send_period, flags.gpu, run_label, flags.gt_video, vid_num, [0], flags.train_period)
        summary = infer_output(ctx, 0, length, flags.gpu, run_label, flags.gt_video, vid_num, [0])
    else:  # horizon: retrain on [t-k1, t), evaluate on [t, t+k2)
        k1s, k2 = [int(k) for k in flags.horizon_k1s.split(",")], flags.horizon_k2
        number_of_points = flags.horizon_points
        step = (length - k2 - k1s[-1]) // max(number_of_points - 1, 1)
        assert step > 0, "video too short for horizon mode"
        # the un-adapted model over the whole video first, as the reference does (run.py:617-619)
        train_model(ctx, 0, 1, flags.send_period, flags.gpu, "pretrained", flags.gt_video, vid_num, [0], flags.train_period)
        infer_output(ctx, 0, length, flags.gpu, "pretrained", flags.gt_video, vid_num, [0])
        for p in range(number_of_points):
            t = k1s[-1] + p * step
            for k1 in k1s:
                run_label = "%d__%d__%d_f%d" % (t - k1, t, t + k2, flags.send_period)
                train_model(ctx, t - k1, t, flags.send_period, flags.gpu, run_label, flags.gt_video, vid_num, [t], flags.train_period)
                summary = infer_output(ctx, t, t + k2, flags.gpu, run_label, flags.gt_video, vid_num, [t])
    print("Process [Main]:", "Done!!!", summary if summary else "")
    return summary


if __name__ == "__main__":
    main(sys.argv[1:])
