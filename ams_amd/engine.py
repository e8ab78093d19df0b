"""Python handle over the C++/HIP student engine (ams_amd/csrc/engine_*.hip, api.hip).

PyTorch-ROCm is plumbing here: it owns the device arena (one ``torch.uint8`` tensor the engine carves up),
the H2D/D2H copies and the stream; all arithmetic happens in libams_hip.so.  There is no CPU path: creating
an engine without a GPU or without the built library raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import coord_masks, hip
from .delta import check_format
from .spec import (BN_DECAY, BN_EPS_FROZEN, PIXEL_SCALE, Layer, StudentSpec, build_spec)
from . import weights as W

_ACT = {"none": hip.ACT_NONE, "relu": hip.ACT_RELU, "relu6": hip.ACT_RELU6}

# Tuning knobs of tools/*.sh and the profiling recipes: environment variable -> ams_student_set_option id.  They are read HERE, once per
# engine, and applied through the one documented option entry point; the library itself reads no per-student environment.
_ENV_OPTIONS = {
    "AMS_DUAL_STREAM": hip.OPT_DUAL_STREAM, "AMS_DUAL_PARTS": hip.OPT_DUAL_PARTS, "AMS_DUAL_AUTOTUNE": hip.OPT_DUAL_AUTOTUNE,
    "AMS_BLOCK_X6": hip.OPT_BLOCK_X6, "AMS_LATE_SUB": hip.OPT_LATE_SUBBATCH, "AMS_STREAM_MIN_ROWS": hip.OPT_STREAM_MIN_ROWS,
    "AMS_OVERLAP_HEAD": hip.OPT_OVERLAP_HEAD, "AMS_FUSE_BLOCK": hip.OPT_FUSE_BLOCK, "AMS_FUSE_XDS": hip.OPT_FUSE_EXPAND_DW_STREAM,
    "AMS_OVERLAP_WGRAD": hip.OPT_OVERLAP_WGRAD, "AMS_FUSE_DGRAD_BN": hip.OPT_FUSE_DGRAD_BN, "AMS_FUSE_GEMM_RED": hip.OPT_FUSE_GEMM_RED,
    "AMS_TRAIN_RECOMPUTE": hip.OPT_TRAIN_RECOMPUTE, "AMS_NAN_GRADS": hip.OPT_NAN_GRADS, "AMS_FUSE_OPERAND_BN": hip.OPT_FUSE_OPERAND_BN,
    "AMS_WGRAD_FORK_EVERY": hip.OPT_WGRAD_FORK_EVERY, "AMS_TRAIN_FWD_F16": hip.OPT_TRAIN_FWD_F16,
    "AMS_FUSE_HEAD": hip.OPT_FUSE_HEAD,
}


def _role(layer: Layer) -> int:
    s = layer.scope
    if s == "MobilenetV2/Conv":
        return hip.ROLE_STEM
    if s.endswith("/expand"):
        return hip.ROLE_EXPAND
    if s.endswith("/depthwise"):
        return hip.ROLE_DEPTHWISE
    if s.endswith("/project"):
        return hip.ROLE_PROJECT
    return {"image_pooling": hip.ROLE_POOL_CONV, "aspp0": hip.ROLE_ASPP, "concat_projection": hip.ROLE_CONCAT_PROJ,
            "logits/semantic": hip.ROLE_LOGITS}[s]


def layer_table(spec: StudentSpec):
    """spec.py layer table -> C array of ams_layer_desc."""
    arr = (hip.LayerDesc * len(spec.layers))()
    for i, l in enumerate(spec.layers):
        d = arr[i]
        d.role = _role(l)
        d.cin, d.cout, d.stride, d.rate = l.cin, l.cout, l.stride, l.rate
        d.act = _ACT[l.act]
        d.residual_from = l.residual_from or 0
        d.w_off = spec.by_name[l.weight_name].offset
        if l.bn_eps is not None:
            d.bn_eps = l.bn_eps
            d.gamma_off = spec.by_name[l.scope + "/BatchNorm/gamma:0"].offset
            d.beta_off = spec.by_name[l.scope + "/BatchNorm/beta:0"].offset
            d.mean_off = spec.by_name[l.scope + "/BatchNorm/moving_mean:0"].offset
            d.var_off = spec.by_name[l.scope + "/BatchNorm/moving_variance:0"].offset
        else:
            d.bn_eps = -1.0
            d.gamma_off = spec.by_name[l.scope + "/biases:0"].offset
            d.beta_off = d.mean_off = d.var_off = 0
    return arr


class StudentEngine:
    """One student network resident on one GPU."""

    def __init__(self, class_indices: Sequence[int], height: int, width: Optional[int] = None, max_batch: int = 1,
                 trainable: bool = False, num_classes: int = 19, device: str | torch.device = "cuda:0"):
        if not torch.cuda.is_available():
            raise hip.AmsHipError("no GPU visible: the AMS student runs only on MI355X (no CPU fallback)")
        self.lib = hip.lib()
        self.device = torch.device(device)
        self.spec = build_spec(num_classes)
        self.height, self.width = int(height), int(width if width is not None else 2 * height)
        self.max_batch = int(max_batch)
        self.trainable = bool(trainable)
        self.num_classes = int(num_classes)
        self.soft_teacher = False
        self.kd_temperature, self.kd_alpha = 1.0, 1.0
        self.loss_class_weights, self.conf_gamma = None, 0.0
        self.loss_top_k, self._mining_scratch = 1.0, None
        self._reg_mask = self._teacher_logits_dev = None
        self._frames_b, self._frames_u8, self._frames_metric = 0, False, False
        self.class_indices = [int(c) for c in class_indices]
        self.K = len(self.class_indices)
        cfg = hip.StudentConfig()
        cfg.abi_version = hip.ABI_VERSION
        cfg.height, cfg.width, cfg.max_batch = self.height, self.width, self.max_batch
        cfg.num_classes, cfg.n_selected = num_classes, self.K
        for i, c in enumerate(self.class_indices):
            cfg.class_indices[i] = c
        cfg.n_layers = len(self.spec.layers)
        cfg.trainable = 1 if trainable else 0
        cfg.act_dtype = hip.DT_F32
        cfg.n_trainable, cfg.n_stats = self.spec.n_trainable, self.spec.n_stats
        cfg.bn_decay, cfg.bn_eps_frozen, cfg.pixel_scale = BN_DECAY, BN_EPS_FROZEN, PIXEL_SCALE
        self._cfg = cfg
        self._layers = layer_table(self.spec)
        need = C.c_size_t(0)
        hip.check(self.lib.ams_student_arena_bytes(C.byref(cfg), self._layers, C.byref(need)), "ams_student_arena_bytes")
        self.arena_bytes = int(need.value)
        with torch.cuda.device(self.device):
            self.arena = torch.zeros(self.arena_bytes, dtype=torch.uint8, device=self.device)
            handle = C.c_void_p()
            hip.check(self.lib.ams_student_create(C.byref(cfg), self._layers, C.c_void_p(self.arena.data_ptr()),
                                                  self.arena_bytes, C.byref(handle)), "ams_student_create")
        self._h = handle
        self.params = self._view(hip.REGION_PARAMS, torch.float32)
        self.stats = self._view(hip.REGION_STATS, torch.float32)
        self.frozen_params = self._view(hip.REGION_FROZEN, torch.float32)
        self.logits_lowres = self._view(hip.REGION_LOGITS, torch.float32)
        self.bn_sync = self._view(hip.REGION_BN_SYNC, torch.float64)
        if trainable:
            self.grads = self._view(hip.REGION_GRADS, torch.float32)
            self.adam_m = self._view(hip.REGION_ADAM_M, torch.float32)
            self.adam_v = self._view(hip.REGION_ADAM_V, torch.float32)
        h, w = C.c_int32(), C.c_int32()
        hip.check(self.lib.ams_student_lowres_size(self._h, C.byref(h), C.byref(w)))
        self.lowres = (h.value, w.value)
        # one output block for the host-returning calls: [conf int64 K*K | loss f64[2] | labels int32 B*H*W], mirrored in pinned
        # host memory, so a call costs ONE device -> host copy and no allocation (SemanticNetwork.predict_with_metric)
        self._out_meta = (self.K * self.K + 2) * 8
        nbytes = self._out_meta * self.max_batch + self.max_batch * self.height * self.width * 4      # room for per-frame metrics too
        self._out_dev = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._out_host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
        # ... and one pinned input block [frames uint8 B*H*W*3 | labels uint8 B*H*W]: host uint8 arrays are gathered there and leave with an
        # asynchronous DMA (a pageable source makes the driver stage the copy itself, synchronously, chunk by chunk); `_in_free` is the event of
        # the last DMA that read the block
        self._in_frames = torch.zeros(self.max_batch * self.height * self.width * 3, dtype=torch.uint8).pin_memory()
        self._in_labels = torch.zeros(self.max_batch * self.height * self.width, dtype=torch.uint8).pin_memory()
        self._in_free = {}
        self._keepalive = []
        # edge-side model updates (apply_delta): pinned staging + device buffer of the largest payload (created on first use), the status words,
        # and the generation a GraphedPredict checks: it moves when a re-freeze after an update may have changed the fp16 fallback set
        self._delta_host = self._delta_dev = self._delta_scratch = None
        self._delta_words = torch.zeros(2, dtype=torch.int64, device=self.device)           # [values applied, status (int32)]
        self._updated_since_freeze = False
        self._fallback_layers = 0
        # server-side model updates (select_changed, encode_delta): scratch (created on first use), [a, b | NaN changes | kept | payload bytes]
        self._select_scratch = self._encode_scratch = None
        self._select_words = torch.zeros(4, dtype=torch.int64, device=self.device)
        # the q8 delta: the base the encoder subtracts (set_delta_base: params / stats in arena order), its scratch, [payload bytes, status (int32)]
        self._q8_base = None
        self._q8_scratch = None
        self._q8_words = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.generation = 0
        for name, opt in _ENV_OPTIONS.items():
            if name in os.environ:
                hip.check(self.lib.ams_student_set_option(self._h, opt, int(os.environ[name])), "ams_student_set_option(%s)" % name)

    # ------------------------------------------------------------------ plumbing
    def _view(self, region: int, dtype: torch.dtype) -> torch.Tensor:
        off, n = C.c_size_t(), C.c_size_t()
        hip.check(self.lib.ams_student_region(self._h, region, C.byref(off), C.byref(n)), "ams_student_region")
        item = torch.empty((), dtype=dtype).element_size()
        return self.arena[off.value:off.value + n.value * item].view(dtype)

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self) -> None:
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self.lib.ams_student_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _frames_to_device(self, frames) -> tuple:
        """[B,H,W,3] uint8 or float array/tensor -> (device tensor, dtype code, B)."""
        if isinstance(frames, torch.Tensor):
            t = frames
        else:
            a = np.asarray(frames)
            if a.dtype == np.uint8 and a.ndim == 4 and tuple(a.shape[1:]) == (self.height, self.width, 3) and 0 < a.shape[0] <= self.max_batch:
                return self._staged(a, self._in_frames), hip.DT_U8, int(a.shape[0])
            a = np.ascontiguousarray(a)
            if a.dtype != np.uint8:
                a = a.astype(np.float32, copy=False)
            t = torch.from_numpy(a)
        if t.dtype not in (torch.uint8, torch.float32):
            t = t.to(torch.float32)
        assert t.dim() == 4 and tuple(t.shape[1:]) == (self.height, self.width, 3), \
            "frames must be [B,%d,%d,3], got %s" % (self.height, self.width, tuple(t.shape))
        assert 0 < t.shape[0] <= self.max_batch, "batch %d outside 1..%d" % (t.shape[0], self.max_batch)
        t = t.to(self.device, non_blocking=True).contiguous()
        return t, (hip.DT_U8 if t.dtype == torch.uint8 else hip.DT_F32), int(t.shape[0])

    def _staged(self, a: np.ndarray, block: torch.Tensor) -> torch.Tensor:
        """host uint8 array -> device tensor through the engine's pinned input block (one host copy, one asynchronous DMA)."""
        prev = self._in_free.get(id(block))
        if prev is not None:
            prev.synchronize()                          # the previous DMA out of THIS block (long done in a synchronous call loop)
        view = block[:a.size].view(a.shape)
        np.copyto(view.numpy(), a)
        t = view.to(self.device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._in_free[id(block)] = ev
        return t

    def _labels_to_device(self, labels, batch: int) -> torch.Tensor:
        if isinstance(labels, torch.Tensor):
            t = labels
        else:
            a = np.asarray(labels)
            if a.dtype == np.uint8 and tuple(a.shape) == (batch, self.height, self.width) and a.size <= self._in_labels.numel():
                return self._staged(a, self._in_labels)
            if a.dtype != np.uint8:
                # tf.cast(labels, int32) truncates toward zero; ids outside 0..255 can never be selected -> 255
                ai = a.astype(np.float32).astype(np.int64)
                a = np.where((ai >= 0) & (ai < 255), ai, 255).astype(np.uint8)
            t = torch.from_numpy(np.ascontiguousarray(a))
        if t.dtype != torch.uint8:
            ti = t.to(torch.int64)
            t = torch.where((ti >= 0) & (ti < 255), ti, torch.full_like(ti, 255)).to(torch.uint8)
        assert tuple(t.shape) == (batch, self.height, self.width), "labels must be [B,H,W], got %s" % (tuple(t.shape),)
        return t.to(self.device, non_blocking=True).contiguous()

    # ------------------------------------------------------------------ variables
    def load_variables(self, variables: Dict[str, np.ndarray]) -> None:
        """Assign every model variable present in ``variables`` (SaveHelper.restore_vars); Adam state untouched."""
        tr = self.params.cpu().numpy()
        st = self.stats.cpu().numpy()
        W.fill_flat(tr, [v for v in self.spec.trainable if v.name in variables], variables)
        W.fill_flat(st, [v for v in self.spec.stats if v.name in variables], variables)
        self.params.copy_(torch.from_numpy(tr))
        self.stats.copy_(torch.from_numpy(st))

    def get_variables(self) -> Dict[str, np.ndarray]:
        return W.unpack(self.spec, self.params.cpu().numpy(), self.stats.cpu().numpy())

    def set_matmul_mode(self, mode: int) -> None:
        """hip.MATMUL_SPLIT_BF16_X6 (default: late-layer products via 6 bf16 MFMAs on three-part splits, f32-level),
        hip.MATMUL_SPLIT_BF16 (3 MFMAs on two-part splits in frozen inference: +5 % frames/s, logits 2e-4..5e-4),
        hip.MATMUL_F32 (exact f32 MFMA everywhere) or hip.MATMUL_BF16 (the opt-in bf16 variant: one part, plain bf16 products in the
        late layers of frozen inference; outside the f32 tolerance — bench.py reports its mismatch beside its speed)."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_MATMUL, int(mode)), "ams_student_set_option")

    def pack_masked_fp16(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Masked trainable parameters as fp16, compacted in trainable order, on the device (the value part of the downlink
        delta, reference run.py:330-332).  mask: uint8 [n_trainable] on the device, None = all.  -> int16 view of the halves."""
        n = self.spec.n_trainable
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == n and mask.device == self.arena.device
        out = torch.empty(n, dtype=torch.int16, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int64, device=self.device)
        scratch = torch.empty(int(self.lib.ams_pack_masked_fp16_scratch(n)), dtype=torch.int64, device=self.device)
        hip.check(self.lib.ams_pack_masked_fp16(C.c_void_p(self.params.data_ptr()), C.c_void_p(mask.data_ptr()) if mask is not None else None,
                                                n, C.c_void_p(out.data_ptr()), C.c_void_p(cnt.data_ptr()),
                                                C.c_void_p(scratch.data_ptr()), scratch.numel(), self._stream()),
                  "ams_pack_masked_fp16")
        return out[:int(cnt.item())]

    def set_fuse_operand_bn(self, on: bool) -> None:
        """Fine-tune step: BN + activation of the depthwise layers applied by the project GEMM / project weight gradient on their operand loads
        (default on; the depthwise activation is never written); bit-identical to off = the pass written."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_OPERAND_BN, int(bool(on))), "ams_student_set_option")

    def set_wgrad_fork_every(self, n: int) -> None:
        """Fine-tune step: weight gradients handed to the side stream ``n`` at a time (default 1: each as soon as its operands exist; larger
        n = fewer events on the main stream, measured slower on MI355X).  Bit-identical for every n."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_WGRAD_FORK_EVERY, int(n)), "ams_student_set_option")

    def set_train_recompute(self, on: bool, fuse_dgrad_bn: Optional[bool] = None, fuse_gemm_red: Optional[int] = None) -> None:
        """Fine-tune step of the early blocks without their 6x-expanded tensors (default on); off = every tensor materialised.
        ``fuse_dgrad_bn``: the one-kernel depthwise backward of the stride-16 blocks (default on).
        ``fuse_gemm_red``: BN column reductions in the 1x1 GEMM epilogues, bit 0 forward statistics, bit 1 backward sums (default 3)."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_TRAIN_RECOMPUTE, 2 if on is True else int(on)), "ams_student_set_option")
        if fuse_gemm_red is not None:
            hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_GEMM_RED, int(fuse_gemm_red)), "ams_student_set_option")
        if fuse_dgrad_bn is not None:
            hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_DGRAD_BN, 2 if fuse_dgrad_bn is True else int(fuse_dgrad_bn)), "ams_student_set_option")

    def set_soft_teacher(self, on: bool) -> None:
        """create_student_v3(soft_teacher=True) (utils/graph_utils.py:403-404): the fine-tune loss targets softmax(gather(teacher logits)); every
        ``train_step`` then needs ``teacher_logits``."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_SOFT_TEACHER, int(bool(on))), "ams_student_set_option")
        self.soft_teacher = bool(on)

    def set_kd(self, temperature: float = 1.0, alpha: float = 1.0) -> None:
        """Temperature and soft : hard mix of the soft-teacher step (this project's own; the reference's soft loss is ``(1, 1)``): per valid
        pixel ``alpha T^2 CE(softmax(t / T), softmax(z / T)) + (1 - alpha) CE(onehot(y), softmax(z))``.  ``temperature`` finite and > 0,
        ``alpha`` in [0, 1]; read only while ``set_soft_teacher(True)`` holds.  ``alpha = 0`` is the hard-label step."""
        hip.check(self.lib.ams_student_set_kd(self._h, float(temperature), float(alpha)), "ams_student_set_kd")
        self.kd_temperature, self.kd_alpha = float(temperature), float(alpha)

    def set_loss_weights(self, class_weights=None, conf_gamma: float = 0.0) -> None:
        """Weights of the fine-tune loss (this project's own): ``class_weights``, K floats in the order of the class index list, each 0 or in
        [2^-6, 16] (None = ones), and ``conf_gamma`` in [0, 8], the exponent of the teacher's confidence ``c = max_k softmax(t / T)_k`` (needs
        ``set_soft_teacher(True)`` when > 0).  Per valid pixel ``w = cw_y c^gamma``; loss and gradient become the ``w``-weighted means, and a
        step's second number is the sum of the weights instead of the pixel count.  Ones and 0 are the unweighted step, bit for bit."""
        cw = None
        if class_weights is not None:
            cw = np.ascontiguousarray(np.asarray(class_weights, dtype=np.float32).reshape(-1))
        hip.check(self.lib.ams_student_set_loss_weights(self._h, cw.ctypes.data_as(C.POINTER(C.c_float)) if cw is not None else None,
                                                        int(cw.size) if cw is not None else 0, float(conf_gamma)), "ams_student_set_loss_weights")
        self.loss_class_weights, self.conf_gamma = cw, float(conf_gamma)

    def set_loss_mining(self, top_k: float = 1.0) -> None:
        """Hard-pixel mining (DeepLab's ``top_k_percent_pixels``; this project's own knob): a step's loss and gradient are those of the
        objective over the fraction ``top_k`` in (0, 1] of the valid pixels whose own objective value is largest, ties at the threshold all
        kept; the mean divides by what was kept.  ``1.0`` (the default) is the unmined step, launch for launch.  The scratch (key map, mined
        labels, histograms, result) is a torch tensor of this engine's, allocated at the first ``top_k < 1``; the arena does not change."""
        top_k = float(top_k)
        if top_k < 1.0 and self._mining_scratch is None:
            n = self.lib.ams_k_loss_mining_scratch(self.max_batch, self.height, self.width)
            self._mining_scratch = torch.zeros(n, dtype=torch.uint8, device=self.device)
        scr = self._mining_scratch
        hip.check(self.lib.ams_student_set_loss_mining(self._h, top_k, C.c_void_p(scr.data_ptr() if scr is not None else 0),
                                                       int(scr.numel()) if scr is not None else 0), "ams_student_set_loss_mining")
        self.loss_top_k = top_k

    def mining_result(self) -> dict:
        """The last mined step's block: ``threshold`` (the k-th largest key), ``valid`` (n), ``rank`` (k) and ``kept``.  Synchronises."""
        r = hip.MiningResult()
        hip.check(self.lib.ams_student_mining_result(self._h, C.byref(r), self._stream()), "ams_student_mining_result")
        return {"threshold": float(r.threshold), "valid": int(r.valid), "rank": int(r.rank), "kept": int(r.kept)}

    def mined_labels(self, batch: int) -> torch.Tensor:
        """The label map the last mined step of ``batch`` frames ran its loss on (uint8 [batch, H, W], a dropped pixel reads 255): a view of
        the scratch, valid until the next mined step."""
        n = self.max_batch * self.height * self.width
        off = hip.MINING_KEYS_OFFSET + (4 * n + 15) // 16 * 16
        return self._mining_scratch[off:off + batch * self.height * self.width].view(batch, self.height, self.width)

    def set_regularizer(self, on: bool, biases_only: bool = False, coef: float = 0.01) -> None:
        """create_student_v3(regularize=True[, train_biases_only=True]) (utils/graph_utils.py:451-456): loss += coef * mean over tvars of
        l2_loss(v); tvars = every trainable variable, or those without 'weight' in their name."""
        if not on:
            hip.check(self.lib.ams_student_set_regularizer(self._h, None, 0, 0.0), "ams_student_set_regularizer")
            self._reg_mask = None
            return
        flat = np.zeros(self.spec.n_trainable, dtype=np.uint8)
        tvars = [v for v in self.spec.trainable if not (biases_only and 'weight' in v.name)]
        for part in W.split_flat(flat, tvars):
            part[...] = 1
        n_vars = len(tvars)
        self._reg_mask = torch.from_numpy(flat).to(self.device)          # referenced by the handle: kept alive here
        hip.check(self.lib.ams_student_set_regularizer(self._h, C.c_void_p(self._reg_mask.data_ptr()), n_vars, float(coef)),
                  "ams_student_set_regularizer")

    def teacher_logits_layout(self, channels: int, layout: Optional[str] = None) -> int:
        """AMS_TLOGITS_* of teacher logits whose last dimension is ``channels``.  ``layout`` None: ``num_classes`` channels are the full
        layout, ``K`` channels (K != num_classes) the selected one — the student's classes, in the order of its class index list."""
        channels = int(channels)
        if layout is None:
            assert channels in (self.num_classes, self.K), \
                "teacher logits must be [batch, th, tw, %d] (full) or [batch, th, tw, %d] (the selected classes), got %d channels" % (self.num_classes, self.K, channels)
            layout = "full" if channels == self.num_classes else "selected"
        assert layout in hip.TLOGITS_LAYOUTS, "layout is 'full' or 'selected', got %r" % (layout,)
        want = self.num_classes if layout == "full" else self.K
        assert channels == want, "teacher logits in the %s layout must be [batch, th, tw, %d], got %d channels" % (layout, want, channels)
        return hip.TLOGITS_LAYOUTS[layout]

    def _feed_teacher_logits(self, teacher_logits, b: int, layout: Optional[str] = None):
        """feed_dict[student['teacher_labels_logits_pl']]: f32 [b, th, tw, num_classes], or [b, th, tw, K] in the selected layout (host array
        or device tensor); returns the device tensor (the caller keeps it alive until the step has been enqueued on the same stream order)."""
        if teacher_logits is None:
            assert not self.soft_teacher, "soft_teacher is on: teacher_logits must be fed (teacher_labels_logits_pl)"
            return None
        t = teacher_logits if isinstance(teacher_logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(teacher_logits, dtype=np.float32))
        assert t.dim() == 4 and t.shape[0] == b, "teacher logits must be [batch, th, tw, %d]" % self.num_classes
        code = self.teacher_logits_layout(t.shape[3], layout)
        assert t.shape[1] <= self.height and t.shape[2] <= self.width
        t = t.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        hip.check(self.lib.ams_student_feed_teacher_logits_layout(self._h, C.c_void_p(t.data_ptr()), int(t.shape[1]), int(t.shape[2]), code),
                  "ams_student_feed_teacher_logits_layout")
        return t

    def set_nan_grads(self, on: bool) -> None:
        """A fine-tune batch without one valid pixel: False (default) NaN loss and ZERO gradients, TensorFlow's result for
        utils/graph_utils.py:408 (reduce_mean over the empty boolean_mask: the weights survive); True NaN gradients instead."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_NAN_GRADS, int(bool(on))), "ams_student_set_option")

    def set_fuse_first_block(self, on: int) -> None:
        """Frozen inference, stem + depthwise + project of the first block: 0 three kernels, 1 one kernel with a tile per block
        (k_first_block.hip; default), 2 one kernel with a tile per wave (k_block.hip; measured slower).  Forms 0 and 2 keep an exact-f32 stem;
        form 1 runs the stem as six bf16 products on three-part splits while set_block_x6 is on (default; f32-level), else the same bits."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_FIRST_BLOCK, int(on)), "ams_student_set_option")

    def set_fuse_dw_project(self, on: bool) -> None:
        """Frozen inference: depthwise + project of the stride-16 blocks as one kernel (default off: measured no faster than
        the two kernels; split-bf16 mode only)."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_DW_PROJECT, int(bool(on))), "ams_student_set_option")

    def set_block_x6(self, on: bool) -> None:
        """Whole-block kernels: expand products of the K = 24 / 32 blocks as six bf16 MFMAs on three-part splits (default on, f32-level)
        or as exact f32 MFMAs (bit-identical to the layer-by-layer plan).  Also selects the stem's products in the one-kernel first block."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_BLOCK_X6, int(bool(on))), "ams_student_set_option")

    def set_dual_stream(self, mode: int, parts: Optional[int] = None, autotune: Optional[bool] = None) -> None:
        """Frozen inference as two to four part-batches on as many streams: 0 never, 1 (default) a fixed function of the batch size
        (never synchronises), n >= 2 always ``parts`` parts from n frames on.  ``autotune=True`` (with mode 1): time the plans inside the
        first call per batch size instead of the static rule (that call synchronises)."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_DUAL_STREAM, int(mode)), "ams_student_set_option")
        if parts is not None:
            hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_DUAL_PARTS, int(parts)), "ams_student_set_option")
        if autotune is not None:
            hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_DUAL_AUTOTUNE, int(bool(autotune))), "ams_student_set_option")

    def set_late_subbatch(self, frames: int) -> None:
        """Frozen inference: frames per pass of the output-stride-16 section (0 = the whole batch); same bits either way."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_LATE_SUBBATCH, int(frames)), "ams_student_set_option")

    def set_fuse_block(self, on: bool) -> None:
        """Frozen inference: every early block with Cin <= 32 as ONE kernel (expand + depthwise + project [+ input]; default on)."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_BLOCK, int(bool(on))), "ams_student_set_option")

    def set_fuse_head(self, on) -> None:
        """Frozen inference, two bits: 1 = aspp0 -> concat_projection -> logits as one chained kernel where all three layers run the fp16
        product; 2 = no f32 store of a project result that only the next block's part planes carry on.  True = both (3, the default),
        False = the three GEMMs and every store.  Bit-identical for every value."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_HEAD, 3 if on is True else int(on)), "ams_student_set_option")

    def set_fuse_expand_dw(self, on: int) -> None:
        """Frozen inference, expand + depthwise of a block as one kernel: 0 never, 1 (default) the blocks where it is
        measured faster, 2 every supported block."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_EXPAND_DW, int(on)), "ams_student_set_option")

    def set_fuse_expand_dw_stream(self, on: int) -> None:
        """Frozen inference, split-bf16 modes: expand + depthwise of the stride-16 blocks as one streaming kernel, bit-identical
        to the two kernels it replaces: 0 never, 1 (default) where measured faster, 2 every supported block."""
        hip.check(self.lib.ams_student_set_option(self._h, hip.OPT_FUSE_EXPAND_DW_STREAM, int(on)), "ams_student_set_option")

    def freeze(self) -> None:
        """Device-side server->edge hand-off (replaces save_to_frozen_graph + reload)."""
        hip.check(self.lib.ams_student_freeze(self._h, self._stream()), "ams_student_freeze")
        before, self._fallback_layers = self._fallback_layers, self.f16_fallback_layers()
        if self._updated_since_freeze and (before or self._fallback_layers):
            # the frozen weights changed with layers in the fp16 fallback before or after: a graph captured earlier may hold the wrong
            # kernel forms (the library reports how many layers fell back, not which: any set but the empty one counts as changed)
            self.generation += 1
        self._updated_since_freeze = False

    def f16_fallback_layers(self) -> int:
        """layers the last freeze moved off the fp16 product form (ams_student_f16_fallback_layers)"""
        n = C.c_int32()
        hip.check(self.lib.ams_student_f16_fallback_layers(self._h, C.byref(n)), "ams_student_f16_fallback_layers")
        return int(n.value)

    def apply_delta(self, payload, layout, fmt: str = "fp16") -> int:
        """Decode a downlink delta (``SemanticNetwork.delta_payload`` bytes of ``layout``, an ``ams_amd.delta.DeltaLayout``) into the unfolded
        variables (``params`` / ``stats``) on the device; returns the number of values written.  ``payload``: bytes / uint8 array (through a
        pinned staging buffer) or a uint8 device tensor.  A malformed payload raises AmsHipError and changes nothing.  The frozen snapshot is
        not touched: call ``freeze`` to serve the update.  Synchronises the stream once (the status word).

        ``fmt="q8"``: the payload holds int8 codes of the change and one scale per variable (``ams_student_apply_delta_q8``); every masked
        element becomes its current value plus scale x code, so the variables must hold the base the server encoded against."""
        q8 = check_format(fmt) == "q8"
        limit = layout.payload_limit(fmt)
        if isinstance(payload, torch.Tensor):
            assert payload.dtype == torch.uint8 and payload.device == self.arena.device, "payload: a uint8 tensor on the engine's device"
            dev = payload.contiguous().view(-1)
            n = int(dev.numel())
        else:
            a = np.frombuffer(payload, dtype=np.uint8) if isinstance(payload, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1)
            n = int(a.size)
            if n > limit:
                raise hip.AmsHipError("delta payload rejected: %d bytes, the %s layout holds at most %d%s; the model is unchanged"
                                      % (n, layout.kind, limit, " in the q8 format" if q8 else ""))
            if self._delta_host is None or self._delta_host.numel() < limit:
                room = max(layout.max_payload_bytes, layout.max_payload_bytes_q8)
                self._delta_host = torch.empty(room, dtype=torch.uint8).pin_memory()
                self._delta_dev = torch.empty(room, dtype=torch.uint8, device=self.device)
            np.copyto(self._delta_host[:n].numpy(), a)          # (the previous update's copy out of this buffer ended with its status read)
            self._delta_dev[:n].copy_(self._delta_host[:n], non_blocking=True)
            dev = self._delta_dev
        table = layout.table()
        entry, scratch_of = (self.lib.ams_student_apply_delta_q8, self.lib.ams_student_apply_delta_q8_scratch) if q8 else \
            (self.lib.ams_student_apply_delta, self.lib.ams_student_apply_delta_scratch)
        need = int(scratch_of(table, len(table)))
        if self._delta_scratch is None or self._delta_scratch.numel() < need:
            self._delta_scratch = torch.empty(need, dtype=torch.int64, device=self.device)
        words = self._delta_words.data_ptr()
        hip.check(entry(self._h, C.c_void_p(dev.data_ptr()) if n else None, n, table, len(table), C.c_void_p(words), C.c_void_p(words + 8),
                        C.c_void_p(self._delta_scratch.data_ptr()), self._delta_scratch.numel(), self._stream()),
                  "ams_student_apply_delta_q8" if q8 else "ams_student_apply_delta")
        w = self._delta_words.cpu().numpy()
        applied, status = int(w[0]), int(w[1:].view(np.int32)[0])
        if status != hip.DELTA_OK:
            size_rule = "%d mask bytes + 4 per variable + 1 per set bit" % layout.mask_bytes if q8 else "%d mask bytes + 2 per set bit" % layout.mask_bytes
            why = {hip.DELTA_BAD_SIZE: "its size does not match its mask (%s): truncated, over-long or corrupted" % size_rule,
                   hip.DELTA_BAD_PADDING: "a padding bit after a variable's last element is set",
                   hip.DELTA_BAD_SCALE: "a variable's scale is NaN, infinite, negative or denormal"}.get(status, "status %d" % status)
            raise hip.AmsHipError("delta payload rejected (%d bytes, %s layout%s): %s; the model is unchanged"
                                  % (n, layout.kind, ", q8" if q8 else "", why))
        if applied:
            self._updated_since_freeze = True
        return applied

    # ------------------------------------------------------------------ server-side model updates (k_select.hip)
    def snapshot_params(self) -> torch.Tensor:
        """A device copy of the trainable arena: the ``before`` of ``select_changed``."""
        return self.params.clone()

    def select_changed(self, before: torch.Tensor, frac: float):
        """coord_desc_auto's selection on the device (reference SemanticNetwork.py:263-288): keeps the coordinates whose |params - before| lies
        above ``np.percentile(changes, 100 * (1 - frac))`` and sets the others back to ``before``.  Returns (mask uint8 [n_trainable] on the
        device, the number kept as an int64 device tensor of one element).  The two order statistics the percentile interpolates between
        come back to the host (16 bytes, the one synchronisation) and the threshold is formed there with NumPy's arithmetic
        (``coord_masks.percentile_cut``), so it has np.percentile's bits; Adam moments and statistics are not touched."""
        n = self.spec.n_trainable
        assert before.dtype == torch.float32 and before.numel() == n and before.device == self.arena.device
        q = 100 * (1 - frac)
        k = coord_masks.percentile_rank(n, q)
        if self._select_scratch is None:
            self._select_scratch = torch.empty(int(self.lib.ams_select_changed_scratch(n)), dtype=torch.int64, device=self.device)
        words = self._select_words
        hip.check(self.lib.ams_select_changed(C.c_void_p(self.params.data_ptr()), C.c_void_p(before.data_ptr()), n, k, C.c_void_p(words.data_ptr()),
                                              C.c_void_p(self._select_scratch.data_ptr()), self._select_scratch.numel(), self._stream()),
                  "ams_select_changed")
        w = words[:2].cpu().numpy()
        a, b = w[:1].view(np.float32)
        cut = coord_masks.percentile_cut(a, b, n, q, int(w[1]))
        mask = torch.empty(n, dtype=torch.uint8, device=self.device)
        hip.check(self.lib.ams_select_apply(C.c_void_p(self.params.data_ptr()), C.c_void_p(before.data_ptr()), n, float(cut),
                                            C.c_void_p(mask.data_ptr()), C.c_void_p(words.data_ptr() + 16), self._stream()), "ams_select_apply")
        return mask, words[2:3].clone()

    def set_delta_base(self, variables: Optional[Dict[str, np.ndarray]]) -> None:
        """The model the q8 encoder takes the change against: a device copy of ``variables`` in arena order (params and stats), uploaded once
        per call; a variable the dict does not name keeps the engine's current value, so its change is zero.  A pair of f32 device tensors
        (params, stats) of the arena's sizes is taken as it is, and ``advance_base`` then writes into it.  None drops the base."""
        if variables is None:
            self._q8_base = None
            return
        if isinstance(variables, tuple):
            p, s = variables
            assert p.dtype == s.dtype == torch.float32 and p.numel() == self.params.numel() and s.numel() == self.stats.numel()
            assert p.device == s.device == self.arena.device and p.is_contiguous() and s.is_contiguous()
            self._q8_base = (p, s)
            return
        tr = self.params.cpu().numpy()
        st = self.stats.cpu().numpy()
        W.fill_flat(tr, [v for v in self.spec.trainable if v.name in variables], variables)
        W.fill_flat(st, [v for v in self.spec.stats if v.name in variables], variables)
        self._q8_base = (torch.from_numpy(tr).to(self.device), torch.from_numpy(st).to(self.device))

    def _encode_delta_q8(self, layout, mask, cap, advance_base) -> torch.Tensor:
        if self._q8_base is None:
            raise hip.AmsHipError("encode_delta(fmt='q8'): no base; call set_delta_base with the model the receiver holds")
        base_p, base_s = self._q8_base
        table = layout.table()
        need = int(self.lib.ams_student_encode_delta_q8_scratch(table, len(table)))
        if self._q8_scratch is None or self._q8_scratch.numel() < need:
            self._q8_scratch = torch.empty(need, dtype=torch.int64, device=self.device)
        cap = layout.max_payload_bytes_q8 if cap is None else int(cap)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        words = self._q8_words.data_ptr()
        hip.check(self.lib.ams_student_encode_delta_q8(self._h, C.c_void_p(mask.data_ptr()) if mask is not None else None, table, len(table),
                                                       C.c_void_p(base_p.data_ptr()), C.c_void_p(base_s.data_ptr()), int(bool(advance_base)),
                                                       C.c_void_p(out.data_ptr()), cap, C.c_void_p(words), C.c_void_p(words + 8),
                                                       C.c_void_p(self._q8_scratch.data_ptr()), self._q8_scratch.numel(), self._stream()),
                  "ams_student_encode_delta_q8")
        w = self._q8_words.cpu().numpy()
        nbytes, status = int(w[0]), int(w[1:].view(np.int32)[0])
        if status == hip.DELTA_Q8_NONFINITE:
            raise hip.AmsHipError("encode_delta(fmt='q8'): a masked change (variable - base) is NaN or infinite; nothing was written")
        if status != hip.DELTA_OK:
            raise hip.AmsHipError("encode_delta(fmt='q8'): status %d" % status)
        if nbytes > cap:
            raise hip.AmsHipError("encode_delta: the payload has %d bytes, the buffer %d; nothing was written" % (nbytes, cap))
        return out[:nbytes]

    def encode_delta(self, layout, mask: Optional[torch.Tensor] = None, cap: Optional[int] = None, fmt: str = "fp16",
                     advance_base: bool = False) -> torch.Tensor:
        """The downlink delta of ``layout`` (an ``ams_amd.delta.DeltaLayout``) encoded on the device from the current variables: the bytes of
        ``SemanticNetwork.delta_payload`` as a uint8 device tensor (what ``apply_delta`` accepts).  ``mask``: uint8 on the device, one entry per
        element in layout order (the trainable layout: arena order), None = every element.  ``cap``: bytes of the output buffer (default: the
        layout's largest payload); a payload beyond it raises AmsHipError with nothing written.  Synchronises once (the payload's size).

        ``fmt="q8"``: int8 codes of the change against the base of ``set_delta_base`` with one f32 scale per variable
        (``ams_student_encode_delta_q8``); a NaN or infinite masked change raises AmsHipError with nothing written.  ``advance_base=True``
        also moves the base's masked elements to what the receiver decodes, so that the next payload starts from the receiver's model."""
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == layout.n_elements and mask.device == self.arena.device
        if check_format(fmt) == "q8":
            return self._encode_delta_q8(layout, mask, cap, advance_base)
        assert not advance_base, "advance_base belongs to the q8 format: an fp16 payload carries values, not changes"
        table = layout.table()
        need = int(self.lib.ams_student_encode_delta_scratch(table, len(table)))
        if self._encode_scratch is None or self._encode_scratch.numel() < need:
            self._encode_scratch = torch.empty(need, dtype=torch.int64, device=self.device)
        cap = layout.max_payload_bytes if cap is None else int(cap)
        out = torch.empty(cap, dtype=torch.uint8, device=self.device)
        size = self._select_words.data_ptr() + 24
        hip.check(self.lib.ams_student_encode_delta(self._h, C.c_void_p(mask.data_ptr()) if mask is not None else None, table, len(table),
                                                    C.c_void_p(out.data_ptr()), cap, C.c_void_p(size), C.c_void_p(self._encode_scratch.data_ptr()),
                                                    self._encode_scratch.numel(), self._stream()), "ams_student_encode_delta")
        nbytes = int(self._select_words[3].item())
        if nbytes > cap:
            raise hip.AmsHipError("encode_delta: the payload has %d bytes, the buffer %d; nothing was written" % (nbytes, cap))
        return out[:nbytes]

    # ------------------------------------------------------------------ compute
    def predict(self, frames, mode: int = hip.MODE_FROZEN) -> torch.Tensor:
        t, dt, b = self._frames_to_device(frames)
        out = torch.empty((b, self.height, self.width), dtype=torch.int32, device=self.device)
        hip.check(self.lib.ams_student_predict(self._h, C.c_void_p(t.data_ptr()), dt, b, mode, C.c_void_p(out.data_ptr()),
                                               self._stream()), "ams_student_predict")
        return out

    def graphed_predict(self, batch: int, mode: int = hip.MODE_FROZEN) -> "GraphedPredict":
        """Capture one inference step for ``batch`` frames into a hipGraph (see GraphedPredict)."""
        return GraphedPredict(self, batch, mode)

    def predict_with_metric(self, frames, labels_teacher, mode: int = hip.MODE_FROZEN):
        """-> (labels int32 [B,H,W] (device), conf_mat int64 [K,K] (device), loss_sum_count f64[2] (device))."""
        t, dt, b = self._frames_to_device(frames)
        lab = self._labels_to_device(labels_teacher, b)
        out = torch.empty((b, self.height, self.width), dtype=torch.int32, device=self.device)
        conf = torch.empty(self.K * self.K, dtype=torch.int64, device=self.device)
        loss = torch.empty(2, dtype=torch.float64, device=self.device)
        hip.check(self.lib.ams_student_predict_with_metric(
            self._h, C.c_void_p(t.data_ptr()), dt, b, mode, C.c_void_p(lab.data_ptr()), C.c_void_p(out.data_ptr()),
            C.c_void_p(conf.data_ptr()), C.c_void_p(loss.data_ptr()), self._stream()), "ams_student_predict_with_metric")
        return out, conf.view(self.K, self.K), loss

    # Host-returning calls (what SemanticNetwork.predict_input / predict_with_metric make): the label maps leave the device as uint8 (an index
    # inside the subset of K <= 32 classes) and are widened to the reference's int32 on the host: 0.5 MB instead of 2 MB per 512 x 1024 frame over
    # PCIe, and the widening writes the fresh array the caller gets anyway (copying 2 MB of int32 out of the pinned mirror took longer than the
    # transfer).  Metrics come back per frame (ams_student_predict_frames_u8) and are summed here: integers and exact fixed-point sums.
    def predict_host(self, frames, mode: int = hip.MODE_FROZEN) -> np.ndarray:
        """predict() with the label maps returned as a fresh int32 ndarray (one device -> host copy, preallocated buffers)."""
        self.predict_frames(frames, None, mode, u8=True)
        return self.fetch_frames(labels_only=True)[0]

    def predict_with_metric_host(self, frames, labels_teacher, mode: int = hip.MODE_FROZEN):
        """predict_with_metric() -> (labels int32 [B,H,W], conf_mat int64 [K,K], loss_sum_count f64[2]) as fresh ndarrays."""
        self.predict_frames(frames, labels_teacher, mode, u8=True)
        labels, confs, losses = self.fetch_frames()
        return labels, confs.sum(axis=0), losses.sum(axis=0)

    def predict_frames(self, frames, labels_teacher=None, mode: int = hip.MODE_FROZEN, u8: bool = False):
        """Per-FRAME results of one batched pass (ams_student_predict_frames): device tensors labels int32 [B,H,W] (``u8``: uint8, for results
        that go to the host), conf int64 [B,K,K], loss f64 [B,2] (views of the engine's output block, valid until the next host-returning /
        predict_frames call).  Nothing is synchronised; ``fetch_frames`` brings them to the host."""
        t, dt, b = self._frames_to_device(frames)
        lab = self._labels_to_device(labels_teacher, b) if labels_teacher is not None else None
        kk = self.K * self.K
        base = self._out_dev.data_ptr()
        meta = self._out_meta * b
        fn = self.lib.ams_student_predict_frames_u8 if u8 else self.lib.ams_student_predict_frames
        hip.check(fn(self._h, C.c_void_p(t.data_ptr()), dt, b, mode, C.c_void_p(lab.data_ptr()) if lab is not None else None, C.c_void_p(base + meta),
                     C.c_void_p(base), C.c_void_p(base + kk * 8 * b), self._stream()), "ams_student_predict_frames")
        self._keepalive = [t, lab]
        self._frames_b = b
        self._frames_u8 = bool(u8)
        self._frames_metric = lab is not None
        conf = self._out_dev[:kk * 8 * b].view(torch.int64).view(b, self.K, self.K)
        loss = self._out_dev[kk * 8 * b:meta].view(torch.float64).view(b, 2)
        px = b * self.height * self.width
        labels = (self._out_dev[meta:meta + px].view(b, self.height, self.width) if u8 else
                  self._out_dev[meta:meta + px * 4].view(torch.int32).view(b, self.height, self.width))
        return labels, conf, loss

    def last_inputs(self):
        """(frames, teacher labels or None) of the last ``predict_frames`` as the device tensors the pass read (kept alive until the next one)."""
        return self._keepalive[0], self._keepalive[1]

    def fetch_frames(self, labels_only: bool = False):
        """(labels [B,H,W] int32, conf [B,K,K] int64, loss [B,2] f64) of the last ``predict_frames`` as fresh ndarrays: one copy, one sync.
        (``labels_only``, or a pass without teacher labels: conf and loss are None and only the label bytes cross PCIe.)"""
        b = self._frames_b
        kk = self.K * self.K
        meta = self._out_meta * b
        px = b * self.height * self.width
        n = meta + (px if self._frames_u8 else px * 4)
        first = meta if (labels_only or not self._frames_metric) else 0
        self._out_host[first:n].copy_(self._out_dev[first:n], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        host = self._out_host.numpy()
        conf = loss = None
        if first == 0:
            conf = host[:kk * 8 * b].view(np.int64).reshape(b, self.K, self.K).copy()
            loss = host[kk * 8 * b:meta].view(np.float64).reshape(b, 2).copy()
        if self._frames_u8:
            labels = host[meta:n].reshape(b, self.height, self.width).astype(np.int32)       # widened into the fresh array the caller gets
        else:
            labels = host[meta:n].view(np.int32).reshape(b, self.height, self.width).copy()
        return labels, conf, loss

    def confidence(self, teacher=None, f32: bool = False, batch: Optional[int] = None):
        """The student's certainty about the frames of the LAST pass (k_confidence.hip; one launch on the current stream, nothing is
        synchronised): (uint8 map [B,H,W] = rint(p * 255), f32 map [B,H,W] or None, int64 statistics [B, confidence.STATS_LEN]) as fresh
        device tensors, p = the largest softmax value over the selected classes.  ``teacher``: uint8 labels [B,H,W] (host array or device
        tensor) for the calibration fields of the statistics, None = the label-free fields only.  ``batch``: frames of that pass (default:
        those of the last ``predict_frames``).  Call it before the next pass, which overwrites the low-resolution logits it reads."""
        b = int(batch if batch is not None else self._frames_b)
        assert 0 < b <= self.max_batch, "confidence: no pass to read (batch %d outside 1..%d)" % (b, self.max_batch)
        lab = self._labels_to_device(teacher, b) if teacher is not None else None
        n = int(self.lib.ams_confidence_stats_len())
        conf_u8 = torch.empty((b, self.height, self.width), dtype=torch.uint8, device=self.device)
        conf_f32 = torch.empty((b, self.height, self.width), dtype=torch.float32, device=self.device) if f32 else None
        stats = torch.empty((b, n), dtype=torch.int64, device=self.device)
        hip.check(self.lib.ams_student_confidence(self._h, b, C.c_void_p(lab.data_ptr()) if lab is not None else None,
                                                  C.c_void_p(conf_u8.data_ptr()), C.c_void_p(conf_f32.data_ptr()) if f32 else None,
                                                  C.c_void_p(stats.data_ptr()), self._stream()), "ams_student_confidence")
        return conf_u8, conf_f32, stats

    def soft_metric(self, batch: Optional[int], teacher, teacher_logits, want_maps: bool = False, layout: Optional[str] = None):
        """The soft-teacher loss and the probabilistic confusion matrices of the frames of the LAST pass (k_soft_metric.hip; one launch on the
        current stream, nothing is synchronised): (int64 statistics [B, soft_metric.stats_len(K)], f32 p [B,H,W,K] or None, f32 pixel loss
        [B,H,W] or None) as fresh device tensors.  ``teacher``: uint8 ids [B,H,W] (host array or device tensor) or None = every pixel counts;
        ``teacher_logits``: f32 [B,th,tw,num_classes] with th <= H, tw <= W (host array or device tensor), or [B,th,tw,K] in the selected
        layout (``layout``: 'full', 'selected', or None = by the last dimension, ``teacher_logits_layout``).  ``batch``: frames of that pass
        (None: those of the last ``predict_frames``).  Call it before the next pass, which overwrites the low-resolution logits it reads."""
        b = int(batch if batch is not None else self._frames_b)
        assert 0 < b <= self.max_batch, "soft_metric: no pass to read (batch %d outside 1..%d)" % (b, self.max_batch)
        lab = self._labels_to_device(teacher, b) if teacher is not None else None
        t = teacher_logits if isinstance(teacher_logits, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(teacher_logits, dtype=np.float32))
        assert t.dim() == 4 and t.shape[0] == b, "teacher logits must be [%d, th, tw, %d], got %s" % (b, self.num_classes, tuple(t.shape))
        code = self.teacher_logits_layout(t.shape[3], layout)
        assert 1 <= t.shape[1] <= self.height and 1 <= t.shape[2] <= self.width
        t = t.to(self.device, dtype=torch.float32, non_blocking=True).contiguous()
        stats = torch.empty((b, int(self.lib.ams_soft_metric_stats_len(self.K))), dtype=torch.int64, device=self.device)
        p = torch.empty((b, self.height, self.width, self.K), dtype=torch.float32, device=self.device) if want_maps else None
        ce = torch.empty((b, self.height, self.width), dtype=torch.float32, device=self.device) if want_maps else None
        hip.check(self.lib.ams_student_soft_metric_layout(self._h, b, C.c_void_p(lab.data_ptr()) if lab is not None else None, C.c_void_p(t.data_ptr()),
                                                          int(t.shape[1]), int(t.shape[2]), C.c_void_p(stats.data_ptr()),
                                                          C.c_void_p(p.data_ptr()) if want_maps else None,
                                                          C.c_void_p(ce.data_ptr()) if want_maps else None, self._stream(), code),
                  "ams_student_soft_metric_layout")
        self._soft_keepalive = (lab, t)          # alive until the next call replaces them (the launch is stream-ordered behind their copies)
        return stats, p, ce

    def cross_confusion(self, labels_pair) -> torch.Tensor:
        a = np.asarray(labels_pair)
        assert a.shape[0] == 2
        lab = self._labels_to_device(a.reshape(2, *a.shape[1:]), 2) if a.shape[1:] == (self.height, self.width) else None
        assert lab is not None, "labels must be [2,H,W]"
        conf = torch.empty(self.K * self.K, dtype=torch.int64, device=self.device)
        hip.check(self.lib.ams_cross_confusion(self._h, C.c_void_p(lab.data_ptr()), self.height * self.width,
                                               C.c_void_p(conf.data_ptr()), self._stream()), "ams_cross_confusion")
        return conf.view(self.K, self.K)

    def train_step(self, frames, labels_teacher, lr: float, mask: Optional[torch.Tensor] = None,
                   allreduce=None, global_batch: Optional[int] = None, comm=None, teacher_logits=None,
                   teacher_logits_layout: Optional[str] = None) -> torch.Tensor:
        """One Adam iteration; returns the device tensor f64[2] = (CE sum over valid pixels, valid pixel count).

        Data-parallel step, ``global_batch`` = frames over all ranks: ``comm`` = an ``ams_amd.dist.RcclComm``
        (production: the engine issues its all-reduces on the launch stream through RCCL), or ``allreduce`` = an
        ``ams_amd.dist.ArenaAllReduce`` / a callable(tensor) summing in place across ranks (host callback: gloo tests)."""
        assert self.trainable, "Can't train frozen graph!!!"
        t, dt, b = self._frames_to_device(frames)
        lab = self._labels_to_device(labels_teacher, b)
        self._teacher_logits_dev = self._feed_teacher_logits(teacher_logits, b, teacher_logits_layout)          # soft_teacher only; alive until the next step replaces it
        loss = torch.empty(2, dtype=torch.float64, device=self.device)
        mptr = C.c_void_p(mask.data_ptr()) if mask is not None else C.c_void_p(0)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.numel() == self.spec.n_trainable and mask.device == self.arena.device
        if comm is not None:
            assert allreduce is None, "pass either comm (RCCL inside the engine) or allreduce (host callback), not both"
            hip.check(self.lib.ams_student_train_step_rccl(self._h, C.c_void_p(t.data_ptr()), dt, C.c_void_p(lab.data_ptr()), b,
                                                           int(global_batch or b), float(lr), mptr, C.c_void_p(loss.data_ptr()),
                                                           comm._h, self._stream()), "ams_student_train_step_rccl")
            return loss
        if allreduce is None:
            hip.check(self.lib.ams_student_train_step(self._h, C.c_void_p(t.data_ptr()), dt, C.c_void_p(lab.data_ptr()), b,
                                                      float(lr), mptr, C.c_void_p(loss.data_ptr()), self._stream()),
                      "ams_student_train_step")
            return loss
        from .dist import ArenaAllReduce
        reducer = allreduce if isinstance(allreduce, ArenaAllReduce) else ArenaAllReduce(self.arena, reduce_fn=allreduce)
        cb = hip.ALLREDUCE_CB(reducer)
        rc = self.lib.ams_student_train_step_dp(self._h, C.c_void_p(t.data_ptr()), dt, C.c_void_p(lab.data_ptr()), b,
                                                int(global_batch or b), float(lr), mptr, C.c_void_p(loss.data_ptr()),
                                                cb, None, self._stream())
        if reducer.error is not None:
            raise reducer.error
        hip.check(rc, "ams_student_train_step_dp")
        return loss

    @property
    def adam_step(self) -> int:
        t = C.c_int64()
        hip.check(self.lib.ams_student_get_adam_step(self._h, C.byref(t)))
        return int(t.value)

    @adam_step.setter
    def adam_step(self, value: int) -> None:
        hip.check(self.lib.ams_student_set_adam_step(self._h, int(value)))


class GraphedPredict:
    """The ~60 kernel launches of one inference step captured once into a hipGraph and replayed.

    At batch 1 the step is launch-bound (60 launches x ~3.5 us of host time against ~0.4 ms of kernels); a replay costs
    one launch.  Frames are copied into a static uint8 buffer, labels come back in a static int32 buffer (valid until the
    next call).  Capture goes through torch.cuda.graph: the engine launches on torch's current stream, which is the
    capturing stream inside that context."""

    def __init__(self, engine: StudentEngine, batch: int, mode: int = hip.MODE_FROZEN):
        assert 0 < batch <= engine.max_batch
        self.engine, self.batch, self.mode = engine, batch, mode
        dev = engine.device
        self.generation = engine.generation
        self.frames = torch.zeros((batch, engine.height, engine.width, 3), dtype=torch.uint8, device=dev)
        self.labels = torch.empty((batch, engine.height, engine.width), dtype=torch.int32, device=dev)
        self._run()                                   # warm-up outside capture (lazy one-time initialisations)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._run()

    def _run(self) -> None:
        e = self.engine
        hip.check(e.lib.ams_student_predict(e._h, C.c_void_p(self.frames.data_ptr()), hip.DT_U8, self.batch, self.mode,
                                            C.c_void_p(self.labels.data_ptr()), e._stream()), "ams_student_predict")

    def __call__(self, frames) -> torch.Tensor:
        if self.engine.generation != self.generation:
            raise hip.AmsHipError("GraphedPredict: a model update re-froze the engine with another fp16 fallback set than at capture "
                                  "(the graph holds the kernel forms of that time); capture a new one")
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(frames))
        self.frames.copy_(frames, non_blocking=True)
        self.graph.replay()
        return self.labels
