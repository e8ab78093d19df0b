"""``SemanticNetwork`` — the drop-in boundary of the AMS hot path on MI355X.

Mirrors the public surface of the reference class (SemanticNetwork.py:24-755): constructor arguments,
method names, argument meaning, return types, assertion behaviour and the process-wide lock, so that the
reference's edge/server loop (run.py) can use it unchanged.  Underneath, one ``StudentEngine`` (HIP) per
instance replaces the tf.Session; there is no CPU fallback.

Deliberate differences (all listed in INTEGRATION.md):
  * ``<meta_dir>.pb`` written by ``save_to_frozen_graph`` is an ``AMSF`` container (weights + statistics),
    not a TensorFlow GraphDef: the hand-off semantic (inference-mode BN with eps 1e-3 everywhere, trained
    gamma/beta, moving statistics; reference utils/graph_utils.py:52-126) is the same, the bytes are not.
  * ``infer`` / ``train_step`` aliases are added (BASELINE.json north-star names).
  * per-iteration loss printing is off unless ``verbose=True`` (each print forces a device sync).
  * ``device_masks=True`` keeps the server side of a model update on the device (coordinate selection, masks, the delta's bytes); same results.
  * ``train_with_deque`` also takes an ``ams_amd.replay.DeviceReplayMemory`` in place of the two deques: the replay memory and its sampler on
    the device, no helper thread; ``flip=True`` (the reference passes False) is reachable on that path, and so are ``soft_teacher`` batches
    with ``scale != [1]``, crops and flips: teacher logits cached at the frame size are resampled with their frames (ams_amd/replay.py).
  * ``colorize`` / ``colorize_teacher`` / ``cross_ignore`` also take torch device tensors and then paint on the device (k_render.hip) and return
    device tensors; ``predict_rendered`` and ``predict_with_metric_async(..., render=)`` / ``take_rendered`` paint right behind the inference pass.
    On the device a label out of range gives defined output where the host helpers raise IndexError (ams_amd/render.py).
  * ``predict_with_confidence`` / ``predict_probabilities`` / ``predict_with_metric_async(..., confidence=True)`` + ``take_confidence`` expose
    the student graph's ``probabilities_reduced`` (the per-pixel softmax maximum) and its statistics, computed right behind the inference pass
    (k_confidence.hip, ams_amd/confidence.py).
  * ``predict_with_soft_metric`` / ``predict_soft_probabilities`` / ``evaluate_memory`` evaluate the soft-teacher objective and the reference's
    ``prob_confmat`` / ``prob_confmat_star`` against given teacher logits without an optimisation step (k_soft_metric.hip, ams_amd/soft_metric.py).
"""
from __future__ import annotations

import io
import threading
import time
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from . import coord_masks, hip
from .batch_feed import HostBatchFeed
from .confidence import Confidence, ConfidenceStats
from . import weights as W
from .delta import check_format, delta_layout
from .edge_pipeline import EdgePipeline
from .engine import StudentEngine
from .render import VIEWS as RENDER_VIEWS, DeviceRenderer
from .replay import LOW_RES_LOGITS, SAMPLE_FIELDS, DeviceReplayMemory, draw_samples
from .soft_metric import SoftMetric
from .utils import calculate_miou, colormap, loss_knobs_problem, mining_fraction
from .weights import load_npy

FROZEN_MAGIC = b"AMSF\x01"


class FrozenGraph:
    """What the server ships to the edge: every model variable after training (reference: a GraphDef with the
    variables folded to constants and BN rebound to inference mode, utils/graph_utils.py:79-126)."""

    def __init__(self, variables: Dict[str, np.ndarray], class_indices, height: int, num_classes: int):
        self.variables = variables
        self.class_indices = [int(c) for c in class_indices]
        self.height = int(height)
        self.num_classes = int(num_classes)

    def SerializeToString(self) -> bytes:
        buf = io.BytesIO()
        np.savez(buf, __class_indices=np.asarray(self.class_indices, dtype=np.int32),
                 __height=np.asarray(self.height), __num_classes=np.asarray(self.num_classes),
                 **{k.replace("/", "|"): v for k, v in self.variables.items()})
        return FROZEN_MAGIC + buf.getvalue()

    @staticmethod
    def ParseFromString(data: bytes) -> "FrozenGraph":
        if not data.startswith(FROZEN_MAGIC):
            raise ValueError("not an AMSF frozen student (TensorFlow .pb files cannot be loaded by this build)")
        z = np.load(io.BytesIO(data[len(FROZEN_MAGIC):]))
        variables = {k.replace("|", "/"): z[k] for k in z.files if not k.startswith("__")}
        return FrozenGraph(variables, z["__class_indices"].tolist(), int(z["__height"]), int(z["__num_classes"]))


def pass_metrics(conf_i64, loss_sum_count):
    """What follows the labels in a result: (confusion matrix float64, IoU per class, mIoU, loss float32 or NaN) from the int64 confusion
    matrix of a frame (or summed over a pass) and its f64 [loss sum, valid pixel count]."""
    conf_mat_ = conf_i64.astype(np.float64)
    iou_ = calculate_miou(conf_mat_, nan=True)
    loss_ = np.float32(loss_sum_count[0] / loss_sum_count[1]) if loss_sum_count[1] > 0 else np.float32(np.nan)
    return conf_mat_, iou_, np.nanmean(iou_), loss_


class _Pass(NamedTuple):                    # one synchronous inference pass, on the host
    labels: np.ndarray                      # int32 [B,H,W]
    metrics: Optional[tuple]                # pass_metrics summed over the frames; None without teacher labels
    rendered: object                        # RenderedViews (device tensors [B,H,W,3]) or None
    confidence: Optional[Confidence]
    soft: Optional[SoftMetric] = None       # over the frames of the pass

    def result(self, *extras):
        """the tuple the public calls return: labels[, the four metrics][, extras]"""
        return (self.labels,) + (self.metrics or ()) + extras


class SemanticNetwork(object):
    OPT_FILTER = ['Adam', 'Momentum']
    OP_FILTER = ['image_cache:0', 'global_step:0']
    THREAD_SLEEP_INTERVAL = 1 / 1000.
    TOTAL_CLASSES = 19
    WHITE = np.array([255, 255, 255], dtype=np.uint8)
    BLACK = np.array([0, 0, 0], dtype=np.uint8)

    def __init__(self, meta_dir, class_weights_exp=None, height=None, gpu_id='0', frozen=False,
                 scale=None, mini_batch_size=None, lr=None, mem_frac=1, coord_frac=0.1, cross_miou_compat=False,
                 filter_out=None, over_ride_total_classes=None, **kwargs):
        assert height is not None, "No height is given"
        assert class_weights_exp is not None, "No class weights specified"
        assert frozen or None not in [scale, mini_batch_size, lr], "Training parameters must be specified for " \
                                                                   "non-frozen graph"
        self.lr = lr
        self.mini_batch_size = mini_batch_size
        self.scale = scale
        if over_ride_total_classes is not None:
            self.TOTAL_CLASSES = over_ride_total_classes
        self.coord_frac = coord_frac

        self.class_weights_graph = class_weights_exp
        self.class_indices_graph = np.where(self.class_weights_graph == 1)[0]
        assert self.class_weights_graph.shape == (self.TOTAL_CLASSES, 1)
        self.class_count = len(self.class_indices_graph)
        assert self.class_indices_graph.shape == (self.class_count,)
        assert self.class_count > 0
        self.cross_miou_compat = cross_miou_compat

        self.color_map_reduced_ = np.take(colormap(), self.class_indices_graph, axis=0)
        ranks = np.cumsum(self.class_weights_graph).reshape(self.TOTAL_CLASSES) * \
            self.class_weights_graph.reshape(self.TOTAL_CLASSES)
        self.take_array = np.where(ranks != 0, ranks - 1, ranks).astype(int)
        assert self.take_array.shape == (self.TOTAL_CLASSES,)

        self.frozen = frozen
        self.height = height
        assert self.height > 0
        self.meta_dir = meta_dir
        self.process_lock = threading.Lock()
        self.verbose = bool(kwargs.pop("verbose", False))
        # kwargs the reference forwards to create_student_v3 (graph_utils.py:338-339); only the ones run.py can
        # switch on are meaningful here
        self.masked_gradients = bool(kwargs.pop("masked_gradients", False))
        for dead in ("threshold", "map_misc", "test_mode"):
            kwargs.pop(dead, None)
        # create_student_v3's remaining kwargs (utils/graph_utils.py:338-339, 403-404, 451-456); run.py:150 leaves them off
        self.train_biases_only = bool(kwargs.pop("train_biases_only", False))
        self.regularize = bool(kwargs.pop("regularize", False))
        self.soft_teacher = bool(kwargs.pop("soft_teacher", False))
        # this project's own (the reference's soft loss has neither): temperature and soft : hard mix of the soft step (StudentEngine.set_kd).
        # Evaluation (predict_with_soft_metric, evaluate_memory) keeps reporting the reference's T = 1 soft loss
        self.kd_temperature = float(kwargs.pop("kd_temperature", 1.0))
        self.kd_alpha = float(kwargs.pop("kd_alpha", 1.0))
        # this project's own as well: per-class weights of the fine-tune loss and the exponent of the teacher's confidence (StudentEngine.set_loss_weights).
        # Evaluation stays unweighted, so that runs trained under different weights stay comparable
        self.loss_class_weights = kwargs.pop("loss_class_weights", None)
        self.kd_conf_gamma = float(kwargs.pop("kd_conf_gamma", 0.0))
        # ... and hard-pixel mining (StudentEngine.set_loss_mining): a phase's iteration `it` keeps the fraction utils.mining_fraction(loss_top_k,
        # loss_top_k_warmup, it) of the valid pixels.  Evaluation stays unmined, for the reason it stays unweighted
        self.loss_top_k = float(kwargs.pop("loss_top_k", 1.0))
        self.loss_top_k_warmup = kwargs.pop("loss_top_k_warmup", 0)
        self.last_mining = None    # after a phase whose last iteration was mined: that step's threshold, valid, rank and kept
        if frozen:                 # the reference's frozen branch never calls create_student_v3: the kwargs are accepted and unused there too
            self.soft_teacher = self.regularize = self.train_biases_only = False
            self.kd_temperature = self.kd_alpha = 1.0
            self.loss_class_weights, self.kd_conf_gamma = None, 0.0
            self.loss_top_k, self.loss_top_k_warmup = 1.0, 0
        self.loss_class_weights = self._checked_loss_weights(self.loss_class_weights, self.kd_conf_gamma)
        self.loss_top_k_warmup = self._checked_mining(self.loss_top_k, self.loss_top_k_warmup)
        initial_variables = kwargs.pop("initial_variables", None)
        frozen_graph = kwargs.pop("frozen_graph", None)
        max_batch = kwargs.pop("max_batch", None)
        # frozen only: depth of the asynchronous single-call pipeline (predict_with_metric_async / collect); 1 = off
        self.pipeline_depth = int(kwargs.pop("pipeline_depth", 1))
        # training only: masks, coord_desc_auto's selection and the delta's bytes stay on the device (same results; see _train, delta_payload)
        self.device_masks = bool(kwargs.pop("device_masks", False)) and not frozen
        # training from a DeviceReplayMemory only: mini_batch's flip augmentation (the reference passes flip=False, SemanticNetwork.py:687)
        self.flip = bool(kwargs.pop("flip", False))
        assert 1 <= self.pipeline_depth <= 4, "pipeline_depth must be 1 .. 4"
        assert not kwargs, "unknown arguments: %s" % sorted(kwargs)

        # gpu_id is the reference's visible_device_list string (SemanticNetwork.py:74): an ordinal among the devices this process
        # can see.  An ordinal that does not exist is an error, as it is for tf.ConfigProto (no silent fallback to device 0);
        # mem_frac (per_process_gpu_memory_fraction, :73) has no counterpart: the engine allocates exactly its arena.
        device = "cuda:%d" % int(str(gpu_id).split(",")[0]) if not str(gpu_id).startswith("cuda") else str(gpu_id)
        if torch.cuda.is_available() and int(device.split(":")[1]) >= torch.cuda.device_count():
            raise ValueError("gpu_id %r: this process sees %d GPU(s) (ordinals are relative to the visible devices, "
                             "cf. HIP_VISIBLE_DEVICES)" % (gpu_id, torch.cuda.device_count()))
        assert 0 < float(mem_frac) <= 1, "mem_frac must be in (0, 1]"
        self._mem_frac = float(mem_frac)
        if self.frozen:
            if frozen_graph is None:
                with open(meta_dir + ".pb", 'rb') as pb_file:
                    frozen_graph = FrozenGraph.ParseFromString(pb_file.read())
            self._call_batch = int(max_batch or 1)
            self.engine = StudentEngine(self.class_indices_graph, self.height, 2 * self.height,
                                        max_batch=self._call_batch * self.pipeline_depth, trainable=False,
                                        num_classes=self.TOTAL_CLASSES, device=device)
            self.engine.load_variables(frozen_graph.variables)
            self.engine.freeze()
        else:
            self.engine = StudentEngine(self.class_indices_graph, self.height, 2 * self.height,
                                        max_batch=int(max_batch or max(int(mini_batch_size), 1)), trainable=True,
                                        num_classes=self.TOTAL_CLASSES, device=device)
            if filter_out is not None:
                self.OPT_FILTER = list(self.OPT_FILTER) + list(filter_out)
            self.filter = lambda elem: elem if all(
                keyword not in elem for keyword in self.OPT_FILTER) and elem not in self.OP_FILTER else None
            self._initial = initial_variables if initial_variables is not None else load_npy("%s.npy" % self.meta_dir)
            self._restore_dict(self._initial)
            if self.soft_teacher:
                self.engine.set_soft_teacher(True)
                if (self.kd_temperature, self.kd_alpha) != (1.0, 1.0):
                    self.engine.set_kd(self.kd_temperature, self.kd_alpha)
            if self.loss_class_weights is not None or self.kd_conf_gamma != 0.0:
                self.engine.set_loss_weights(self.loss_class_weights, self.kd_conf_gamma)
            if self.regularize:
                self.engine.set_regularizer(True, biases_only=self.train_biases_only)
            self.mask = None
            self.train_params = None
            self.curr_mask = None
            self.last_losses: List[float] = []
        self._last_train_ms = 0.0
        self._renderer = None              # the render tables (DeviceRenderer), built and uploaded on first use
        self._confidence_host = None       # pinned block the statistics rows of a synchronous pass leave through, on first use
        self._soft_host = None             # the same for the rows of the soft-teacher metric
        self._held = None                  # device_masks: what the last phase left on the device (_hold_phase)
        self._q8_tracked = False           # delta_payload(fmt="q8", track_edge=True) has run: the engine's delta base follows the edge's model
        self._auto_mask_dev = None         # device_masks: coord_desc_auto's selection, kept for keep_mask=True
        self._feed = None                  # training from host deques: the helper threads and their pinned ring (_host_feed)
        # frozen with pipeline_depth >= 2: predict_with_metric_async / collect.  Every synchronous pass drains it first (one output block).
        self._pipeline = EdgePipeline(self.engine, self._mode(), self.pipeline_depth, self._get_renderer, pass_metrics, self.class_count)
        # mem_frac (tf.ConfigProto per_process_gpu_memory_fraction, SemanticNetwork.py:73): TensorFlow refuses allocations past that share of
        # the device; the engine allocates exactly one arena, so the cap is checked once, against it
        if torch.cuda.is_available():
            total = torch.cuda.get_device_properties(self.engine.device).total_memory
            if self.engine.arena_bytes > self._mem_frac * total:
                need = self.engine.arena_bytes
                self.engine.close()
                raise MemoryError("the student's arena (%.2f GB) exceeds mem_frac = %g of the device's %.1f GB" % (need / 1e9, self._mem_frac, total / 1e9))

    # ------------------------------------------------------------------ mask / curr_mask / train_params
    # Plain attributes on the host path.  With device_masks=True a phase leaves them on the device (``_held``: the phase's device mask and a
    # device copy of the variables at its end) and the first read brings them to the host, with the values, types and shapes of the host path.
    # ``del`` makes one absent again (the next read materialises it); absent differs from None, so the values live in __dict__ under the
    # properties' own names.
    def _lazy(name):
        def get(self):
            if name not in self.__dict__:
                self._materialise(name)
            return self.__dict__.get(name)

        def put(self, value):
            self.__dict__[name] = value
            if name == "mask" and value is None:
                self._auto_mask_dev = None

        def drop(self):
            self.__dict__.pop(name, None)

        return property(get, put, drop)

    mask = _lazy("mask")
    curr_mask = _lazy("curr_mask")
    train_params = _lazy("train_params")
    del _lazy

    def _materialise(self, name):
        spec = self.engine.spec
        if name == "mask":                                    # coord_desc_auto's selection, kept for keep_mask=True
            if self._auto_mask_dev is not None:
                flat = self._auto_mask_dev.cpu().numpy().astype(bool)
                self.mask = dict(zip((v.name for v in spec.trainable), W.split_flat(flat, spec.trainable)))
            return
        held = self._held
        if held is None:
            return
        if held["mask"] is not None:                          # a coord_desc_* phase: the trainable variables in arena order
            flat = held["mask"].cpu().numpy().astype(bool) if name == "curr_mask" else held["params"].cpu().numpy()
            value = W.split_flat(flat, spec.trainable)
        else:                                                 # full_model: every variable, all-ones masks
            every = W.unpack(spec, held["params"].cpu().numpy(), held["stats"].cpu().numpy())
            value = [every[k] for k in every.keys()] if name == "train_params" else [np.ones_like(every[k], dtype=bool) for k in every.keys()]
        setattr(self, name, value)

    def _hold_phase(self, train_strategy, mask_dev):
        """End of a device_masks phase: what curr_mask / train_params / delta_payload are made from, without a copy to the host."""
        eng = self.engine
        held = self._held or {"params": torch.empty_like(eng.params), "stats": None}
        held["params"].copy_(eng.params)
        if mask_dev is None:
            if held["stats"] is None:
                held["stats"] = torch.empty_like(eng.stats)
            held["stats"].copy_(eng.stats)
        held["mask"], held["strategy"] = mask_dev, train_strategy
        self._held = held
        del self.curr_mask, self.train_params

    # ------------------------------------------------------------------ variables (SaveHelper semantics)
    def _restore_dict(self, variables: Dict[str, np.ndarray]) -> None:
        kept = {k: v for k, v in variables.items() if self.filter(k) is not None}
        self.engine.load_variables(kept)

    def restore_initial(self):
        """Reload ``<meta_dir>.npy``; optimizer state (Adam moments, step count) is NOT reset."""
        self._restore_dict(self._initial)

    def restore(self, chk):
        if isinstance(chk, str):
            chk = load_npy(chk)
        elif not isinstance(chk, dict):
            raise SystemExit(1)
        self._restore_dict(chk)

    def get_vars(self):
        out = self.engine.get_variables()
        if not self.frozen:
            trainable = self.engine.spec.trainable
            moments = (W.split_flat(self.engine.adam_m.cpu().numpy(), trainable), W.split_flat(self.engine.adam_v.cpu().numpy(), trainable))
            for var, m, v in zip(trainable, *moments):
                out[var.name[:-2] + "/Adam:0"], out[var.name[:-2] + "/Adam_1:0"] = m.copy(), v.copy()
            t = self.engine.adam_step
            out["beta1_power:0"] = np.float32(0.9 ** (t + 1))
            out["beta2_power:0"] = np.float32(0.999 ** (t + 1))
        return out

    def _model_vars(self) -> Dict[str, np.ndarray]:
        return self.engine.get_variables()

    # ------------------------------------------------------------------ inference
    def _mode(self) -> int:
        return hip.MODE_FROZEN if self.frozen else hip.MODE_LIVE

    def _run_pass(self, frames, labels_teacher, views=None, confidence=False, soft_logits=None, soft_layout=None) -> _Pass:
        """One inference pass and what is launched behind it on the same stream: every synchronous host-returning call is this, under
        ``process_lock``.  The engine has ONE output block, one uint8 label view and one set of low-resolution logits: the order below is fixed."""
        eng = self.engine
        # 1. a pass of the asynchronous pipeline that is still on the GPU leaves the output block first: ``collect`` later returns ITS metrics
        self._pipeline.drain()
        # 2. the pass (returns at once; the labels leave as uint8)
        labels_dev, _conf, _loss = eng.predict_frames(frames, labels_teacher, self._mode(), u8=True)
        frames_dev, teacher_dev = eng.last_inputs()
        rendered = certain = None
        # 3. one render launch: it reads the label view, the frames and the teacher labels where they are on the device, before anything
        #    else writes the label view
        if views is not None:
            rendered = self._get_renderer().render(frames_dev, labels_dev, teacher_dev, views)
        # 4. one confidence launch, before the next pass overwrites the logits; its statistics rows start towards a pinned host block (made on
        #    first use) BEFORE the one synchronisation, so they arrive with the pass's results
        if confidence:
            conf_map, _f32, stats_dev = eng.confidence(teacher_dev)
            if self._confidence_host is None:
                self._confidence_host = torch.empty((eng.max_batch, stats_dev.shape[1]), dtype=torch.int64).pin_memory()
            rows = self._confidence_host[:stats_dev.shape[0]]
            rows.copy_(stats_dev, non_blocking=True)
        #    ... and, with teacher logits, one soft-metric launch under the same rule (it reads the same logits and writes only its own rows)
        if soft_logits is not None:
            soft_dev = eng.soft_metric(None, teacher_dev, soft_logits, layout=soft_layout)[0]
            if self._soft_host is None:
                self._soft_host = torch.empty((eng.max_batch, soft_dev.shape[1]), dtype=torch.int64).pin_memory()
            soft_rows = self._soft_host[:soft_dev.shape[0]]
            soft_rows.copy_(soft_dev, non_blocking=True)
        # 5. one device -> host copy for labels + confusion matrices + losses (they share the output block) and one synchronisation
        labels_student, confs, losses = eng.fetch_frames()
        # 6. the rows are valid now
        if confidence:
            certain = Confidence(conf_map, [ConfidenceStats(r, self.class_count) for r in rows.numpy().copy()])
        soft = SoftMetric.sum(soft_rows.numpy().copy()) if soft_logits is not None else None
        assert labels_student.shape == tuple(frames.shape[:-1] if hasattr(frames, 'shape') else np.shape(frames)[:-1])
        metrics = pass_metrics(confs.sum(axis=0), losses.sum(axis=0)) if labels_teacher is not None else None
        return _Pass(labels_student, metrics, rendered, certain, soft)

    def predict_input(self, frames):
        with self.process_lock:
            return self._run_pass(frames, None).labels

    infer = predict_input

    def calc_cross_miou(self, labels):
        assert not self.frozen or self.cross_miou_compat
        assert labels.shape == (2, self.height, 2 * self.height)
        with self.process_lock:
            conf_mat_ = self.engine.cross_confusion(labels).cpu().numpy().astype(np.float64)
            iou_ = calculate_miou(conf_mat_, nan=True)
            miou_ = np.nanmean(iou_)
        return conf_mat_, iou_, miou_

    def predict_with_metric(self, frames, labels_teacher):
        with self.process_lock:
            return self._run_pass(frames, labels_teacher).result()

    def predict_rendered(self, frames, labels_teacher=None, views=RENDER_VIEWS, confidence=False):
        """One inference pass and one render launch behind it on the same stream (an addition; the reference paints on the host after the
        call, run.py:441-454).  The launch reads the pass's uint8 label view, the frames and the teacher labels where they are on the device.
        Returns what ``predict_with_metric`` returns (``predict_input`` when ``labels_teacher`` is None: the labels alone), bit for bit, plus a
        ``RenderedViews`` dict: view name -> uint8 device tensor [B,H,W,3] (``.host()``: all of them in one copy).  ``confidence=True``: the
        confidence launch of ``predict_with_confidence`` behind the same pass too, its ``Confidence`` as one more element at the end."""
        with self.process_lock:
            p = self._run_pass(frames, labels_teacher, views if views is not None else (), confidence)      # no views: the renderer refuses
        return p.result(p.rendered, p.confidence) if confidence else p.result(p.rendered)

    def predict_with_confidence(self, frames, labels_teacher=None):
        """One inference pass and one confidence launch behind it on the same stream: the student graph's ``probabilities_reduced``
        (utils/graph_utils.py:388-389), which the reference builds and no caller of it fetches.  Returns what ``predict_with_metric`` returns
        (``predict_input`` when ``labels_teacher`` is None: the labels alone), bit for bit, plus a ``Confidence``: ``.map`` the uint8 device
        tensor [B,H,W] = rint(p * 255) and ``.stats`` one ``ConfidenceStats`` per frame (calibration fields only with teacher labels)."""
        with self.process_lock:
            p = self._run_pass(frames, labels_teacher, confidence=True)
        return p.result(p.confidence)

    def predict_probabilities(self, frames):
        """``student['probabilities_reduced']`` of the reference's graph: f32 ndarray [B,H,W], per pixel the largest softmax value over the
        selected classes."""
        with self.process_lock:
            self._pipeline.drain()
            self.engine.predict_frames(frames, None, self._mode(), u8=True)
            return self.engine.confidence(None, f32=True)[1].cpu().numpy()

    def predict_with_soft_metric(self, frames, labels_teacher, teacher_logits):
        """One inference pass and one soft-metric launch behind it on the same stream: what a ``soft_teacher=True`` graph of the reference
        reports as ``student['loss']`` (utils/graph_utils.py:375-376, 403-408) and its ``prob_confmat`` / ``prob_confmat_star``
        (:265-317), evaluated without an optimisation step.  ``teacher_logits``: f32 [B, th, tw, TOTAL_CLASSES] with th <= H, tw <= 2H (host
        array or device tensor), or [B, th, tw, K] = the network's own classes alone, in the order of its class index list (the selected
        layout; the same bits); ``soft_teacher`` need not be set.  Returns what ``predict_with_metric`` returns, bit for bit, plus one
        ``SoftMetric`` over the frames of the call (``.row``: their summed integer row)."""
        layout = self._logits_layout(teacher_logits, len(frames))
        with self.process_lock:
            p = self._run_pass(frames, labels_teacher, soft_logits=teacher_logits, soft_layout=layout)
        return p.result(p.soft)

    def _logits_layout(self, teacher_logits, batch: int) -> str:
        """The layout of explicit teacher logits, by their last dimension: TOTAL_CLASSES channels are the full layout, K != TOTAL_CLASSES
        channels the selected one."""
        shape = tuple(teacher_logits.shape)
        assert len(shape) == 4 and shape[0] == batch and shape[-1] in (self.TOTAL_CLASSES, self.class_count), \
            "teacher_logits must be [%d, th, tw, %d] or, reduced to the network's classes, [%d, th, tw, %d], got %s" \
            % (batch, self.TOTAL_CLASSES, batch, self.class_count, shape)
        return "full" if shape[-1] == self.TOTAL_CLASSES else "selected"

    def _memory_layout(self, memory) -> str:
        """The layout of a DeviceReplayMemory's cached logits; a memory that selected other channels than this network's is refused (the
        kernels would take channel k for class k of THIS network)."""
        if memory.logits_select is not None:
            own = [int(c) for c in self.class_indices_graph]
            assert list(memory.logits_select) == own, \
                "the replay memory caches the teacher-logit channels logits_select = %s, this network's class index list is %s" \
                % (list(memory.logits_select), own)
        return memory.logits_layout

    def predict_soft_probabilities(self, frames, teacher_logits):
        """The per-pixel values behind ``predict_with_soft_metric``: (f32 ndarray [B,H,W,K] = the teacher's distribution over the selected
        classes, ``filtered_teacher_labels_probs``; f32 ndarray [B,H,W] = the pixel's soft cross-entropy against the student)."""
        layout = self._logits_layout(teacher_logits, len(frames))
        with self.process_lock:
            self._pipeline.drain()
            self.engine.predict_frames(frames, None, self._mode(), u8=True)
            _rows, p, ce = self.engine.soft_metric(None, None, teacher_logits, want_maps=True, layout=layout)
            return p.cpu().numpy(), ce.cpu().numpy()

    def evaluate_memory(self, memory, slots=None):
        """The soft-teacher loss and both confusion matrices over a ``DeviceReplayMemory`` built with ``logits_shape``, without stepping: the
        call to make before a model is published.  The frames are taken as stored (no rescale, crop or flip: the memory's frames have the
        network's size), ``max_batch`` at a time, gathered on the device.  ``slots``: logical indices (0 = the oldest), None = all.  Returns
        (``SoftMetric`` summed over the slots, hard confusion matrix float64 [K,K] summed over them); one synchronisation per pass."""
        assert isinstance(memory, DeviceReplayMemory), "evaluate_memory walks a DeviceReplayMemory"
        if memory.logits_shape is None:
            raise ValueError("evaluate_memory needs the teacher logits: construct the DeviceReplayMemory with logits_shape")
        eng = self.engine
        layout = self._memory_layout(memory)
        assert (memory.src_h, memory.src_w) == (eng.height, eng.width), "the memory's frames must be [%d, %d]" % (eng.height, eng.width)
        slots = np.arange(len(memory), dtype=np.int64) if slots is None else np.asarray(slots, dtype=np.int64).reshape(-1)
        assert slots.size > 0, "no slot to evaluate"
        table = np.zeros((slots.size, SAMPLE_FIELDS), dtype=np.int32)
        table[:, 0], table[:, 1], table[:, 2] = slots, memory.src_h, memory.src_w          # (slot, th, tw, top, left, flip): the copy case
        rows, conf = [], np.zeros((self.class_count, self.class_count), dtype=np.int64)
        with self.process_lock:
            for first in range(0, slots.size, eng.max_batch):
                frames, labels, logits = memory.plan(table[None, first:first + eng.max_batch], eng.height, eng.width).batch(0)
                p = self._run_pass(frames, labels, soft_logits=logits, soft_layout=layout)
                rows.append(p.soft.row)
                conf += p.metrics[0].astype(np.int64)
        return SoftMetric.sum(rows), conf.astype(np.float64)

    def _get_renderer(self):
        """The render tables of this network, built and uploaded once."""
        if self._renderer is None:
            self._renderer = DeviceRenderer(self.color_map_reduced_, colormap(), self.take_array, self.TOTAL_CLASSES, self.engine.device)
        return self._renderer

    # The edge's per-frame call, pipeline_depth frames at a time (an addition: the reference's call is synchronous): ams_amd/edge_pipeline.py.
    # Each frame's result is what predict_with_metric returns for it, bit for bit.  ``render=views`` paints that frame's views right behind its
    # pass, ``confidence=True`` adds the confidence launch; ``take_rendered`` / ``take_confidence`` hand them over, ``collect`` keeps its 5-tuple.
    def predict_with_metric_async(self, frames, labels_teacher, render=None, confidence=False):
        assert self.frozen and self.pipeline_depth > 1, "construct the frozen network with pipeline_depth >= 2"
        assert np.shape(frames)[0] == 1 and np.shape(labels_teacher)[0] == 1, "one frame per call"
        with self.process_lock:
            return self._pipeline.submit(frames, labels_teacher, render, confidence)

    def collect(self, ticket):
        with self.process_lock:
            return self._pipeline.collect(ticket)

    def take_rendered(self, ticket):
        """The views of a frame submitted with ``render=``: a ``RenderedViews`` dict of device tensors [1,H,W,3] (once per ticket; before or
        after ``collect``).  A frame that is still queued is launched first."""
        with self.process_lock:
            return self._pipeline.take_rendered(ticket)

    def take_confidence(self, ticket):
        """The ``Confidence`` of a frame submitted with ``confidence=True``: map [1,H,W] on the device, one ``ConfidenceStats`` (once per
        ticket; before or after ``collect``).  A frame that is still queued is launched first."""
        with self.process_lock:
            return self._pipeline.take_confidence(ticket)

    # ------------------------------------------------------------------ training
    def train_with_deque(self, frame_deque, label_deque, num_of_iterations, train_strategy='full_model',
                         keep_mask=False, teacher_logits_deque=None):
        """``teacher_logits_deque`` (soft_teacher=True only; the reference's _train never feeds teacher_labels_logits_pl, so its soft graph cannot
        run through this method at all): the cached teacher logits of the replay memory, one f32 [th, tw, TOTAL_CLASSES] array per frame of
        ``frame_deque`` (or [th, tw, K]: the network's classes alone, in the order of its class index list, uploaded as they are); a
        mini-batch takes the logits of the frames it drew.

        ``frame_deque`` may be an ``ams_amd.replay.DeviceReplayMemory`` (``label_deque`` and ``teacher_logits_deque`` are then None; with
        ``soft_teacher=True`` the logits come from the memory: cached at the frame size they are rescaled, cropped and flipped with the frames,
        cached on a smaller grid they follow whole frames only, as on the host path).  That path starts no helper thread and uses no pinned
        staging: the calling thread draws the phase's descriptors (``replay.draw_samples``, all iterations), uploads them once, and per iteration launches the gather
        on the engine's stream into one resident batch buffer before the same ``engine.train_step``; everything after the step is shared with
        the host path.  Order of the random draws: the sample descriptors of the whole phase FIRST, then ``get_train_mask``.  On the host path
        that order is a race between the sampler thread and ``get_train_mask`` (in the reference too), so the two paths are bit-identical,
        given equal seeds, for the strategies whose mask draws nothing: ``full_model`` and ``coord_desc_auto``."""
        assert not self.frozen, "Can't train frozen graph!!!"
        on_memory = isinstance(frame_deque, DeviceReplayMemory)
        if on_memory:
            assert label_deque is None and teacher_logits_deque is None, "a DeviceReplayMemory carries its labels and teacher logits itself"
            assert (frame_deque.logits_shape is not None) == self.soft_teacher, \
                "soft_teacher=True goes with a memory constructed with logits_shape (and needs one)"
        else:
            assert (teacher_logits_deque is not None) == self.soft_teacher, \
                "teacher_logits_deque goes with soft_teacher=True (and is required then)"
        if teacher_logits_deque is not None:
            assert len(teacher_logits_deque) == len(frame_deque), "one teacher-logit array per frame of the replay memory"
        if not keep_mask:
            self.mask = None
        with self.process_lock:
            feed = None if on_memory else self._host_feed()
            try:
                if feed is not None:
                    feed.start(num_of_iterations, frame_deque, label_deque, teacher_logits_deque)
                self._train(frame_deque if on_memory else feed, num_of_iterations, train_strategy)
            finally:
                if feed is not None:
                    feed.stop()                     # both helper threads joined, whatever happened, before the lock is released
        if feed is not None and feed.error is not None:
            raise feed.error                        # a helper's own exception (the reference would hang with the lock held)

    def _checked_loss_weights(self, class_weights, conf_gamma):
        """The K weights as f32 (or None), after the assertion that the loss's knobs (these two, kd_temperature, kd_alpha) can be served."""
        problem = loss_knobs_problem(self.soft_teacher, self.kd_temperature, self.kd_alpha, conf_gamma, class_weights, self.class_count)
        assert problem is None, problem
        return None if class_weights is None else np.asarray(class_weights, dtype=np.float32).reshape(-1)

    def set_loss_weights(self, class_weights=None, conf_gamma: float = 0.0) -> None:
        """``StudentEngine.set_loss_weights`` for the phases to come: K per-class weights (None = ones) and the exponent of the teacher's
        confidence (needs ``soft_teacher=True`` when > 0).  Training only; evaluation keeps reporting the unweighted losses."""
        assert not self.frozen, "Can't train frozen graph!!!"
        cw = self._checked_loss_weights(class_weights, float(conf_gamma))
        with self.process_lock:
            self.engine.set_loss_weights(cw, float(conf_gamma))
        self.loss_class_weights, self.kd_conf_gamma = cw, float(conf_gamma)

    def _checked_mining(self, top_k, warmup):
        """The warm-up as an int, after the assertion that the two mining knobs can be served."""
        problem = loss_knobs_problem(self.soft_teacher, self.kd_temperature, self.kd_alpha, loss_top_k=top_k, loss_top_k_warmup=warmup)
        assert problem is None, problem
        return int(warmup)

    def set_loss_mining(self, top_k: float = 1.0, warmup: int = 0) -> None:
        """Hard-pixel mining for the phases to come: iteration ``it`` of a phase keeps the hardest ``utils.mining_fraction(top_k, warmup, it)``
        of the valid pixels (``StudentEngine.set_loss_mining``).  ``1.0`` is off.  Training only; evaluation stays unmined."""
        assert not self.frozen, "Can't train frozen graph!!!"
        warmup = self._checked_mining(float(top_k), warmup)
        self.loss_top_k, self.loss_top_k_warmup = float(top_k), warmup

    def _host_feed(self) -> HostBatchFeed:
        """The helper threads and pinned staging ring of training from host deques (ams_amd/batch_feed.py), kept from phase to phase; made
        on first use and again when the instance's batch geometry changed since."""
        f = self._feed
        if f is None or f.mini_batch_size != self.mini_batch_size or list(f.scale) != list(self.scale):
            f = self._feed = HostBatchFeed(self.height, self.mini_batch_size, self.scale, self.engine.device)
        return f

    def train_step(self, frames, labels_teacher, train_strategy='full_model', teacher_logits=None):
        """North-star alias: ONE optimisation step on an explicit batch; returns the loss (float).  With ``soft_teacher=True`` the cached teacher
        logits of the batch are fed as ``teacher_logits`` f32 [B, th, tw, TOTAL_CLASSES] — what a caller of the reference puts into
        ``feed_dict[student['teacher_labels_logits_pl']]`` (th x tw = the label size, or a smaller cached grid: include/ams_hip.h) — or as
        [B, th, tw, K], the network's classes alone (the selected layout: the same loss and update, bit for bit)."""
        assert not self.frozen, "Can't train frozen graph!!!"
        assert (teacher_logits is not None) == self.soft_teacher, "teacher_logits go with soft_teacher=True (and are required then)"
        layout = self._logits_layout(teacher_logits, len(frames)) if teacher_logits is not None else None
        with self.process_lock:
            mask_dev = None
            if 'coord_desc_' in train_strategy:
                _before, train_mask_ = self.get_train_mask(train_strategy)
                mask_dev = self._mask_to_device(train_mask_)
            ls = self.engine.train_step(frames, labels_teacher, self.lr, mask_dev, teacher_logits=teacher_logits,
                                        teacher_logits_layout=layout).cpu().numpy()
        return float(ls[0] / ls[1]) if ls[1] > 0 else float("nan")

    def _mask_to_device(self, train_mask_: Dict[str, np.ndarray]) -> torch.Tensor:
        flat = np.empty(self.engine.spec.n_trainable, dtype=np.uint8)
        W.fill_flat(flat, self.engine.spec.trainable, train_mask_)
        return torch.from_numpy(flat).to(self.engine.device)

    def _train(self, source, num_of_iterations, train_strategy):
        """``source``: a DeviceReplayMemory, or a started HostBatchFeed."""
        plan = feed = logits_layout = None                          # (no layout named: the engine tells it by the last dimension)
        if isinstance(source, DeviceReplayMemory):
            logits_layout = self._memory_layout(source)
            plan = self._replay_plan(source, num_of_iterations)        # the phase's draws, before get_train_mask; no helper thread
        else:
            feed = source

        on_device = self.device_masks
        before_dev = None
        if on_device:
            before_dev, mask_dev = self._device_train_mask(train_strategy)
        else:
            _before, train_mask_ = self.get_train_mask(train_strategy)
            mask_dev = self._mask_to_device(train_mask_) if train_mask_ is not None else None
        losses = []
        mined, frac = getattr(self, "loss_top_k", 1.0) < 1.0, 1.0          # (a subclass that skips __init__ trains unmined)
        self.last_mining = None
        t_phase = time.time()
        for it in range(num_of_iterations):
            if feed is not None:
                staged = feed.next_staged()
                if staged is None:                  # a helper died: its exception is raised by train_with_deque
                    if mined:
                        self.engine.set_loss_mining(1.0)
                    return
            t1 = time.time()
            if mined:                               # host code: the fraction this iteration keeps (iteration 0 of a warm-up is unmined)
                frac = mining_fraction(self.loss_top_k, self.loss_top_k_warmup, it)
                self.engine.set_loss_mining(frac)
            if plan is not None:
                frames_dev, labels_dev, logits_dev = plan.batch(it)       # one launch on this stream into the resident batch buffer
            else:
                frames_dev, labels_dev, logits_dev = feed.consume(staged)
            if logits_dev is not None and logits_layout == "selected":
                loss_dev = self.engine.train_step(frames_dev, labels_dev, self.lr, mask_dev, teacher_logits=logits_dev,
                                                  teacher_logits_layout=logits_layout)
            elif logits_dev is not None:
                loss_dev = self.engine.train_step(frames_dev, labels_dev, self.lr, mask_dev, teacher_logits=logits_dev)
            else:
                loss_dev = self.engine.train_step(frames_dev, labels_dev, self.lr, mask_dev)
            losses.append(loss_dev)
            if self.verbose:
                ls = loss_dev.cpu().numpy()
                print('Loss is %.3f at iteration %d and took %.1f ms' % (ls[0] / ls[1] if ls[1] > 0 else float('nan'), it,   # ls[1]: the weight sum, maybe < 1
                                                                         (time.time() - t1) * 1000.0))
            if on_device:
                if it == 0 and before_dev is not None:
                    # the same selection on the device: two order statistics of |delta w| come back, the threshold is np.percentile's
                    mask_dev, kept = self.engine.select_changed(before_dev, self.coord_frac)
                    before_dev = None
                    if self.verbose:
                        print("Using auto mode, Training %.3f%% of variables" % (100 * int(kept.item()) / mask_dev.numel()))
                    del self.mask
                    self._auto_mask_dev = mask_dev
            elif train_strategy == 'coord_desc_auto':
                if it == 0 and self.mask is None:
                    # derive the mask from the first step's |delta w|: keep the top coord_frac, roll back the rest
                    _after = self._model_vars()
                    names = [v.name for v in self.engine.spec.trainable]
                    changes = np.concatenate([np.abs(_after[k] - _before[k]).reshape(-1) for k in names], axis=0)
                    cut_threshold = np.percentile(changes, 100 * (1 - self.coord_frac))
                    _combine = {}
                    kept = total = 0
                    for k in names:
                        train_mask_[k] = np.abs(_after[k] - _before[k]) > cut_threshold
                        kept += int(np.sum(train_mask_[k]))
                        total += train_mask_[k].size
                        _combine[k] = np.where(train_mask_[k], _after[k], _before[k])
                    if self.verbose:
                        print("Using auto mode, Training %.3f%% of variables" % (100 * kept / total))
                    self._restore_dict(_combine)
                    self.mask = train_mask_
                    mask_dev = self._mask_to_device(train_mask_)
        if mined:
            if frac < 1.0:
                self.last_mining = self.engine.mining_result()         # of the phase's last iteration
            self.engine.set_loss_mining(1.0)                           # steps outside a phase (train_step) stay unmined
        stacked = torch.stack(losses).cpu().numpy() if losses else np.zeros((0, 2))
        self.last_losses =[float(s / c) if c > 0 else float("nan") for s, c in stacked]
        self._last_train_ms = (time.time() - t_phase) * 1000.0

        if on_device:
            self._hold_phase(train_strategy, mask_dev)
            return
        self._held = None
        _after_train = self._model_vars()
        if 'coord_desc_' in train_strategy:
            names = [v.name for v in self.engine.spec.trainable]
            self.curr_mask = [np.asarray(train_mask_[k]) for k in names]
            self.train_params = [_after_train[k] for k in names]
        else:
            self.train_params = [_after_train[k] for k in _after_train.keys()]
            self.curr_mask = [np.ones_like(_after_train[k], dtype=bool) for k in _after_train.keys()]

    def _device_train_mask(self, train_strategy):
        """device_masks=True: (snapshot of the trainable arena or None, device mask or None) for a phase.  coord_desc_auto starts from an
        all-ones mask and a snapshot, or from the mask the previous phase selected (keep_mask=True); the table / Bernoulli strategies draw
        their masks on the host as ever (their random numbers are part of the contract) and upload them once."""
        if train_strategy == 'full_model':
            return None, None
        if train_strategy == 'coord_desc_auto':
            if self._auto_mask_dev is not None:
                return None, self._auto_mask_dev
            if self.mask is not None:          # a mask assigned by the caller
                return None, self._mask_to_device(self.mask)
            return self.engine.snapshot_params(), torch.ones(self.engine.spec.n_trainable, dtype=torch.uint8, device=self.engine.device)
        _before, train_mask_ = self.get_train_mask(train_strategy)
        return None, self._mask_to_device(train_mask_)

    def _replay_plan(self, memory, num_of_iterations):
        """A phase on a DeviceReplayMemory: mini_batch's draws for every iteration, on the calling thread, uploaded once."""
        crop = [self.height, self.height * 2]
        # soft targets follow the frames a batch drew: logits cached at the frame size through rescale, crop and flip (ams_replay_gather_logits),
        # logits cached on a smaller grid only where frames are taken as they are, unless the memory was built with logits_upsample: its grid
        # then stands for its align-corners upsample to the frame size (ams_replay_gather_logits_lowres)
        whole_frames = list(self.scale) == [1] and (memory.src_h, memory.src_w) == tuple(crop) and not self.flip
        assert memory.logits_shape is None or whole_frames or memory.logits_follow_frames, \
            LOW_RES_LOGITS % (memory.logits_shape[:2] + (memory.src_h, memory.src_w))
        samples = draw_samples(len(memory), (memory.src_h, memory.src_w), crop, self.scale, self.mini_batch_size, num_of_iterations,
                               flip=self.flip)
        return memory.plan(samples, crop[0], crop[1])

    def _delta_payload_q8(self, device, base_variables, track_edge):
        """delta_payload(fmt="q8"): always encoded on the device, whichever path the phase took."""
        eng = self.engine
        held = self._held
        with self.process_lock:
            if held is not None:
                layout, mask = delta_layout(eng.spec, held["strategy"]), held["mask"]
            else:
                assert self.curr_mask is not None, "no training phase has run yet"
                layout = delta_layout(eng.spec, "coord_desc_rand" if len(self.curr_mask) == len(eng.spec.trainable) else "full_model")
                assert [m.size for m in self.curr_mask] == [e.count for e in layout.entries], "curr_mask does not follow a delta layout"
                flat = np.concatenate([np.asarray(m).reshape(-1) for m in self.curr_mask]).astype(np.uint8)
                mask = None if flat.all() else torch.from_numpy(flat).to(eng.device)          # NULL = every element
            if base_variables is not None:
                eng.set_delta_base(base_variables)
                self._q8_tracked = False
            elif not self._q8_tracked:
                eng.set_delta_base({k: v for k, v in self._initial.items() if self.filter(k) is not None})
            dev = eng.encode_delta(layout, mask, fmt="q8", advance_base=track_edge)
            self._q8_tracked = self._q8_tracked or bool(track_edge)
            return dev if device else dev.cpu().numpy().tobytes()

    def delta_payload(self, device: bool = False, fmt: str = "fp16", base_variables=None, track_edge: bool = False):
        """The downlink model delta of reference run.py:316-336 as bytes: per variable ``np.packbits(mask.flatten())``, then
        per variable the masked parameters as fp16.  Under the coordinate-descent strategies (``train_params`` = the
        trainable variables, in arena order) the value part is gathered and cast on the device by ``ams_pack_masked_fp16``;
        otherwise (``full_model``: every model variable incl. BN statistics) it is the reference's host loop.

        After a ``device_masks=True`` phase the whole payload, mask bits included, is encoded on the device from the phase's device mask and the
        engine's current variables (``ams_student_encode_delta``; call it before the model changes again, as run.py does) and comes to the
        host in one copy.  ``device=True`` returns the payload as a uint8 device tensor instead, which ``apply_delta`` accepts.

        ``fmt="q8"`` (an addition; fp16 is the reference's format and the default): after the same mask bits, one f32 scale per variable and one
        int8 code of (value - base) per masked element, always encoded on the device (``ams_student_encode_delta_q8``).  The base is
        ``base_variables``, by default the checkpoint ``restore_initial`` loads.  ``track_edge=True`` serves continual training (run.py
        --no_restore): after encoding, the base's masked elements become what the edge decodes, and later calls encode against that
        tracked base, so each update's quantisation error is carried into the next instead of accumulating on the edge."""
        if check_format(fmt) == "q8":
            return self._delta_payload_q8(device, base_variables, track_edge)
        assert base_variables is None and not track_edge, "base_variables / track_edge belong to the q8 format"
        held = self._held
        if held is not None:
            with self.process_lock:
                dev = self.engine.encode_delta(delta_layout(self.engine.spec, held["strategy"]), held["mask"])
                return dev if device else dev.cpu().numpy().tobytes()
        if device:
            return torch.from_numpy(np.frombuffer(self.delta_payload(), dtype=np.uint8).copy()).to(self.engine.device)
        assert self.curr_mask is not None and self.train_params is not None, "no training phase has run yet"
        payload = bytearray()
        for val in self.curr_mask:
            payload += np.packbits(val.flatten()).tobytes()
        trainable = self.engine.spec.trainable
        on_device = len(self.curr_mask) == len(trainable) and all(m.size == v.size for m, v in zip(self.curr_mask, trainable))
        if on_device:
            flat = np.concatenate([m.reshape(-1) for m in self.curr_mask]).astype(np.uint8)
            with self.process_lock:
                halves = self.engine.pack_masked_fp16(torch.from_numpy(flat).to(self.engine.device))
                payload += halves.cpu().numpy().tobytes()
        else:
            for p_, m_ in zip(self.train_params, self.curr_mask):
                assert p_.shape == m_.shape
                payload += p_[m_].astype(np.float16).tobytes()
        return bytes(payload)

    def apply_delta(self, payload, train_strategy, base_variables=None, fmt: str = "fp16") -> int:
        """The edge half of the downlink (an addition: the reference's edge reloads the server's full model, run.py:401-411): decode a
        ``delta_payload`` of a server running ``train_strategy`` into this network's variables on the device and, on a frozen instance,
        re-freeze (which repeats the fp16 range check).  ``base_variables`` (a {name: array} dict, e.g. the initial model's) are loaded
        first, so that the update lands on the model the server started from; None applies it to the current model.  Returns the number of
        values applied.  A malformed payload raises AmsHipError and leaves the model as it was (including a base loaded for it).

        Frames submitted with ``predict_with_metric_async`` before this call are answered by the old model, frames submitted after it by the
        new one: the queued ones are launched and fetched first.

        ``fmt="q8"``: the payload carries changes, added to the base (``base_variables``, or the current model when None)."""
        layout = delta_layout(self.engine.spec, train_strategy)
        with self.process_lock:
            self._pipeline.flush()
            eng = self.engine
            saved = None
            if base_variables is not None:
                saved = (eng.params.clone(), eng.stats.clone())
                eng.load_variables(base_variables)
                eng._updated_since_freeze = True
            try:
                n = eng.apply_delta(payload, layout, fmt)
            except hip.AmsHipError:
                if saved is not None:
                    eng.params.copy_(saved[0])
                    eng.stats.copy_(saved[1])
                    eng._updated_since_freeze = False
                raise
            if self.frozen:
                eng.freeze()
        return n

    def get_train_mask(self, train_strategy):
        """Coordinate-descent masks (SemanticNetwork.py:302-669): dict variable name -> bool array, or None."""
        if train_strategy == 'full_model':
            return None, None
        _before = {v.name: None for v in self.engine.spec.trainable}
        shapes = {v.name: v.shape for v in self.engine.spec.trainable}
        if train_strategy == 'coord_desc_auto':
            _before = {k: v for k, v in self._model_vars().items() if k in shapes}
            if self.mask is None:
                train_mask_ = {k: np.ones(shapes[k], dtype=bool) for k in shapes}
            else:
                train_mask_ = self.mask
            return _before, train_mask_
        train_mask_ = coord_masks.build_mask(train_strategy, self.coord_frac, shapes)   # raises NameError if unknown
        if self.verbose:
            all_vars, train_vars_len = self.train_vars_count(train_mask_)
            print("Using %s mode, Training %.3f%% of variables" % (train_strategy, 100 * train_vars_len / all_vars))
        return _before, train_mask_

    def train_vars_count(self, train_mask_):
        all_vars = sum(m.size for m in train_mask_.values())
        train_vars_len = sum(int(np.sum(m)) for m in train_mask_.values())
        return all_vars, train_vars_len

    # ------------------------------------------------------------------ freeze / export
    def get_frozen_graph(self):
        return FrozenGraph(self._model_vars(), self.class_indices_graph, self.height, self.TOTAL_CLASSES)

    def save_to_frozen_graph(self, save_dir):
        graph_def = self.get_frozen_graph()
        with open(save_dir + ".pb", 'wb') as pb_file:
            pb_file.write(graph_def.SerializeToString())

    def close_model(self):
        self._pipeline.clear()             # views and confidence maps nobody took: their device memory goes with the engine
        self.engine.close()

    # ------------------------------------------------------------------ visualisation helpers
    # Same signatures and return conventions as the reference (SemanticNetwork.py:719-755); bodies are this build's own:
    # palettes are looked up through one helper, the 50/50 overlay is integer arithmetic (cv2.addWeighted rounds half
    # to even on the float sum; so does _overlay), and the disagreement picture is built from boolean planes.
    # Routed by input type: host arrays take the NumPy bodies and return ndarrays; torch tensors are painted by k_render.hip on the engine's
    # device and return device tensors, equal bit for bit for labels in range (out of range: ams_amd/render.py).
    def _check_hw(self, arr, channels=None, what="array"):
        want = (self.height, 2 * self.height) + (() if channels is None else (channels,))
        assert tuple(arr.shape) == want, "%s must be %s, got %s" % (what, want, tuple(arr.shape))

    @staticmethod
    def _on_device(*arrays):
        return any(isinstance(a, torch.Tensor) for a in arrays)

    def _predict_device(self, frame):
        """Labels of one device frame as an int32 device tensor [H, W]; nothing goes through the host."""
        with self.process_lock:
            self._pipeline.drain()
            return self.engine.predict(frame[None], self._mode())[0]

    def _render_one(self, views, frame=None, student=None, teacher=None):
        b1 = lambda x: None if x is None else (x[None] if isinstance(x, torch.Tensor) else np.asarray(x)[None])     # noqa: E731
        with self.process_lock:
            out = self._get_renderer().render(b1(frame), b1(student), b1(teacher), views)
        return [out[v][0] for v in views]

    @staticmethod
    def _overlay(frame, colours):
        total = frame.astype(np.uint16) + colours.astype(np.uint16)           # 0..510
        half = total >> 1
        half += (total & 1) & (half & 1)                                      # x.5 -> nearest even, like rint
        return half.astype(np.uint8)

    def _paint(self, palette, label, frame):
        colours = np.asarray(palette)[np.asarray(label)]
        return colours if frame is None else (colours, self._overlay(frame, colours))

    def colorize(self, frame=None, label=None):
        assert frame is not None or label is not None, "At least a label or frame must be given"
        if frame is not None:
            self._check_hw(frame, 3, "frame")
        if self._on_device(frame, label):
            if label is None:
                label = self._predict_device(frame)
            self._check_hw(label, None, "label")
            if frame is None:
                return self._render_one(("colour_student",), student=label)[0]
            return tuple(self._render_one(("colour_student", "overlay_student"), frame=frame, student=label))
        if label is None:
            label = self.predict_input(frame[None])[0]
        self._check_hw(label, None, "label")
        return self._paint(self.color_map_reduced_, label, frame)

    def colorize_teacher(self, label, frame=None):
        if frame is not None:
            self._check_hw(frame, 3, "frame")
        self._check_hw(label, None, "label")
        if self._on_device(frame, label):
            if frame is None:
                return self._render_one(("colour_teacher",), teacher=label)[0]
            return tuple(self._render_one(("colour_teacher", "overlay_teacher"), frame=frame, teacher=label))
        return self._paint(colormap(), label, frame)

    def cross_ignore(self, label_teacher, label_student=None, frame_student=None):
        """(cross_mask, ignore_mask): where teacher and student disagree (teacher colour, black elsewhere) and which
        pixels the metric skips (white).  As in the reference, subset index 0 doubles as 'ignored'."""
        assert label_student is not None or frame_student is not None, \
            "At least a label or frame from student must be given"
        self._check_hw(label_teacher, None, "label_teacher")
        if self._on_device(label_teacher, label_student, frame_student):
            if label_student is None:
                label_student = self._predict_device(frame_student if isinstance(frame_student, torch.Tensor) else torch.from_numpy(frame_student))
            self._check_hw(label_student, None, "label_student")
            return tuple(self._render_one(("cross_mask", "ignore_mask"), student=label_student, teacher=label_teacher))
        if label_student is None:
            label_student = self.predict_input(frame_student[None])[0]
        self._check_hw(label_student, None, "label_student")
        teacher_k = self.take_array[label_teacher]
        skipped = teacher_k == 0
        ignore_mask = np.zeros(teacher_k.shape + (3,), dtype=np.uint8)
        ignore_mask[skipped] = self.WHITE
        differs = ~skipped & (teacher_k != label_student)
        cross_mask = np.zeros_like(ignore_mask)
        cross_mask[differs] = self.color_map_reduced_[teacher_k[differs]]
        return cross_mask, ignore_mask
