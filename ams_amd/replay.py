"""The server's replay memory on the device (reference run.py:136-137: ``frame_memory`` / ``label_memory``, two host deques) and the
mini-batch sampler that reads it there (reference utils/utils.py:129-185, ``mini_batch``).

    memory = DeviceReplayMemory(capacity, H, 2 * H, device)                  # a ring of uint8 slots in HBM, deque(maxlen=capacity) semantics
    memory.append(frame, label)                                              # host arrays or device tensors (FrameIngest's: no host hop)
    network.train_with_deque(memory, None, iterations, 'coord_desc_auto')    # no helper thread, no pinned staging
    phis = [r[2] for r in memory.cross_miou_pairs(network, first)]           # ASR's phi-score: one launch, one device -> host copy

The random numbers are the host generators', drawn in ``mini_batch``'s order (``draw_samples``): which frames a seeded run trains on does not
depend on where the memory lives.  What the draws select is built by one launch per mini-batch (``ams_replay_gather``, k_replay.hip), bit for
bit what ``mini_batch`` returns for them: the crop of the rescaled frame (cv2.resize's 8-bit INTER_LINEAR; INTER_NEAREST for the label),
mirrored when flipped.  Teacher logits cached at the frame size follow the frame through the same descriptors (``ams_replay_gather_logits``:
this project's rule, include/ams_hip.h; the reference never resamples logits); logits cached on a smaller grid follow whole frames only,
unless the memory is constructed with ``logits_upsample=True``: then a slot behaves, bit for bit, as a frame-size slot holding its own
align-corners upsample (the soft loss kernel's), evaluated inside the gather (``ams_replay_gather_logits_lowres``) and never stored.
One source geometry per memory (the frames of one video have one size); the host deques stay the answer for mixed
sizes.  ``logits_select=class_idx`` caches only the student's K channels of every frame's logits (the selected layout, AMS_TLOGITS_SELECTED:
the loss gathers exactly those, so nothing is lost and every result keeps its bits; K / classes of the memory, the upload and the gather
traffic).  A memory that caches logits needs no labels from the caller: ``append(frame, None, logits)`` derives the slot's hard labels from
the full logits on the device (``ams_teacher_labels_from_logits``: the argmax of their align-corners upsample, the teacher's own
``predictions``), so a 512x1024 sample uploads its 33x65x19 grid (163 KB) and no 512 KB label map.  No CPU fallback: the launches need the
HIP library and a GPU; the bookkeeping (``Ring``, ``draw_samples``, the byte budget) does not.
"""
from __future__ import annotations

import ctypes as C
import random
from typing import Optional, Sequence

import numpy as np
import torch

from . import hip
from .utils import calculate_miou

SAMPLE_FIELDS = 6            # ams_replay_sample: slot, th, tw, top, left, flip (int32 each)
SLOT_ALIGN = 256             # slots start at multiples of this many bytes: every 16-byte access of the copy case is aligned
LOW_RES_LOGITS = ("a low-resolution teacher-logit cache (%dx%d logits for %dx%d frames) follows whole frames only: scale == [1], frames at the "
                  "network size, no flip; cache the logits at the frame size to rescale, crop or flip them with the frames, or construct the "
                  "memory with logits_upsample=True (the cached grid then stands for its align-corners upsample to the frame size)")
LARGE_LOGITS = ("logits_upsample=True needs a teacher-logit grid no larger than the frame on either axis: %dx%d logits for %dx%d frames would be "
                "down-sampled, and only the align-corners upsample (the soft loss kernel's) is defined")


def draw_samples(n_mem: int, src_hw: Sequence[int], crop: Sequence[int], scale: Sequence[float], batch: int, iters: int,
                 flip: bool = False) -> np.ndarray:
    """The draws of ``utils.mini_batch`` for a memory of ``n_mem`` frames of one size ``src_hw``, without touching a frame: int32
    ``[iters, batch, 6]`` descriptors (slot, th, tw, top, left, flip) with LOGICAL slot indices (0 = the oldest frame).

    Consumes the global generators exactly as ``mini_batch`` does — per sample ``np.random.choice(n_mem)``, then ``random.randint`` for the
    scale choice, the row offset and the column offset, with ``flip`` one ``np.random.random()`` more — and keeps its two asserts on the
    slack.  (th, tw) = the size of the rescaled image the crop is cut from."""
    src_h, src_w = int(src_hw[0]), int(src_hw[1])
    crop_h, crop_w = crop[0], crop[1]
    out = np.empty((iters, batch, SAMPLE_FIELDS), dtype=np.int32)
    for it in range(iters):
        for j in range(batch):
            slot = np.random.choice(n_mem)
            s = scale[random.randint(0, len(scale) - 1)]
            factor = s * crop_w / src_w
            th, tw = int(src_h * factor), int(src_w * factor)
            slack_h = th - crop_h
            slack_w = tw - crop_w
            assert slack_w >= 0
            assert slack_h >= 0
            top = random.randint(0, slack_h)
            left = random.randint(0, slack_w)
            mirrored = bool(flip and np.random.random() > 0.5)
            out[it, j] = (slot, th, tw, top, left, int(mirrored))
    return out


class Ring:
    """Slot bookkeeping of ``collections.deque(maxlen=capacity)``: logical index 0 is the oldest element, appending to a full ring evicts it."""

    def __init__(self, capacity: int):
        assert capacity >= 1, "a replay memory holds at least one frame"
        self.capacity = int(capacity)
        self.head = 0            # physical slot of logical index 0
        self.count = 0

    def __len__(self) -> int:
        return self.count

    def push(self) -> int:
        """The physical slot the next element is written to."""
        if self.count < self.capacity:
            slot = (self.head + self.count) % self.capacity
            self.count += 1
            return slot
        slot = self.head
        self.head = (self.head + 1) % self.capacity
        return slot

    def clear(self) -> None:
        self.head = self.count = 0

    def physical(self, logical):
        """Logical index (an int, negative from the end as for a deque, or an integer array of non-negative ones) -> physical slot."""
        if isinstance(logical, np.ndarray):
            assert logical.size == 0 or (logical.min() >= 0 and logical.max() < self.count), "slot outside the memory"
            return (self.head + logical) % self.capacity
        i = int(logical)
        if i < 0:
            i += self.count
        if not 0 <= i < self.count:
            raise IndexError("replay memory index out of range")
        return (self.head + i) % self.capacity


def _round_up(n: int, to: int) -> int:
    return (n + to - 1) // to * to


def labels_to_u8(label):
    """The uint8 rule of ``StudentEngine._labels_to_device``: tf.cast(labels, int32) truncates toward zero; ids outside 0..254 -> 255."""
    if isinstance(label, torch.Tensor):
        if label.dtype == torch.uint8:
            return label
        ti = label.to(torch.int64)
        return torch.where((ti >= 0) & (ti < 255), ti, torch.full_like(ti, 255)).to(torch.uint8)
    a = np.asarray(label)
    if a.dtype != np.uint8:
        ai = a.astype(np.float32).astype(np.int64)
        a = np.where((ai >= 0) & (ai < 255), ai, 255).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(a))


class ReplayPlan:
    """One training phase's draws, uploaded once: ``batch(it)`` builds mini-batch ``it`` in the memory's resident batch buffer on the current
    stream and returns its device tensors (frames, labels, teacher logits or None).  Stream order keeps the buffer safe: the step that reads
    it and the next gather that overwrites it are enqueued on the same stream."""

    def __init__(self, memory: "DeviceReplayMemory", table_host: np.ndarray, H: int, W: int):
        self.memory, self.table_host, self.H, self.W = memory, table_host, H, W
        self.iters, self.batch_size = int(table_host.shape[0]), int(table_host.shape[1])
        self.table_dev = memory._upload(table_host)
        # whole frames: every draw takes a frame of the crop's size as it is.  Only then may the logits live on another grid than the frame's
        # (they are copied slot by slot, the path and the bits of a scale == [1] phase); otherwise they are resampled with the frame (a smaller
        # grid only on a memory with logits_upsample)
        self.whole_frames = (memory.src_h, memory.src_w) == (H, W) and bool((table_host[..., 1:] == (H, W, 0, 0, 0)).all())
        assert memory.logits_shape is None or self.whole_frames or memory.logits_follow_frames, \
            LOW_RES_LOGITS % (memory.logits_shape[:2] + (memory.src_h, memory.src_w))
        self.frames, self.labels, self.logits = memory._batch_buffers(self.batch_size, H, W, self.whole_frames)

    def batch(self, it: int):
        m = self.memory
        m._gather(self.table_host[it], self.table_dev[it], self.H, self.W, self.frames, self.labels)
        if self.logits is not None:
            m._gather_logits(self.table_host[it], self.table_dev[it], self.logits, None if self.whole_frames else (self.H, self.W))
        return self.frames, self.labels, self.logits


class DeviceReplayMemory:
    def __init__(self, capacity: int, src_h: int, src_w: int, device, logits_shape: Optional[Sequence[int]] = None,
                 max_bytes: Optional[int] = None, logits_select: Optional[Sequence[int]] = None, logits_upsample: bool = False):
        """``capacity`` slots of uint8 [src_h, src_w, 3] frames and uint8 [src_h, src_w] labels, with ``logits_shape`` = (th, tw, classes) also
        f32 teacher logits per slot (soft_teacher; (src_h, src_w, classes) lets them follow rescale, crop and flip, a smaller grid follows
        whole frames only, or with ``logits_upsample=True`` every descriptor too: the grid, no larger than the frame on either axis, then stands
        for its align-corners upsample to the frame size, formed inside the gather).  ``logits_select`` = the student's class index list: a slot keeps those K channels alone, in that order
        (``logits_cached_shape`` = (th, tw, K), ``logits_layout`` = "selected"); ``logits_shape`` stays what ``append`` is fed.  The bytes
        wanted are computed up front (``nbytes``; at 512x1024: 2 MB per slot, 42 MB with full-size logits of 19 classes, 14.6 MB with six
        selected) and ``MemoryError`` is raised above ``max_bytes`` before anything is allocated."""
        self.ring = Ring(capacity)
        self.capacity, self.src_h, self.src_w = int(capacity), int(src_h), int(src_w)
        assert self.src_h > 0 and self.src_w > 0
        self.device = torch.device(device)
        self.logits_shape = tuple(int(d) for d in logits_shape) if logits_shape is not None else None
        assert self.logits_shape is None or len(self.logits_shape) == 3, "logits_shape is (th, tw, classes)"
        self.logits_upsample = bool(logits_upsample)
        if self.logits_upsample:
            assert self.logits_shape is not None, "logits_upsample goes with logits_shape"
            assert 1 <= self.logits_shape[0] <= self.src_h and 1 <= self.logits_shape[1] <= self.src_w, \
                LARGE_LOGITS % (self.logits_shape[:2] + (self.src_h, self.src_w))
        self.frame_stride = _round_up(self.src_h * self.src_w * 3, SLOT_ALIGN)          # bytes
        self.label_stride = _round_up(self.src_h * self.src_w, SLOT_ALIGN)
        self.logits_select = tuple(int(c) for c in logits_select) if logits_select is not None else None
        if self.logits_select is not None:
            assert self.logits_shape is not None, "logits_select goes with logits_shape"
            assert 1 <= len(self.logits_select) <= 32, "logits_select names 1..32 classes, got %d" % len(self.logits_select)
            assert all(0 <= c < self.logits_shape[2] for c in self.logits_select), \
                "logits_select %s names a class outside 0..%d" % (list(self.logits_select), self.logits_shape[2] - 1)
            assert self.logits_shape[2] <= 256, "at most 256 classes"
        self.logits_layout = "selected" if self.logits_select is not None else "full"
        # what a slot holds: every class, or the selected ones
        self.logits_cached_shape = None
        if self.logits_shape is not None:
            self.logits_cached_shape = self.logits_shape[:2] + (len(self.logits_select) if self.logits_select is not None else self.logits_shape[2],)
        self.logits_stride = _round_up(4 * int(np.prod(self.logits_cached_shape)), SLOT_ALIGN) // 4 if self.logits_shape else 0     # f32 elements
        self.nbytes = self.capacity * (self.frame_stride + self.label_stride + 4 * self.logits_stride)
        if max_bytes is not None and self.nbytes > int(max_bytes):
            raise MemoryError("a replay memory of %d slots of %dx%d needs %d bytes, above max_bytes = %d"
                              % (self.capacity, self.src_h, self.src_w, self.nbytes, int(max_bytes)))
        self._frames = torch.empty(self.capacity * self.frame_stride, dtype=torch.uint8, device=self.device)
        self._labels = torch.empty(self.capacity * self.label_stride, dtype=torch.uint8, device=self.device)
        self._logits = torch.empty(self.capacity * self.logits_stride, dtype=torch.float32, device=self.device) if self.logits_shape else None
        self._buffers = None

    @property
    def logits_at_source(self) -> bool:
        """The teacher logits are cached at the frames' size: they can follow a frame through rescale, crop and flip."""
        return self.logits_shape is not None and self.logits_shape[:2] == (self.src_h, self.src_w)

    @property
    def logits_follow_frames(self) -> bool:
        """The teacher logits can follow a frame through rescale, crop and flip: cached at the frames' size, or on a smaller grid that stands
        for its upsample (``logits_upsample``)."""
        return self.logits_at_source or (self.logits_shape is not None and self.logits_upsample)

    # ------------------------------------------------------------------ deque(maxlen=capacity) surface
    def __len__(self) -> int:
        return len(self.ring)

    def clear(self) -> None:
        self.ring.clear()

    def _slot_views(self, p: int):
        f = self._frames[p * self.frame_stride:p * self.frame_stride + self.src_h * self.src_w * 3].view(self.src_h, self.src_w, 3)
        l = self._labels[p * self.label_stride:p * self.label_stride + self.src_h * self.src_w].view(self.src_h, self.src_w)
        if self._logits is None:
            return f, l
        n = int(np.prod(self.logits_cached_shape))
        return f, l, self._logits[p * self.logits_stride:p * self.logits_stride + n].view(self.logits_cached_shape)

    def __getitem__(self, i: int):
        """Device views (frame, label[, logits]) of logical element ``i`` (0 = the oldest); valid until the slot is evicted.  The logits have
        ``logits_cached_shape``."""
        return self._slot_views(self.ring.physical(i))

    def append(self, frame, label, logits=None) -> None:
        """Host arrays or device tensors; a device tensor (e.g. ``FrameIngest``'s) is stored by a device copy on the current stream.  Past the
        capacity the oldest element is evicted.  Labels go through the uint8 rule of ``StudentEngine._labels_to_device``.

        A memory with ``logits_select`` takes full logits (``logits_shape``) or logits already reduced (``logits_cached_shape``): full logits
        on the device go through ``ams_replay_pack_logits`` on the current stream, a full host array is reduced on the host (``np.take``)
        so that only the K channels are uploaded, reduced logits are stored as they are.

        ``label=None`` (a memory with ``logits_shape`` only): the label slot is derived from the logits on the device, on the current stream
        (``ams_teacher_labels_from_logits``: the argmax over every class of the logits' align-corners upsample to the frame size, what the
        teacher itself calls its predictions).  The logits must be full (``logits_shape``): host logits are uploaded once at every class, the
        labels are derived from them, and only then are they reduced for a selected slot."""
        f = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
        assert f.dtype == torch.uint8, "the replay memory holds uint8 frames, got %s" % f.dtype
        assert tuple(f.shape) == (self.src_h, self.src_w, 3), "one source geometry per memory: [%d, %d, 3], got %s" % (self.src_h, self.src_w, tuple(f.shape))
        if label is None:
            full = self._full_logits_on_device(logits)
            views = self._slot_views(self.ring.push())
            views[0].copy_(f, non_blocking=f.is_cuda)
            self._derive_labels(full, views[1])
            if self.logits_select is not None:
                self._pack_logits(full, views[2])
            else:
                views[2].copy_(full, non_blocking=True)
            return
        l = labels_to_u8(label)
        assert tuple(l.shape) == (self.src_h, self.src_w), "labels must be [%d, %d], got %s" % (self.src_h, self.src_w, tuple(l.shape))
        assert (logits is not None) == (self._logits is not None), "teacher logits go with a memory constructed with logits_shape (and are required then)"
        t = None
        if logits is not None:
            t = self._logits_for_slot(logits)
        views = self._slot_views(self.ring.push())
        # device -> device copies are stream-ordered; a host array is copied before this returns (the caller may reuse it at once)
        views[0].copy_(f, non_blocking=f.is_cuda)
        views[1].copy_(l, non_blocking=l.is_cuda)
        if isinstance(t, tuple):          # full logits on the device for a selected slot
            self._pack_logits(t[0], views[2])
        elif t is not None:
            views[2].copy_(t.to(torch.float32), non_blocking=t.is_cuda)

    def _logits_for_slot(self, logits):
        """What ``append`` stores: a tensor of ``logits_cached_shape`` to copy, or ``(full device tensor,)`` for the pack kernel."""
        shape = tuple(logits.shape)
        if self.logits_select is None:
            assert shape == self.logits_shape, "teacher logits must be %s, got %s" % (self.logits_shape, shape)
        else:
            assert shape in (self.logits_shape, self.logits_cached_shape), \
                "teacher logits must be %s or, already reduced to the selected classes, %s, got %s" % (self.logits_shape, self.logits_cached_shape, shape)
        reduce = self.logits_select is not None and shape == self.logits_shape          # (K == classes: the two shapes coincide and mean full)
        if isinstance(logits, torch.Tensor):
            if reduce and logits.is_cuda:
                return (logits.to(torch.float32).contiguous(),)
            return logits[..., list(self.logits_select)] if reduce else logits
        a = np.asarray(logits, dtype=np.float32)
        if reduce:
            a = np.take(a, self.logits_select, axis=-1)          # only the K channels cross to the device
        return torch.from_numpy(np.ascontiguousarray(a))

    def _pack_logits(self, full: torch.Tensor, slot_view: torch.Tensor) -> None:
        th, tw, nc = self.logits_shape
        idx = (C.c_int32 * len(self.logits_select))(*self.logits_select)
        hip.check(hip.lib().ams_replay_pack_logits(C.c_void_p(full.data_ptr()), th, tw, nc, idx, len(self.logits_select), hip.TLOGITS_SELECTED,
                                                   C.c_void_p(slot_view.data_ptr()), self._stream()), "ams_replay_pack_logits")

    # ------------------------------------------------------------------ hard labels from the teacher logits
    def _full_logits_on_device(self, logits) -> torch.Tensor:
        """The full logits of one frame as a contiguous f32 device tensor: a device tensor in place, a host array uploaded once."""
        assert self._logits is not None and logits is not None, \
            "label=None derives the labels from the teacher logits: it needs a memory constructed with logits_shape, and the logits"
        shape = tuple(logits.shape)
        if shape != self.logits_shape and shape == self.logits_cached_shape:
            raise ValueError("label=None needs the full teacher logits %s: the argmax over all classes is not defined for logits already "
                             "reduced to the selected classes %s (a class outside the selection may hold the maximum)"
                             % (self.logits_shape, shape))
        assert shape == self.logits_shape, "teacher logits must be %s, got %s" % (self.logits_shape, shape)
        assert self.logits_shape[2] <= 255, "labels are derived for at most 255 classes (id 255 stays \"unlabelled\")"
        assert self.logits_shape[0] <= self.src_h and self.logits_shape[1] <= self.src_w, LARGE_LOGITS.replace("logits_upsample=True", "label=None") \
            % (self.logits_shape[:2] + (self.src_h, self.src_w))
        if isinstance(logits, torch.Tensor):
            return logits.to(device=self.device, dtype=torch.float32).contiguous()
        return torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(self.device)

    def _derive_labels(self, full: torch.Tensor, out: torch.Tensor) -> None:
        lh, lw, nc = self.logits_shape
        hip.check(hip.lib().ams_teacher_labels_from_logits(C.c_void_p(full.data_ptr()), lh * lw * nc, 1, lh, lw, nc, self.src_h, self.src_w,
                                                           C.c_void_p(out.data_ptr()), self.src_h * self.src_w, self._stream()),
                  "ams_teacher_labels_from_logits")

    def labels_from_logits(self, logits) -> torch.Tensor:
        """The label map ``append(frame, None, logits)`` would store, as a fresh uint8 [src_h, src_w] device tensor; nothing is stored."""
        out = torch.empty((self.src_h, self.src_w), dtype=torch.uint8, device=self.device)
        self._derive_labels(self._full_logits_on_device(logits), out)
        return out

    # ------------------------------------------------------------------ sampling
    def plan(self, samples: np.ndarray, H: int, W: int) -> ReplayPlan:
        """``samples``: ``draw_samples``' descriptors (logical slots) for a whole phase -> the phase's table on the device (physical slots)."""
        table = np.ascontiguousarray(samples, dtype=np.int32).copy()
        assert table.ndim == 3 and table.shape[2] == SAMPLE_FIELDS
        table[..., 0] = self.ring.physical(table[..., 0].astype(np.int64))
        return ReplayPlan(self, table, int(H), int(W))

    def _batch_buffers(self, batch: int, H: int, W: int, whole_frames: bool = True):
        """The resident mini-batch buffer: allocated once per batch geometry.  The logits of whole frames keep their cached grid; resampled
        with the frames they have the label size."""
        logits_shape = None
        if self.logits_shape:
            logits_shape = (batch,) + (self.logits_cached_shape if whole_frames else (H, W, self.logits_cached_shape[2]))
        key = (batch, H, W, logits_shape)
        if self._buffers is None or self._buffers[0] != key:
            logits = torch.empty(logits_shape, dtype=torch.float32, device=self.device) if logits_shape else None
            self._buffers = (key, torch.empty((batch, H, W, 3), dtype=torch.uint8, device=self.device),
                             torch.empty((batch, H, W), dtype=torch.uint8, device=self.device), logits)
        return self._buffers[1:]

    # the device touch points (tests/test_replay_cpu.py replaces them with stand-ins)
    def _upload(self, table: np.ndarray) -> torch.Tensor:
        return torch.from_numpy(table).to(self.device)

    def _stream(self) -> C.c_void_p:
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _gather(self, samples_host: np.ndarray, samples_dev: torch.Tensor, H: int, W: int, frames_out: torch.Tensor, labels_out: torch.Tensor) -> None:
        batch = int(samples_host.shape[0])
        assert samples_host.dtype == np.int32 and samples_host.flags.c_contiguous and samples_dev.is_contiguous()
        assert frames_out.numel() == batch * H * W * 3 and labels_out.numel() == batch * H * W
        hip.check(hip.lib().ams_replay_gather(C.c_void_p(self._frames.data_ptr()), self.frame_stride, C.c_void_p(self._labels.data_ptr()), self.label_stride,
                                              self.capacity, self.src_h, self.src_w, C.c_void_p(samples_dev.data_ptr()),
                                              samples_host.ctypes.data_as(C.c_void_p), batch, H, W, C.c_void_p(frames_out.data_ptr()),
                                              C.c_void_p(labels_out.data_ptr()), self._stream()), "ams_replay_gather")

    def _gather_logits(self, samples_host: np.ndarray, samples_dev: torch.Tensor, out: torch.Tensor, crop=None) -> None:
        """``crop`` None: whole slots on their cached grid.  ``crop`` = (H, W): source-size logits rescaled, cropped and mirrored with the frame;
        on a ``logits_upsample`` memory with a smaller grid, the grid's align-corners upsample to the source size takes their place."""
        th, tw, ch = self.logits_cached_shape
        batch = int(samples_host.shape[0])
        assert samples_host.dtype == np.int32 and samples_host.flags.c_contiguous and samples_dev.is_contiguous()
        oh, ow = (th, tw) if crop is None else crop
        assert out.numel() == batch * oh * ow * ch
        slots = (C.c_void_p(self._logits.data_ptr()), self.logits_stride, self.capacity)
        samples = (C.c_void_p(samples_dev.data_ptr()), samples_host.ctypes.data_as(C.c_void_p), batch)
        tail = (C.c_void_p(out.data_ptr()), self._stream())
        if crop is None:
            name, args = "ams_replay_gather_f32", slots + (th, tw, ch) + samples + tail
        elif self.logits_at_source:
            name, args = "ams_replay_gather_logits", slots + (self.src_h, self.src_w, ch) + samples + (oh, ow) + tail
        else:
            assert self.logits_upsample
            name, args = "ams_replay_gather_logits_lowres", slots + (th, tw, ch, self.src_h, self.src_w) + samples + (oh, ow) + tail
        hip.check(getattr(hip.lib(), name)(*args), name)

    def gather(self, samples: np.ndarray, H: int, W: int):
        """One mini-batch for ``[batch, 6]`` descriptors with logical slots: fresh device tensors (frames uint8 [batch,H,W,3], labels uint8
        [batch,H,W]).  ``train_with_deque`` uses ``plan`` instead (one upload per phase, one resident buffer)."""
        p = self.plan(np.asarray(samples)[None], H, W)
        frames, labels, _ = p.batch(0)
        return frames.clone(), labels.clone()

    def gather_logits(self, samples: np.ndarray, H: int, W: int) -> torch.Tensor:
        """The teacher logits of that mini-batch: a fresh f32 device tensor, [batch, H, W, channels] for logits cached at the frame size or,
        with ``logits_upsample``, on a smaller grid (rescaled, cropped and mirrored with the frames), the cached grid for whole frames;
        channels = ``logits_cached_shape[2]``."""
        assert self.logits_shape is not None, "the memory was constructed without logits_shape"
        return self.plan(np.asarray(samples)[None], H, W).batch(0)[2].clone()

    # ------------------------------------------------------------------ ASR's phi-score
    def cross_miou_pairs(self, network, first: int = 0):
        """``network.calc_cross_miou(np.array([memory[k], memory[k + 1]]))`` for k = first .. len - 2 (the loop of reference run.py:287-291), as
        one launch and one device -> host copy: a list of (conf_mat float64 [K, K], iou list, miou), one entry per pair, equal to the per-pair
        results.  The memory's labels must have the network's size."""
        assert not network.frozen or network.cross_miou_compat
        eng = network.engine
        assert (self.src_h, self.src_w) == (network.height, 2 * network.height), "labels must be [%d, %d]" % (network.height, 2 * network.height)
        first = max(0, int(first))
        n = len(self) - 1 - first
        if n <= 0:
            return []
        logical = np.arange(first, first + n, dtype=np.int64)
        pairs = np.ascontiguousarray(np.stack([self.ring.physical(logical), self.ring.physical(logical + 1)], axis=1), dtype=np.int32)
        with network.process_lock:
            conf = self._cross_confusion_pairs(eng, pairs)
        out = []
        for k in range(n):
            conf_mat_ = conf[k].astype(np.float64)
            iou_ = calculate_miou(conf_mat_, nan=True)
            out.append((conf_mat_, iou_, np.nanmean(iou_)))
        return out

    def class_counts(self, network) -> np.ndarray:
        """Pixels per class of the network's subset over every label map in the memory, int64 [K]: the label-confusion kernel on each slot
        against itself has the slot's histogram on its diagonal (one launch, one copy; no kernel of its own)."""
        n = len(self)
        if n == 0:
            return np.zeros(network.engine.K, dtype=np.int64)
        phys = self.ring.physical(np.arange(n, dtype=np.int64))
        pairs = np.ascontiguousarray(np.stack([phys, phys], axis=1), dtype=np.int32)
        with network.process_lock:
            conf = self._cross_confusion_pairs(network.engine, pairs)
        return np.einsum("nkk->k", conf).astype(np.int64)

    def _cross_confusion_pairs(self, eng, pairs: np.ndarray) -> np.ndarray:
        n = int(pairs.shape[0])
        pairs_dev = self._upload(pairs)
        conf = torch.empty((n, eng.K, eng.K), dtype=torch.int64, device=self.device)
        hip.check(eng.lib.ams_cross_confusion_pairs(eng._h, C.c_void_p(self._labels.data_ptr()), self.label_stride, self.capacity, self.src_h * self.src_w,
                                                    C.c_void_p(pairs_dev.data_ptr()), pairs.ctypes.data_as(C.c_void_p), n,
                                                    C.c_void_p(conf.data_ptr()), self._stream()), "ams_cross_confusion_pairs")
        return conf.cpu().numpy()
