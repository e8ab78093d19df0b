"""The edge's pictures on the device (k_render.hip, ``ams_render_views``): the six RGB views that ``SemanticNetwork.colorize``,
``colorize_teacher`` and ``cross_ignore`` paint with NumPy on host arrays, for callers whose frame and labels are device tensors.

  colour_student / overlay_student     ``colorize(frame, label)``            -> (colour, overlay)
  colour_teacher / overlay_teacher     ``colorize_teacher(label, frame)``    -> (colour, overlay)
  cross_mask / ignore_mask             ``cross_ignore(teacher, student)``    -> (cross_mask, ignore_mask)

The host helpers are the yardstick: every view equals them bit for bit (tests/test_gpu_render.py).  One difference is deliberate and is the
kernel's, not the helpers': labels out of range give defined output instead of an ``IndexError``.  A student label outside ``[0, K)`` paints
black; a teacher id from ``TOTAL_CLASSES`` on counts as ignored (white in ``ignore_mask``, black in ``cross_mask`` and ``colour_teacher``),
which is also what the metric of ``predict_with_metric`` does with such an id (its class table maps every id outside the subset to ignored).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence

import numpy as np

from . import hip

VIEWS = hip.RENDER_VIEWS                      # the order of ams_render_out
TABLE_BYTES = hip.RENDER_TABLE_BYTES
_PALETTE, _REDUCED, _TAKE = 0, 768, 864      # byte offsets of the three tables inside the block (k_render.hip)
MAX_K = 32

# which inputs a view reads
_READS = {"colour_student": "s", "overlay_student": "fs", "colour_teacher": "t", "overlay_teacher": "ft", "ignore_mask": "t", "cross_mask": "st"}


def build_tables(color_map_reduced, palette, take_array, total_classes: Optional[int] = None) -> np.ndarray:
    """The table block of ``ams_render_views`` as uint8 [TABLE_BYTES] (pure host arithmetic): the full palette [256, 3], the reduced
    palette [32, 3] with the rows from K on zero, and the take table [256] (teacher id -> subset index) with zeros from
    ``total_classes`` (default ``len(take_array)``) on."""
    reduced = np.asarray(color_map_reduced, dtype=np.uint8).reshape(-1, 3)
    palette = np.asarray(palette, dtype=np.uint8).reshape(-1, 3)
    take = np.asarray(take_array).reshape(-1)
    total = len(take) if total_classes is None else int(total_classes)
    assert 1 <= len(reduced) <= MAX_K, "the reduced palette holds 1 .. %d colours, got %d" % (MAX_K, len(reduced))
    assert len(palette) == 256, "the full palette has 256 rows"
    assert 0 < total <= 256 and len(take) >= total
    assert take[:total].min() >= 0 and take[:total].max() < len(reduced), "take_array points outside the reduced palette"
    block = np.zeros(TABLE_BYTES, dtype=np.uint8)
    block[_PALETTE:_PALETTE + 768] = palette.reshape(-1)
    block[_REDUCED:_REDUCED + 3 * len(reduced)] = reduced.reshape(-1)
    block[_TAKE:_TAKE + total] = take[:total].astype(np.uint8)
    return block


class RenderedViews(dict):
    """view name -> uint8 device tensor [B, H, W, 3].  The views of one launch are slices of one device block: ``host()`` brings them all
    to the host in ONE copy and returns name -> ndarray."""
    block = None

    def host(self) -> Dict[str, np.ndarray]:
        flat = self.block.cpu().numpy()
        return {name: flat[j] for j, name in enumerate(self)}


class DeviceRenderer:
    """The uploaded table block of one network and the launch.  Built once per network (``SemanticNetwork`` makes it on first use)."""

    def __init__(self, color_map_reduced, palette, take_array, total_classes, device):
        import torch
        self.lib = hip.lib()
        assert int(self.lib.ams_render_table_bytes()) == TABLE_BYTES, "libams_hip.so lays the render tables out differently"
        self.device = torch.device(device)
        self.K = int(np.asarray(color_map_reduced).reshape(-1, 3).shape[0])
        self.tables_host = build_tables(color_map_reduced, palette, take_array, total_classes)
        self.tables = torch.from_numpy(self.tables_host).to(self.device)

    def _u8(self, x):
        import torch
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if t.dtype != torch.uint8:                       # the engine's rule for teacher ids: outside 0..254 can never be selected -> 255
            ti = t.to(torch.int64)
            t = torch.where((ti >= 0) & (ti < 255), ti, torch.full_like(ti, 255)).to(torch.uint8)
        return t.to(self.device, non_blocking=True).contiguous()

    def render(self, frames=None, student=None, teacher=None, views: Sequence[str] = VIEWS) -> RenderedViews:
        """One launch on the current stream.  ``frames`` uint8 [B,H,W,3], ``student`` uint8 or int32 [B,H,W] (indices into the subset),
        ``teacher`` uint8 [B,H,W] (dataset ids): device tensors, or host arrays that are uploaded first.  Nothing is synchronised."""
        import torch
        views = tuple(views)
        assert views and all(v in VIEWS for v in views) and len(set(views)) == len(views), "views: a non-empty choice of %s" % (VIEWS,)
        reads = set("".join(_READS[v] for v in views))
        assert "f" not in reads or frames is not None, "an overlay needs the frames"
        assert "s" not in reads or student is not None, "%s need the student labels" % (views,)
        assert "t" not in reads or teacher is not None, "%s need the teacher labels" % (views,)
        dtype = hip.DT_U8
        if student is not None:
            if not isinstance(student, torch.Tensor):
                student = torch.from_numpy(np.ascontiguousarray(student))
            if student.dtype != torch.uint8:
                student, dtype = student.to(torch.int32), hip.DT_I32
            student = student.to(self.device, non_blocking=True).contiguous()
        if teacher is not None:
            teacher = self._u8(teacher)
        if frames is not None:
            frames = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
            assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3, "frames must be uint8 [B,H,W,3]"
            frames = frames.to(self.device, non_blocking=True).contiguous()
        shape = tuple((student if student is not None else teacher).shape)
        assert len(shape) == 3, "labels must be [B,H,W]"
        for other in (student, teacher):
            assert other is None or tuple(other.shape) == shape, "student and teacher labels differ in shape"
        assert frames is None or tuple(frames.shape[:3]) == shape, "frames and labels differ in shape"
        b, h, w = shape
        block = torch.empty((len(views), b, h, w, 3), dtype=torch.uint8, device=self.device)
        out = hip.RenderOut()
        result = RenderedViews()
        for j, name in enumerate(views):
            setattr(out, name, block[j].data_ptr())
            result[name] = block[j]
        result.block = block
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None     # noqa: E731
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        hip.check(self.lib.ams_render_views(ptr(frames), ptr(student), dtype, ptr(teacher), b, h, w, self.K, C.c_void_p(self.tables.data_ptr()),
                                            C.byref(out), stream), "ams_render_views")
        return result
