"""The edge's asynchronous per-frame call, ``depth`` frames at a time (an addition: the reference's call is synchronous)."""
# A one-frame forward is ~45 dependent launches that leave most of the chip idle (0.49 ms); two frames in one pass take 0.59 ms, three 0.68 ms.
# Submitted frames wait until ``depth`` of them are there (or until one of them is collected), then run as ONE pass with per-frame metrics
# (ams_student_predict_frames).  Each frame's result is what ``SemanticNetwork.predict_with_metric`` returns for it, bit for bit.  Views and
# confidence asked for with a frame are launched right behind its pass on the same stream and handed over by ``take_rendered`` /
# ``take_confidence``; ``collect`` keeps its 5-tuple.
#
# The engine has ONE output block, one label view and one set of low-resolution logits.  So the previous pass is fetched before the next one
# is launched, and everything that reads a pass on the device is enqueued behind it and before the next one.  The caller serialises the calls
# (``SemanticNetwork.process_lock``).
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from .confidence import Confidence, ConfidenceStats


class Submitted(NamedTuple):                # a frame that waits for its pass
    ticket: int
    frames: object
    labels: object
    views: Optional[tuple]
    wants_confidence: bool


class PassRows:
    """The confidence statistics rows of one pass: on the device until the first of its tickets asks, then on the host for all of them."""

    def __init__(self, dev):
        self.dev, self._host = dev, None

    def host(self) -> np.ndarray:
        if self._host is None:
            self._host = self.dev.cpu().numpy()
        return self._host


class EdgePipeline:
    def __init__(self, engine, mode: int, depth: int, renderer, metrics, class_count: int):
        # renderer: () -> the network's DeviceRenderer (built on first use); metrics: (confusion matrix int64, loss [sum, count]) -> what
        # follows the labels in a result
        self.engine, self.mode, self.depth = engine, mode, depth
        self._renderer, self._metrics, self._class_count = renderer, metrics, class_count
        self._queued = []              # Submitted, not yet launched
        self._pending = []             # tickets of the pass that is running on the GPU (its results are still on the device)
        self._ready = {}               # ticket -> result, after its pass was fetched
        self._rendered = {}            # ticket -> views painted behind its pass
        self._confident = {}           # ticket -> (confidence map of its frame, its pass's PassRows, frame index)
        self._tickets = 0

    def submit(self, frames, labels_teacher, render=None, confidence=False) -> int:
        self._tickets += 1
        self._queued.append(Submitted(self._tickets, frames, labels_teacher, tuple(render) if render else None, bool(confidence)))
        if len(self._queued) >= self.depth:
            self._launch()
        return self._tickets

    def drain(self) -> None:
        """Fetch the pass that is on the GPU, if any: one device -> host copy, one synchronisation for the whole pass.  Anything else that is
        about to write the engine's output block calls this first, so that ``collect`` later returns the pass's own metrics."""
        if self._pending:
            labs, confs, losses = self.engine.fetch_frames()
            for k, t in enumerate(self._pending):
                self._ready[t] = (labs[k:k + 1],) + self._metrics(confs[k], losses[k])
            self._pending = []

    def _launch(self) -> None:
        self.drain()
        queued, self._queued = self._queued, []
        cat = (lambda xs: torch.cat(list(xs))) if hasattr(queued[0].frames, "unsqueeze") else \
            (lambda xs: np.concatenate([np.asarray(x) for x in xs]))
        self._pending = [q.ticket for q in queued]
        # returns at once: the pass runs while the caller goes on (labels leave as uint8)
        labels_dev, _conf, _loss = self.engine.predict_frames(cat(q.frames for q in queued), cat(q.labels for q in queued), self.mode, u8=True)
        frames_dev, teacher_dev = self.engine.last_inputs()
        for k, q in enumerate(queued):
            if q.views:                           # behind the pass and before the next one, which overwrites the label view
                self._rendered[q.ticket] = self._renderer().render(frames_dev[k:k + 1], labels_dev[k:k + 1], teacher_dev[k:k + 1], q.views)
        if any(q.wants_confidence for q in queued):       # one launch over the whole pass, before the next one overwrites the logits
            conf_map, _f32, stats_dev = self.engine.confidence(teacher_dev)
            rows = PassRows(stats_dev)
            for k, q in enumerate(queued):
                if q.wants_confidence:
                    self._confident[q.ticket] = (conf_map[k:k + 1], rows, k)

    def _launch_if_queued(self, ticket, wanted) -> None:
        if any(q.ticket == ticket and wanted(q) for q in self._queued):
            self._launch()

    def collect(self, ticket):
        if ticket not in self._ready:
            if ticket not in self._pending:
                assert any(q.ticket == ticket for q in self._queued), "unknown ticket"
                self._launch()
            self.drain()
        return self._ready.pop(ticket)

    def take_rendered(self, ticket):
        if ticket not in self._rendered:
            self._launch_if_queued(ticket, lambda q: q.views)
        assert ticket in self._rendered, "no views were requested for this ticket (or they were taken already)"
        return self._rendered.pop(ticket)

    def take_confidence(self, ticket) -> Confidence:
        if ticket not in self._confident:
            self._launch_if_queued(ticket, lambda q: q.wants_confidence)
        assert ticket in self._confident, "no confidence was requested for this ticket (or it was taken already)"
        conf_map, rows, k = self._confident.pop(ticket)
        return Confidence(conf_map, [ConfidenceStats(rows.host()[k], self._class_count)])

    def flush(self) -> None:
        """Launch what is queued and fetch it: afterwards nothing of the current model's is outstanding (``collect`` still hands it over)."""
        if self._queued:
            self._launch()
        self.drain()

    def clear(self) -> None:
        """Views and confidence maps nobody took: their device memory goes with the engine."""
        self._rendered.clear()
        self._confident.clear()
