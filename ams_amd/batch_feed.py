"""Mini-batches from host deques to the device for ``SemanticNetwork.train_with_deque``: the reference's two helper threads
(SemanticNetwork.py:222-231, :679-704) behind one object."""
#   sampler thread   draws mini-batches from the replay memory (utils.mini_batch contract) into a ring of pinned host buffers
#   stager thread    copies them to the device on a side stream (the FIFO queue of the reference graph), a bounded number ahead
#   training loop    ``next_staged`` / ``consume``: makes the compute stream wait for a batch's copy and takes its device tensors
#
# The reference's helpers have no failure path: if one dies — a frame of the wrong shape trips the assert in the sampler — the training loop
# polls its deque forever with the process lock held.  Here every helper hands its exception over (``error``: the first one), every wait loop
# watches the abort flag, ``next_staged`` answers None, and ``stop`` joins both threads whatever happened.
from __future__ import annotations

import random
import threading
import time
from collections import deque

import numpy as np
import torch

from .utils import mini_batch


class HostBatchFeed:
    SLEEP_INTERVAL = 1 / 1000.

    def __init__(self, height, mini_batch_size, scale, device):
        self.height, self.mini_batch_size, self.scale, self.device = height, mini_batch_size, scale, device
        self.error = None                 # the first helper's exception of the last phase
        self._abort, self._threads = threading.Event(), []
        self._ring = None                 # pinned staging slots, created on first use

    # ------------------------------------------------------------------ the training loop's side
    def start(self, iterations, frame_deque, label_deque, teacher_logits_deque=None):
        self.error, self._abort = None, threading.Event()
        self._batches, self._staged = deque(), deque()        # sampler -> stager -> training loop
        self._threads = [threading.Thread(target=self._guarded, args=(self._fill_batch, frame_deque, label_deque, iterations, teacher_logits_deque)),
                         threading.Thread(target=self._guarded, args=(self._fill_queue, iterations))]
        for t in self._threads:
            t.start()

    def next_staged(self):
        """The next staged batch (for ``consume``), or None: a helper died, ``error`` holds its exception."""
        while True:
            try:
                return self._staged.popleft()
            except IndexError:
                if self._abort.is_set():
                    return None
                time.sleep(self.SLEEP_INTERVAL)

    def consume(self, staged):
        """Make the compute stream wait for a staged batch's copy; returns its device tensors (frames, labels, teacher logits or None)."""
        frames_dev, labels_dev, ready = staged[:3]
        logits_dev = staged[3] if len(staged) > 3 else None
        compute = torch.cuda.current_stream(self.device)
        compute.wait_event(ready)
        # the buffers were allocated on the stager's copy stream: tell the caching allocator that the compute stream uses
        # them too, or dropping the references one iteration later hands the block back to the copy stream's pool while
        # this step's kernels (the stem weight gradient re-reads the frames in backward) are still queued
        frames_dev.record_stream(compute)
        labels_dev.record_stream(compute)
        if logits_dev is not None:
            logits_dev.record_stream(compute)
        return frames_dev, labels_dev, logits_dev

    def stop(self):
        """After a clean phase the helpers have returned already; after an error this stops them.  No slot is owed to a stager afterwards."""
        self._abort.set()
        for t in self._threads:
            t.join()
        self._threads = []
        if self._ring is not None:
            for slot in self._ring["slots"]:
                if slot[2] is not None:
                    slot[2].synchronize()
                slot[2], slot[3] = None, False

    def _guarded(self, fn, *args):
        """Body of a helper thread: the first exception of any helper is kept for the caller and stops the others."""
        try:
            fn(*args)
        except BaseException as e:  # noqa: BLE001  (handed to the calling thread, which re-raises it)
            if self.error is None:
                self.error = e
            self._abort.set()

    # ------------------------------------------------------------------ sampler thread
    def _fill_batch(self, frame_deque, label_deque, number_of_batches, teacher_logits_deque=None):
        """Sample mini-batches from the replay memory (utils.mini_batch contract).

        Fast path (the only one run.py exercises: scale == [1], frames already at network size): draws the same
        random numbers in the same order as ``mini_batch`` but gathers the uint8 frames directly instead of
        materialising float64 copies (B x 12.6 MB per batch at 512x1024)."""
        frames = list(frame_deque) if isinstance(frame_deque, deque) else frame_deque
        labels = list(label_deque) if isinstance(label_deque, deque) else label_deque
        crop = [self.height, self.height * 2]
        fast = (list(self.scale) == [1] and all(f.shape[:2] == tuple(crop) for f in frames))
        fast = fast and all(f.dtype == np.uint8 for f in frames) and all(l.dtype == np.uint8 and l.shape == tuple(crop) for l in labels)
        soft = list(teacher_logits_deque) if teacher_logits_deque is not None else None
        # soft targets follow the frames a batch drew: on this path only where frames are taken as they are.  Rescaled, cropped and flipped
        # soft batches are a capability of the device memory (replay.DeviceReplayMemory with logits cached at the frame size)
        assert soft is None or fast, ("teacher_logits_deque needs uint8 frames and labels at the network size and scale == [1]; a "
                                      "DeviceReplayMemory with logits_shape at the frame size trains on rescaled, cropped and flipped soft batches")
        for _ in range(number_of_batches):
            if self._abort.is_set():
                return
            slot = None
            if fast:
                picks = []
                for _j in range(self.mini_batch_size):
                    picks.append(np.random.choice(len(frames)))
                    random.randint(0, 0)      # scale choice
                    random.randint(0, 0)      # row offset  (slack is 0 when the frame already has the crop size)
                    random.randint(0, 0)      # column offset
                # gathered straight into a pinned staging slot: one host copy per frame, none per batch (a fresh pin_memory() per batch
                # costs a page-lock of 12-16 MB each time)
                slot = self._staging_slot()
                if slot is None:              # the stager has died
                    return
                image_batch, label_batch = slot[0].numpy(), slot[1].numpy()
                for j, p in enumerate(picks):
                    image_batch[j] = frames[p]
                    label_batch[j] = labels[p]
            else:
                ib, lb = mini_batch(frames, labels, crop, self.scale, self.mini_batch_size, 1, flip=False)
                image_batch, label_batch = ib[0], lb[0]
            assert np.shape(label_batch) == (self.mini_batch_size, self.height, self.height * 2)
            assert np.shape(image_batch) == (self.mini_batch_size, self.height, self.height * 2, 3)
            batch = {'frames': image_batch, 'labels': label_batch, 'slot': slot}
            if soft is not None:
                # [th, tw, classes] arrays, or [th, tw, K] ones (the network's classes alone): stacked and uploaded as they are, the engine
                # tells the layout by the last dimension
                batch['teacher_logits'] = np.stack([np.asarray(soft[p], dtype=np.float32) for p in picks])
            self._batches.append(batch)

    def _staging_slot(self):
        """Next slot [frames, labels, event of the copy that reads it, handed out] of a ring of four pairs of pinned host buffers
        [mini_batch, H, 2H, 3] / [mini_batch, H, 2H] uint8.  A slot is handed out again only after the stager has issued the H2D copy that
        reads it AND that copy has finished (its event): the sampler runs at most four batches ahead of the copies.  None: aborted."""
        if self._ring is None:
            shape = (self.mini_batch_size, self.height, 2 * self.height)
            self._ring = {"next": 0, "slots": [[self._pinned(shape + (3,)), self._pinned(shape), None, False] for _ in range(4)]}
        ring = self._ring
        slot = ring["slots"][ring["next"] % len(ring["slots"])]
        ring["next"] += 1
        while slot[3] and slot[2] is None:        # handed out earlier and still waiting in the batch deque for the stager
            if self._abort.is_set():              # ... which has died: do not wait for it
                return None
            time.sleep(self.SLEEP_INTERVAL)
        if slot[2] is not None:
            slot[2].synchronize()
            slot[2] = None
        slot[3] = True
        return slot

    @staticmethod
    def _pinned(shape):
        t = torch.empty(shape, dtype=torch.uint8)
        return t.pin_memory() if torch.cuda.is_available() else t

    # ------------------------------------------------------------------ stager thread
    def _fill_queue(self, number_of_batches):
        """The FIFO queue of the reference graph (capacity 200): H2D on a side stream."""
        copy_stream = self._make_copy_stream()
        max_staged = None
        for _ in range(number_of_batches):
            batch = None
            while batch is None:
                try:
                    batch = self._batches.popleft()
                except IndexError:
                    if self._abort.is_set():
                        return
                    time.sleep(self.SLEEP_INTERVAL)
            staged = self._stage_batch(batch, copy_stream)
            if max_staged is None:
                # the reference's FIFO queue holds 200 batches whatever their size (3 GB of device memory at batch 10 of 512x1024): here the
                # staged-ahead set is bounded by BYTES — 1 GiB, at least two batches, at most the reference's 200 entries
                nbytes = sum(int(t.numel()) * t.element_size() for t in staged[:2])
                max_staged = max(2, min(200, (1 << 30) // max(nbytes, 1)))
            while len(self._staged) >= max_staged:
                if self._abort.is_set():
                    return
                time.sleep(self.SLEEP_INTERVAL)
            self._staged.append(staged)

    def _make_copy_stream(self):
        return torch.cuda.Stream(device=self.device)

    def _stage_batch(self, batch, copy_stream):
        """Host batch -> (frames on the device, labels on the device, event of the copies[, teacher logits]) on the copy stream."""
        dev = self.device
        slot = batch.get('slot')
        if slot is not None:              # already in pinned memory (the sampler's fast path)
            with torch.cuda.stream(copy_stream):
                f_dev = slot[0].to(dev, non_blocking=True)
                l_dev = slot[1].to(dev, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(copy_stream)
            slot[2] = ready
        else:
            fr = batch['frames']
            fr = fr if fr.dtype == np.uint8 else fr.astype(np.float32)
            lb = batch['labels']
            if lb.dtype != np.uint8:
                li = lb.astype(np.float32).astype(np.int64)
                lb = np.where((li >= 0) & (li < 255), li, 255).astype(np.uint8)
            with torch.cuda.stream(copy_stream):
                f_dev = torch.from_numpy(np.ascontiguousarray(fr)).pin_memory().to(dev, non_blocking=True)
                l_dev = torch.from_numpy(np.ascontiguousarray(lb)).pin_memory().to(dev, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(copy_stream)
        if batch.get('teacher_logits') is not None:       # soft_teacher: the batch's cached teacher logits travel with it
            with torch.cuda.stream(copy_stream):
                t_dev = torch.from_numpy(batch['teacher_logits']).pin_memory().to(dev, non_blocking=True)
                ready = torch.cuda.Event()
                ready.record(copy_stream)
            if slot is not None:
                slot[2] = ready
            return f_dev, l_dev, ready, t_dev
        return f_dev, l_dev, ready
