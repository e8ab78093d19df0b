"""The uplink frame codec on the device (k_uplink.hip; format AUC1, stated in include/ams_hip.h): what ``run.py --compress_uplink`` sends.

    codec = UplinkCodec(device)
    payload, quality, fits = codec.encode_to_budget(frame_u8, budget_bytes)      # torch.uint8 [n] on the device
    frame = codec.decode(payload)                                                # torch.uint8 [H, W, 3] on the device

With a reference frame (``reference=``: what the decoder gave for the previous frame) a frame may travel predicted, format AUP1
(k_uplink_inter.hip): one motion vector per macroblock and the residual, chosen per frame against AUC1 from the exact sizes of both.

An intra-frame transform codec of the project's own (colour to 4:2:0 YCbCr, 8 x 8 integer DCT, JPEG quantisation tables with libjpeg's quality
scale, Exp-Golomb run/level codes in independent slices of 32 blocks).  It stands where the reference pushes sampled frames through
ffmpeg/libx264 at a bitrate: lossy frames at a byte budget, counted in real bytes.  Its byte counts are not H.264's.  The rate rule is exact:
the quality used is the largest of 1 .. 100 whose payload fits, taken from the sizes of all 100 (one transform, one table, one
synchronisation).  Frames may be host arrays or device tensors.  No CPU fallback: without the HIP library or a GPU this raises.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import hip

ArrayLike = Union[np.ndarray, torch.Tensor]
STATUS_WORDS = {hip.UPLINK_BAD_HEADER: "header", hip.UPLINK_BAD_TABLE: "slice table", hip.UPLINK_BAD_SLICE_END: "end of a slice",
                hip.UPLINK_BAD_POSITION: "coefficient position past 63", hip.UPLINK_BAD_ZERO_LEVEL: "AC level of 0",
                hip.UPLINK_BAD_LEVEL: "level beyond +-2047", hip.UPLINK_BAD_OVERRUN: "code running past its slice",
                hip.UPLINK_NO_ROOM: "no room for the payload", hip.UPLINK_BAD_VECTOR: "motion vector beyond +-15 or leaving the frame",
                hip.UPLINK_BAD_ZERO_SLICE: "all-zero slice sent with bytes"}
INTRA, INTER = "AUC1", "AUP1"


def kind_of(payload) -> Optional[str]:
    """"AUC1" (intra), "AUP1" (predicted: decode needs the reference) or None, from the payload's first four bytes."""
    head = payload[:4]
    head = bytes(head.cpu().numpy()) if isinstance(head, torch.Tensor) else bytes(np.asarray(head, np.uint8)) if not isinstance(
        head, (bytes, bytearray, memoryview)) else bytes(head)
    return {b"AUC1": INTRA, b"AUP1": INTER}.get(head)


def table_lengths(payload, H: int, W: int) -> np.ndarray:
    """The slice table of a well-formed payload of either kind for an H x W frame: int64 [slices] byte lengths (one copy to the host)."""
    blocks = [(H // 8) * (W // 8), (H // 16) * (W // 16), (H // 16) * (W // 16)]
    n = sum((b + 31) // 32 for b in blocks) + ((blocks[1] + 31) // 32 if kind_of(payload) == INTER else 0)
    table = payload[16:16 + 2 * n]
    table = table.cpu().numpy() if isinstance(table, torch.Tensor) else np.frombuffer(bytes(table), np.uint8)
    return table.view("<u2").astype(np.int64)


def choose_kind(sizes_intra, sizes_inter, budget: int) -> Tuple[str, int, bool]:
    """The per-frame rate rule over the 100 sizes of both kinds -> (kind, quality, fits)."""
    fit_i, fit_p = np.nonzero(np.asarray(sizes_intra) <= budget)[0], np.nonzero(np.asarray(sizes_inter) <= budget)[0]
    qi, qp = (int(fit_i[-1]) + 1 if len(fit_i) else 0), (int(fit_p[-1]) + 1 if len(fit_p) else 0)
    if not qi and not qp:
        return INTRA, 1, False
    if qp > qi or (qp == qi and sizes_inter[qp - 1] < sizes_intra[qi - 1]):
        return INTER, qp, True
    return INTRA, qi, True


class UplinkRefused(ValueError):
    """A payload the decoder refused (``status`` = AMS_UPLINK_*); nothing was decoded."""

    def __init__(self, status: int):
        ValueError.__init__(self, "uplink payload refused: %s (status %d)" % (STATUS_WORDS.get(status, "?"), status))
        self.status = status


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


class UplinkCodec:
    def __init__(self, device: Union[str, torch.device, None] = None):
        if not torch.cuda.is_available():
            raise RuntimeError("UplinkCodec needs an MI355X (there is no CPU fallback)")
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.lib = hip.lib()
        self._enc = {}              # (H, W) -> (scratch, sizes, bytes, status)
        self._dec = {}              # (H, W) -> (scratch, status)
        self._enc_p = {}            # the same for AUP1
        self._dec_p = {}

    def max_payload_bytes(self, H: int, W: int) -> int:
        n = int(self.lib.ams_uplink_max_bytes(H, W))
        if n == 0:
            raise ValueError("uplink codec: a frame is H x W x 3 with H and W multiples of 16 in 16 .. 4096, got %d x %d" % (H, W))
        return n

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _frame(self, frame: ArrayLike) -> torch.Tensor:
        t = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
        assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[2] == 3, "the codec takes uint8 [H, W, 3] frames, got %s %s" % (t.dtype, tuple(t.shape))
        self.max_payload_bytes(int(t.shape[0]), int(t.shape[1]))
        return t.to(self.device, non_blocking=True).contiguous()

    def _encoder(self, H: int, W: int):
        if (H, W) not in self._enc:
            self._enc[(H, W)] = (torch.empty(int(self.lib.ams_uplink_encode_scratch(H, W)), dtype=torch.uint8, device=self.device),
                                 torch.empty(100, dtype=torch.int64, device=self.device), torch.empty(1, dtype=torch.int64, device=self.device),
                                 torch.empty(1, dtype=torch.int32, device=self.device))
        return self._enc[(H, W)]

    def _transform(self, frame: ArrayLike):
        src = self._frame(frame)
        H, W = int(src.shape[0]), int(src.shape[1])
        scratch = self._encoder(H, W)[0]
        hip.check(self.lib.ams_uplink_transform(_ptr(src), H, W, _ptr(scratch), scratch.numel(), self._stream()), "ams_uplink_transform")
        return H, W

    def _write(self, H: int, W: int, quality: int, cap: int) -> torch.Tensor:
        scratch, _sizes, nbytes, status = self._encoder(H, W)
        payload = torch.empty(cap, dtype=torch.uint8, device=self.device)
        hip.check(self.lib.ams_uplink_encode(_ptr(scratch), scratch.numel(), H, W, int(quality), _ptr(payload), cap, _ptr(nbytes), _ptr(status),
                                             self._stream()), "ams_uplink_encode")
        return payload

    def _encoder_p(self, H: int, W: int):
        if (H, W) not in self._enc_p:
            self._enc_p[(H, W)] = (torch.empty(int(self.lib.ams_uplink_inter_encode_scratch(H, W)), dtype=torch.uint8, device=self.device),
                                   torch.empty(100, dtype=torch.int64, device=self.device), torch.empty(1, dtype=torch.int64, device=self.device),
                                   torch.empty(1, dtype=torch.int32, device=self.device))
        return self._enc_p[(H, W)]

    def _transform_p(self, src: torch.Tensor, reference: ArrayLike) -> torch.Tensor:
        """search + residual transform of the frame already on the device; -> the sizes tensor (on the device, not read back)"""
        ref = self._frame(reference)
        assert ref.shape == src.shape, "the reference is a frame of the same size: %s against %s" % (tuple(ref.shape), tuple(src.shape))
        H, W = int(src.shape[0]), int(src.shape[1])
        scratch, sizes = self._encoder_p(H, W)[:2]
        hip.check(self.lib.ams_uplink_inter_transform(_ptr(src), _ptr(ref), H, W, _ptr(scratch), scratch.numel(), self._stream()),
                  "ams_uplink_inter_transform")
        hip.check(self.lib.ams_uplink_inter_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes), self._stream()),
                  "ams_uplink_inter_size_table")
        return sizes

    def _write_p(self, H: int, W: int, quality: int, cap: int) -> torch.Tensor:
        scratch, _sizes, nbytes, status = self._encoder_p(H, W)
        payload = torch.empty(cap, dtype=torch.uint8, device=self.device)
        hip.check(self.lib.ams_uplink_inter_encode(_ptr(scratch), scratch.numel(), H, W, int(quality), _ptr(payload), cap, _ptr(nbytes),
                                                   _ptr(status), self._stream()), "ams_uplink_inter_encode")
        return payload

    def size_table(self, frame: ArrayLike, reference: Optional[ArrayLike] = None) -> np.ndarray:
        """int64 [100]: the exact payload bytes of ``frame`` at quality 1 .. 100 (one synchronisation); with ``reference`` those of AUP1."""
        with torch.cuda.device(self.device):
            if reference is not None:
                return self._transform_p(self._frame(frame), reference).cpu().numpy()
            H, W = self._transform(frame)
            return self._sizes(H, W)

    def _sizes(self, H: int, W: int) -> np.ndarray:
        scratch, sizes = self._encoder(H, W)[:2]
        hip.check(self.lib.ams_uplink_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes), self._stream()), "ams_uplink_size_table")
        return sizes.cpu().numpy()

    def encode(self, frame: ArrayLike, quality: int, reference: Optional[ArrayLike] = None) -> torch.Tensor:
        """The payload of ``frame`` at ``quality`` (1 .. 100): torch.uint8 [n] on the device; with ``reference`` the predicted kind, AUP1."""
        if not 1 <= int(quality) <= 100:
            raise ValueError("uplink codec: quality %r is outside 1 .. 100" % (quality,))
        with torch.cuda.device(self.device):
            if reference is not None:
                src = self._frame(frame)
                H, W = int(src.shape[0]), int(src.shape[1])
                self._transform_p(src, reference)
                payload = self._write_p(H, W, quality, int(self.lib.ams_uplink_inter_max_bytes(H, W)))
                _scratch, _sizes, nbytes, status = self._encoder_p(H, W)
                n, st = int(nbytes.item()), int(status.item())
                assert st == hip.UPLINK_OK, "ams_uplink_inter_encode: status %d for %d bytes" % (st, n)
                return payload[:n].clone()
            H, W = self._transform(frame)
            payload = self._write(H, W, quality, self.max_payload_bytes(H, W))
            _scratch, _sizes, nbytes, status = self._encoder(H, W)
            n, st = int(nbytes.item()), int(status.item())
            assert st == hip.UPLINK_OK, "ams_uplink_encode: status %d for %d bytes" % (st, n)
            return payload[:n].clone()

    def encode_to_budget(self, frame: ArrayLike, budget_bytes: int, reference: Optional[ArrayLike] = None) -> Tuple[torch.Tensor, int, bool]:
        """(payload, quality, fits): the largest quality whose payload has at most ``budget_bytes`` bytes; if none has, quality 1 and
        ``fits`` False.  One synchronisation, for the table of the 100 sizes.

        With ``reference`` both kinds are sized (one search and one residual transform for the 100 AUP1 sizes) and each takes its largest
        fitting quality: the kind with the larger quality wins, on equal quality the smaller payload, then AUC1; if neither fits, AUC1 at
        quality 1 and ``fits`` False.  ``kind_of(payload)`` tells which kind came out.  Still one synchronisation."""
        if reference is not None:
            with torch.cuda.device(self.device):
                src = self._frame(frame)
                H, W = int(src.shape[0]), int(src.shape[1])
                sizes_p = self._transform_p(src, reference)
                self._transform(src)
                scratch, sizes_i = self._encoder(H, W)[:2]
                hip.check(self.lib.ams_uplink_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes_i), self._stream()), "ams_uplink_size_table")
                both = torch.stack([sizes_i, sizes_p]).cpu().numpy()
                kind, quality, fits = choose_kind(both[0], both[1], int(budget_bytes))
                if kind == INTER:
                    return self._write_p(H, W, quality, int(both[1][quality - 1])), quality, fits
                return self._write(H, W, quality, int(both[0][quality - 1])), quality, fits
        with torch.cuda.device(self.device):
            H, W = self._transform(frame)
            sizes = self._sizes(H, W)
            fit = np.nonzero(sizes <= int(budget_bytes))[0]
            quality, fits = (int(fit[-1]) + 1, True) if len(fit) else (1, False)
            return self._write(H, W, quality, int(sizes[quality - 1])), quality, fits

    def decode(self, payload, size: Optional[Tuple[int, int]] = None, reference: Optional[ArrayLike] = None) -> torch.Tensor:
        """uint8 [H, W, 3] on the device from a payload (bytes, a host array or a device tensor); ``size`` = (H, W) spares reading the header
        back.  Raises UplinkRefused on a payload the device refuses; one synchronisation for the status.  With ``reference`` the payload is
        taken for a predicted frame (AUP1) of the reference's size; an AUP1 payload without one raises ValueError."""
        if isinstance(payload, (bytes, bytearray, memoryview)):
            payload = np.frombuffer(bytes(payload), np.uint8).copy()
        t = payload if isinstance(payload, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(payload))
        assert t.dtype == torch.uint8 and t.dim() == 1, "a payload is uint8 [n], got %s %s" % (t.dtype, tuple(t.shape))
        if reference is not None:
            return self._decode_p(t, reference)
        if size is None:
            if t.numel() < 8:
                raise UplinkRefused(hip.UPLINK_BAD_HEADER)
            head = t[4:8].cpu().numpy().astype(np.int64)
            size = (int(head[0] | head[1] << 8), int(head[2] | head[3] << 8))
        H, W = size
        if int(self.lib.ams_uplink_max_bytes(H, W)) == 0:
            raise UplinkRefused(hip.UPLINK_BAD_HEADER)
        t = t.to(self.device, non_blocking=True).contiguous()
        with torch.cuda.device(self.device):
            if (H, W) not in self._dec:
                self._dec[(H, W)] = (torch.empty(int(self.lib.ams_uplink_decode_scratch(H, W)), dtype=torch.uint8, device=self.device),
                                     torch.empty(1, dtype=torch.int32, device=self.device))
            scratch, status = self._dec[(H, W)]
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            hip.check(self.lib.ams_uplink_decode(_ptr(t), t.numel(), H, W, _ptr(out), _ptr(status), _ptr(scratch), scratch.numel(), self._stream()),
                      "ams_uplink_decode")
            st = int(status.item())
        if st == hip.UPLINK_BAD_HEADER and t.numel() >= 4 and kind_of(t) == INTER:      # (read back only once the device has refused)
            raise ValueError("uplink codec: an AUP1 payload is a prediction from the previous decoded frame: decode(payload, reference=...) needs it")
        if st != hip.UPLINK_OK:
            raise UplinkRefused(st)
        return out

    def _decode_p(self, t: torch.Tensor, reference: ArrayLike) -> torch.Tensor:
        ref = self._frame(reference)
        H, W = int(ref.shape[0]), int(ref.shape[1])
        t = t.to(self.device, non_blocking=True).contiguous()
        with torch.cuda.device(self.device):
            if (H, W) not in self._dec_p:
                self._dec_p[(H, W)] = (torch.empty(int(self.lib.ams_uplink_inter_decode_scratch(H, W)), dtype=torch.uint8, device=self.device),
                                       torch.empty(1, dtype=torch.int32, device=self.device))
            scratch, status = self._dec_p[(H, W)]
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=self.device)
            hip.check(self.lib.ams_uplink_inter_decode(_ptr(t), t.numel(), _ptr(ref), H, W, _ptr(out), _ptr(status), _ptr(scratch), scratch.numel(),
                                                       self._stream()), "ams_uplink_inter_decode")
            st = int(status.item())
        if st != hip.UPLINK_OK:
            raise UplinkRefused(st)
        return out
