"""The uplink frame codec on the device (k_uplink.hip; format AUC1, stated in include/ams_hip.h): what ``run.py --compress_uplink`` sends.

    codec = UplinkCodec(device)
    payload, quality, fits = codec.encode_to_budget(frame_u8, budget_bytes)      # torch.uint8 [n] on the device
    frame = codec.decode(payload)                                                # torch.uint8 [H, W, 3] on the device

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
                hip.UPLINK_NO_ROOM: "no room for the payload"}


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

    def size_table(self, frame: ArrayLike) -> np.ndarray:
        """int64 [100]: the exact payload bytes of ``frame`` at quality 1 .. 100 (one synchronisation)."""
        with torch.cuda.device(self.device):
            H, W = self._transform(frame)
            return self._sizes(H, W)

    def _sizes(self, H: int, W: int) -> np.ndarray:
        scratch, sizes = self._encoder(H, W)[:2]
        hip.check(self.lib.ams_uplink_size_table(_ptr(scratch), scratch.numel(), H, W, _ptr(sizes), self._stream()), "ams_uplink_size_table")
        return sizes.cpu().numpy()

    def encode(self, frame: ArrayLike, quality: int) -> torch.Tensor:
        """The payload of ``frame`` at ``quality`` (1 .. 100): torch.uint8 [n] on the device."""
        if not 1 <= int(quality) <= 100:
            raise ValueError("uplink codec: quality %r is outside 1 .. 100" % (quality,))
        with torch.cuda.device(self.device):
            H, W = self._transform(frame)
            payload = self._write(H, W, quality, self.max_payload_bytes(H, W))
            _scratch, _sizes, nbytes, status = self._encoder(H, W)
            n, st = int(nbytes.item()), int(status.item())
            assert st == hip.UPLINK_OK, "ams_uplink_encode: status %d for %d bytes" % (st, n)
            return payload[:n].clone()

    def encode_to_budget(self, frame: ArrayLike, budget_bytes: int) -> Tuple[torch.Tensor, int, bool]:
        """(payload, quality, fits): the largest quality whose payload has at most ``budget_bytes`` bytes; if none has, quality 1 and
        ``fits`` False.  One synchronisation, for the table of the 100 sizes."""
        with torch.cuda.device(self.device):
            H, W = self._transform(frame)
            sizes = self._sizes(H, W)
            fit = np.nonzero(sizes <= int(budget_bytes))[0]
            quality, fits = (int(fit[-1]) + 1, True) if len(fit) else (1, False)
            return self._write(H, W, quality, int(sizes[quality - 1])), quality, fits

    def decode(self, payload, size: Optional[Tuple[int, int]] = None) -> torch.Tensor:
        """uint8 [H, W, 3] on the device from a payload (bytes, a host array or a device tensor); ``size`` = (H, W) spares reading the header
        back.  Raises UplinkRefused on a payload the device refuses; one synchronisation for the status."""
        if isinstance(payload, (bytes, bytearray, memoryview)):
            payload = np.frombuffer(bytes(payload), np.uint8).copy()
        t = payload if isinstance(payload, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(payload))
        assert t.dtype == torch.uint8 and t.dim() == 1, "a payload is uint8 [n], got %s %s" % (t.dtype, tuple(t.shape))
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
        if st != hip.UPLINK_OK:
            raise UplinkRefused(st)
        return out
