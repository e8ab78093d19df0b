"""A small PNG writer (zlib and struct only; there is no OpenCV here): 8-bit RGB [H, W, 3] and 8-bit grey [H, W] images, filter type 0 on
every row, one fixed compression level, so that two runs over the same array give the same bytes.  What ``run.py --save_pic`` writes its
pictures with (reference run.py:445-454, cv2.imwrite)."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
LEVEL = 6                      # fixed: the bytes of a file depend on the image alone


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)


def encode(image) -> bytes:
    a = np.asarray(image)
    assert a.dtype == np.uint8, "8-bit images only, got %s" % a.dtype
    assert a.ndim == 2 or (a.ndim == 3 and a.shape[2] == 3), "grey [H, W] or RGB [H, W, 3], got %s" % (a.shape,)
    h, w = a.shape[:2]
    assert h > 0 and w > 0
    colour_type = 0 if a.ndim == 2 else 2
    rows = np.zeros((h, 1 + w * (1 if a.ndim == 2 else 3)), dtype=np.uint8)          # a filter byte (0 = None) in front of every row
    rows[:, 1:] = a.reshape(h, -1)
    ihdr = struct.pack(">IIBBBBB", w, h, 8, colour_type, 0, 0, 0)
    return SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), LEVEL)) + _chunk(b"IEND", b"")


def write(path: str, image) -> None:
    with open(path, "wb") as f:
        f.write(encode(image))
