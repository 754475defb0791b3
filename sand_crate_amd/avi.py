"""A streaming Motion-JPEG AVI 1.0 writer: the ``video.avi`` the reference's viewer writes with
``cv2.VideoWriter(..., 'MJPG', 50, (screen_x, screen_y))`` (playback.py:120-129), fed with JPEG files such as
`Crate.render_jpeg` returns.

Layout::

    RIFF 'AVI '
      LIST 'hdrl'
        'avih'                     main header (frame count, size, microseconds per frame)
        LIST 'strl'
          'strh'                   'vids' stream, handler 'MJPG', rate / scale = fps
          'strf'                   BITMAPINFOHEADER, compression 'MJPG'
      LIST 'movi'
        '00dc' ...                 one chunk per frame, padded to even length
      'idx1'                       per frame: '00dc', AVIIF_KEYFRAME, offset from the 'movi' fourcc, size

Frames are written as they come; the sizes and counts in the headers are patched by `close()`.  AVI 1.0 stops at
RIFF sizes of 2^32 - 1 bytes: a frame that would pass it raises `ValueError` before anything is written (OpenDML,
the extension beyond it, is not supported).
"""
from __future__ import annotations

import struct
from fractions import Fraction
from pathlib import Path

AVIF_HASINDEX = 0x10
AVIIF_KEYFRAME = 0x10
RIFF_LIMIT = 2 ** 32 - 1


class AviWriter:
    def __init__(self, path, width: int, height: int, fps: float = 50):
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError("width and height must be 1..65535")
        rate = Fraction(fps).limit_denominator(1000000)
        if rate <= 0:
            raise ValueError("fps must be positive")
        self.path = Path(path)
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        self._rate, self._scale = rate.numerator, rate.denominator
        self._index: list[tuple[int, int]] = []  # (offset from the 'movi' fourcc, size) per frame
        self._largest = 0
        self._f = open(self.path, "wb")
        self._write_headers()

    @property
    def frames(self) -> int:
        return len(self._index)

    def _write_headers(self) -> None:
        f = self._f
        f.write(b"RIFF" + struct.pack("<I", 0) + b"AVI ")
        hdrl = bytearray()
        self._avih_at = 12 + 12 + 8  # RIFF header, LIST 'hdrl' header, 'avih' chunk header
        hdrl += b"avih" + struct.pack("<I", 56) + self._avih()
        strh = self._strh()
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG",
                           min(3 * self.width * self.height, RIFF_LIMIT),
                           0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        self._strh_at = self._avih_at + 56 + 12 + 8  # + the 'strl' LIST header and the 'strh' chunk header
        hdrl += b"LIST" + struct.pack("<I", len(strl)) + strl
        f.write(b"LIST" + struct.pack("<I", 4 + len(hdrl)) + b"hdrl" + hdrl)
        self._movi_at = f.tell()  # the LIST header of 'movi'
        f.write(b"LIST" + struct.pack("<I", 0) + b"movi")
        self._end = f.tell()

    def _avih(self) -> bytes:
        usec = round(1e6 * self._scale / self._rate)
        return struct.pack("<10I4I", usec, 0, 0, AVIF_HASINDEX, len(self._index), 0, 1, self._largest, self.width,
                           self.height, 0, 0, 0, 0)

    def _strh(self) -> bytes:
        return struct.pack("<4s4sIHH8Ihhhh", b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate, 0,
                           len(self._index), self._largest, 0xFFFFFFFF, 0, 0, 0, min(self.width, 32767),
                           min(self.height, 32767))

    def _riff_size(self, movi_end: int, frames: int) -> int:
        return movi_end + 8 + 16 * frames - 8  # + 'idx1' header and entries, - the RIFF header itself

    def write(self, jpeg: bytes) -> None:
        """Appends one frame (a JPEG file)."""
        if self._f is None:
            raise ValueError("the AVI writer is closed")
        data = bytes(jpeg)
        n = len(data)
        end = self._end + 8 + n + (n & 1)
        if self._riff_size(end, len(self._index) + 1) > RIFF_LIMIT:
            raise ValueError(f"{self.path}: this frame would take the AVI past 4 GiB, the limit of AVI 1.0 "
                             "(OpenDML is not supported)")
        self._f.write(b"00dc" + struct.pack("<I", n) + data + (b"\0" if n & 1 else b""))
        self._index.append((self._end - (self._movi_at + 8), n))
        self._largest = max(self._largest, n)
        self._end = end

    def close(self) -> None:
        """Writes the index and patches the header sizes."""
        f = self._f
        if f is None:
            return
        self._f = None
        try:
            f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
            f.write(b"".join(b"00dc" + struct.pack("<III", AVIIF_KEYFRAME, off, n) for off, n in self._index))
            f.seek(4)
            f.write(struct.pack("<I", self._riff_size(self._end, len(self._index))))
            f.seek(self._avih_at)
            f.write(self._avih())
            f.seek(self._strh_at)
            f.write(self._strh())
            f.seek(self._movi_at + 4)
            f.write(struct.pack("<I", self._end - (self._movi_at + 8)))
        finally:
            f.close()

    def __enter__(self) -> "AviWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()
