"""A streaming animated-GIF writer: the ``video.gif`` the reference's viewer saves with
``images[0].save(..., save_all=True, duration=10, loop=0)`` (playback.py:131-138), fed with the image data of frames such
as `Crate.render_gif` returns.

Layout::

    'GIF89a'
    logical screen descriptor      width, height, a global palette of 256 entries
    the palette                    entry 0 is black, entry k is (k, k, 255): the colours of `Crate.render`
    application extension          'NETSCAPE2.0', the loop count (0 = for ever)
    per frame
      graphic control extension    the delay in 1/100 s
      image descriptor             the whole screen, no local palette, not interlaced
      image data                   LZW minimum code size, data sub-blocks, terminator: what `write` is given
    0x3B

The header goes out when the file is opened, one frame per `write`, the trailer at `close()`: nothing is kept in memory.
One loss against `Crate.render`: its colour (0, 0, 255) (a pressure of 1 and above) is palette entry 1, (1, 1, 255).
A writer opened with ``arrows=True`` takes frames rendered with debug arrows: entry 1 is their green, (0, 255, 0), and
the loss is that (0, 0, 255) and (1, 1, 255) are both entry 2, (2, 2, 255).
"""
from __future__ import annotations

import struct
from pathlib import Path


def palette(arrows: bool = False) -> bytes:
    """The 768 bytes of the global colour table.  `arrows`: entry 1 is the debug arrows' green, (0, 255, 0), as frames
    rendered with arrows use it (their discs start at entry 2: colour bytes 0 and 1 both become (2, 2, 255))."""
    table = bytes(3) + b"".join(bytes((k, k, 255)) for k in range(1, 256))
    return table[:3] + bytes((0, 255, 0)) + table[6:] if arrows else table


class GifWriter:
    def __init__(self, path, width: int, height: int, delay_cs: int = 1, loop: int = 0, arrows: bool = False):
        if not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
            raise ValueError("width and height must be 1..65535")
        if not (0 <= int(delay_cs) <= 65535 and 0 <= int(loop) <= 65535):
            raise ValueError("delay_cs and loop must be 0..65535")
        self.path = Path(path)
        self.width, self.height, self.delay_cs, self.loop = int(width), int(height), int(delay_cs), int(loop)
        self._frames = 0
        self._f = open(self.path, "wb")
        self._f.write(b"GIF89a" + struct.pack("<HHBBB", self.width, self.height, 0xF7, 0, 0) + palette(arrows)
                      + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", self.loop) + b"\x00")

    @property
    def frames(self) -> int:
        return self._frames

    def write(self, image_data: bytes) -> None:
        """Appends one frame: its image data (minimum code size 8, sub-blocks, terminator) over the writer's palette."""
        if self._f is None:
            raise ValueError("the GIF writer is closed")
        data = bytes(image_data)
        if len(data) < 3 or data[0] != 8 or data[-1] != 0:
            raise ValueError("not the image data of a frame: expected the minimum code size 8 ... a terminating 0")
        self._f.write(b"\x21\xF9\x04\x00" + struct.pack("<H", self.delay_cs) + b"\x00\x00"
                      + b"\x2C" + struct.pack("<HHHHB", 0, 0, self.width, self.height, 0) + data)
        self._frames += 1

    def close(self) -> None:
        """Writes the trailer."""
        f = self._f
        if f is None:
            return
        self._f = None
        try:
            f.write(b"\x3B")
        finally:
            f.close()

    def __enter__(self) -> "GifWriter":
        return self

    def __exit__(self, *exc) -> None:
        self.close()
