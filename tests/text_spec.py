"""The pixel rule of the HUD overlay (sc_set_hud; sand_crate_amd/csrc/sc_hud.h), written once in NumPy.

The device frame with a HUD equals `draw(the frame without one, ...)` bit for bit.

font     sand_crate_amd/hud_font.py: ASCII 0x20..0x7E in a cell of 8 x 16 pixels, one byte per row, most significant
         bit leftmost.  Any other byte except ``\\n`` draws the glyph of ``?``.
lines    the text is split at ``\\n`` (byte 10); a trailing ``\\n`` yields an empty last line, as str.split does.
place    line l starts at pixel row y + l 18 scale, character k of a line at pixel column x + k 8 scale.
scale    a glyph bit covers scale x scale pixels; the last 2 scale rows of a line's 18 scale are leading, never drawn.
ink      a set bit writes white -- (255, 255, 255) into an H x W x 3 RGB frame, 255 into an H x W image of palette
         indices (tests/gif_spec.py) -- and a clear bit leaves what is underneath.
clip     pixels outside the frame are dropped: a glyph cut by the right or bottom edge shows the part that fits, an
         origin outside the frame draws nothing.  x and y are 0..16384, scale 1..64.
default  x = y = 6 (TEXT_MARGIN, playback.py:22); scale = max(1, (width // 60 + 8) // 16), the reference's font size
         of width // 60 pixels (playback.py:215) in whole multiples of the 16-pixel cell.

The product never imports this module.
"""
from __future__ import annotations

import numpy as np

from sand_crate_amd import hud_font as F

PITCH = 18  # rows of cell pixels from one line to the next: our choice, standing in for pygame's line size
MARGIN = 6


def default_scale(width: int) -> int:
    return max(1, (width // 60 + 8) // 16)


def lines(text: bytes) -> list[bytes]:
    return bytes(text).split(b"\n")


def glyph_bits(byte: int) -> np.ndarray:
    """16 x 8 bool: the glyph drawn for this byte value."""
    k = (byte if 0x20 <= byte <= 0x7E else ord("?")) - 0x20
    rows = np.frombuffer(F.FONT, dtype=np.uint8)[16 * k:16 * k + 16]
    return np.unpackbits(rows[:, None], axis=1).astype(bool)


def ink(text: bytes, x: int, y: int, scale: int, width: int, height: int) -> np.ndarray:
    """height x width bool: the pixels the text writes."""
    assert 0 <= x <= 16384 and 0 <= y <= 16384 and 1 <= scale <= 64
    mask = np.zeros((height, width), dtype=bool)
    for l, line in enumerate(lines(text)):
        top = y + l * PITCH * scale
        if top >= height:
            break
        for k, byte in enumerate(line):
            left = x + k * 8 * scale
            if left >= width:
                break
            cell = np.repeat(np.repeat(glyph_bits(byte), scale, axis=0), scale, axis=1)
            part = cell[:height - top, :width - left]
            mask[top:top + part.shape[0], left:left + part.shape[1]] |= part
    return mask


def draw(frame, text: bytes, x: int = MARGIN, y: int = MARGIN, scale: int = 1) -> np.ndarray:
    """A copy of `frame` -- H x W x 3 RGB or H x W palette indices, uint8 -- with the text on it."""
    out = np.array(frame, dtype=np.uint8)
    assert out.ndim in (2, 3) and (out.ndim == 2 or out.shape[2] == 3)
    out[ink(text, x, y, scale, out.shape[1], out.shape[0])] = 255
    return out


def box(text: bytes, x: int, y: int, scale: int, width: int, height: int) -> tuple[int, int]:
    """(columns, rows) of the text's bounding box clipped to the frame, (0, 0) when it is empty: what the overlay
    kernel's grid covers."""
    ls = lines(text)
    w = min(width - x, max(len(line) for line in ls) * 8 * scale)
    h = min(height - y, len(ls) * PITCH * scale)
    return (w, h) if w > 0 and h > 0 else (0, 0)
