"""The texts and placements the HUD overlay is tested on (tests/test_gpu_hud.py), each built to put one property of the
pixel rule of tests/text_spec.py to the test; tests/test_hud_cpu.py checks the rule itself on them on the CPU.

`cases()` -> {name: Case}.  A case is a text, its origin and scale, a frame size, and -- worked out by hand from the rule,
not taken from the specification's code -- the text's bounding box clipped to the frame as (columns, rows): columns
min(width - x, longest line * 8 * scale), rows min(height - y, lines * 18 * scale), (0, 0) when either is not positive.

cut            64 x 48: a line of ten characters (80 pixels) is cut by the right edge two columns into its eighth glyph,
               a `T`, whose bar starts in column 0; the third of four lines is cut by the bottom edge, the fourth unseen
odd            61 x 37: neither side a multiple of four, the last glyph loses its last column
scale_2/_3     96 x 80: every glyph bit a block of 2 x 2 / 3 x 3 pixels; at 3 both edges cut
corner         the origin on the frame's last pixel: a box of 1 x 1
outside        the origin at (width, 0): nothing is drawn
empty_middle   two empty lines between two others
trailing       a trailing newline: an empty last line, which counts for the box
only_newline   two empty lines and nothing else: an empty box
longest_first  the longest line first: the shorter ones must not draw up to its end
all_glyphs     the 95 glyphs, sixteen to a line, and the bytes 0x00, 0x09, 0x7F and 0xFF, which are drawn as `?`
"""
from __future__ import annotations

import functools
from typing import NamedTuple


class Case(NamedTuple):
    text: bytes
    x: int
    y: int
    scale: int
    width: int
    height: int
    box: tuple  # (columns, rows) of the clipped bounding box


def all_glyphs_text() -> bytes:
    codes = bytes(range(0x20, 0x7F)) + bytes([0x00, 0x09, 0x7F, 0xFF])
    return b"\n".join(codes[k:k + 16] for k in range(0, len(codes), 16))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    return {
        # 10 characters = 80 columns > 64 - 6; 4 lines = 72 rows > 48 - 6
        "cut": Case(b"TWTWTWTTWT\n(|b|(|b\n|b(|WT|W|b\nunseen", 6, 6, 1, 64, 48, (58, 42)),
        # 7 characters = 56 columns > 61 - 6 = 55; 2 lines = 36 rows > 37 - 6 = 31
        "odd": Case(b"Tick: 7\nP=#42", 6, 6, 1, 61, 37, (55, 31)),
        # 3 characters * 16 = 48 columns; 2 lines * 36 = 72 rows < 80 - 5
        "scale_2": Case(b"Ab1\n{g}", 3, 5, 2, 96, 80, (48, 72)),
        # 4 characters * 24 = 96 columns > 96 - 1; 2 lines * 54 = 108 rows > 80 - 2
        "scale_3": Case(b"Wq@y\nj", 1, 2, 3, 96, 80, (95, 78)),
        "corner": Case(b"TW\nx", 63, 47, 1, 64, 48, (1, 1)),
        "outside": Case(b"TW\nx", 64, 0, 1, 64, 48, (0, 0)),
        # 2 characters = 16 columns; 4 lines = 72 rows < 80 - 6
        "empty_middle": Case(b"ab\n\n\ncd", 6, 6, 1, 48, 80, (16, 72)),
        "trailing": Case(b"xyz\n", 6, 6, 1, 64, 48, (24, 36)),
        "only_newline": Case(b"\n", 6, 6, 1, 64, 48, (0, 0)),
        # 12 characters = 96 columns < 112 - 6; 4 lines = 72 rows < 80 - 6
        "longest_first": Case(b"longest line\nshort\nmid size\n.", 6, 6, 1, 112, 80, (96, 72)),
        # 16 characters = 128 columns < 140 - 6; 99 bytes in 7 lines = 126 rows < 136 - 6
        "all_glyphs": Case(all_glyphs_text(), 6, 6, 1, 140, 136, (128, 126)),
    }
