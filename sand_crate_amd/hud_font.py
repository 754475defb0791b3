"""The HUD's built-in bitmap font: 95 glyphs, ASCII 0x20..0x7E, in a cell of 8 x 16 pixels, one byte per row, most
significant bit leftmost -- 1520 bytes.  This table is the source of truth; ``csrc/sc_font.h`` is the same table as a C
array, emitted by `c_header()` (``python -m sand_crate_amd.hud_font`` prints it) and committed, and
``docs/hud_font.txt`` is `specimen()` (``python -m sand_crate_amd.hud_font --specimen``).  Nothing regenerates the table:
no build or test step needs a font file or an imaging library.

The reference draws its HUD with pygame's ``SysFont("monospace", screen_x // 60)`` (playback.py:215-219), which is
whatever the machine has, antialiased.  This font is not antialiased: a glyph bit is a white pixel, nothing else.  Rows
0 and 15 and the rightmost column of every glyph are empty, so neighbouring letters and lines never touch.

Where the glyphs come from: DejaVu Sans Mono at 12 pixels per em, rasterised once without antialiasing and then cleaned
up by hand.  The face's licence asks for this notice to travel with it:

    Fonts are (c) Bitstream (see below). DejaVu changes are in public domain.

    Bitstream Vera Fonts Copyright
    ------------------------------

    Copyright (c) 2003 by Bitstream, Inc. All Rights Reserved. Bitstream Vera is
    a trademark of Bitstream, Inc.

    Permission is hereby granted, free of charge, to any person obtaining a copy
    of the fonts accompanying this license ("Fonts") and associated
    documentation files (the "Font Software"), to reproduce and distribute the
    Font Software, including without limitation the rights to use, copy, merge,
    publish, distribute, and/or sell copies of the Font Software, and to permit
    persons to whom the Font Software is furnished to do so, subject to the
    following conditions:

    The above copyright and trademark notices and this permission notice shall
    be included in all copies of one or more of the Font Software typefaces.

    The Font Software may be modified, altered, or added to, and in particular
    the designs of glyphs or characters in the Fonts may be modified and
    additional glyphs or characters may be added to the Fonts, only if the fonts
    are renamed to names not containing either the words "Bitstream" or the word
    "Vera".

    This License becomes null and void to the extent applicable to Fonts or Font
    Software that has been modified and is distributed under the "Bitstream
    Vera" names.

    The Font Software may be sold as part of a larger software package but no
    copy of one or more of the Font Software typefaces may be sold by itself.

    THE FONT SOFTWARE IS PROVIDED "AS IS", WITHOUT WARRANTY OF ANY KIND, EXPRESS
    OR IMPLIED, INCLUDING BUT NOT LIMITED TO ANY WARRANTIES OF MERCHANTABILITY,
    FITNESS FOR A PARTICULAR PURPOSE AND NONINFRINGEMENT OF COPYRIGHT, PATENT,
    TRADEMARK, OR OTHER RIGHT. IN NO EVENT SHALL BITSTREAM OR THE GNOME
    FOUNDATION BE LIABLE FOR ANY CLAIM, DAMAGES OR OTHER LIABILITY, INCLUDING
    ANY GENERAL, SPECIAL, INDIRECT, INCIDENTAL, OR CONSEQUENTIAL DAMAGES,
    WHETHER IN AN ACTION OF CONTRACT, TORT OR OTHERWISE, ARISING FROM, OUT OF
    THE USE OR INABILITY TO USE THE FONT SOFTWARE OR FROM OTHER DEALINGS IN THE
    FONT SOFTWARE.

    Except as contained in this notice, the names of Gnome, the Gnome
    Foundation, and Bitstream Inc., shall not be used in advertising or
    otherwise to promote the sale, use or other dealings in this Font Software
    without prior written authorization from the Gnome Foundation or Bitstream
    Inc., respectively. For further information, contact: fonts at gnome dot
    org.
"""
from __future__ import annotations

import sys

CELL_W, CELL_H = 8, 16
FIRST, LAST = 0x20, 0x7E       # the glyphs' codes; any other byte is drawn as `?`
GLYPHS = LAST - FIRST + 1
LINE_PITCH = 18                # rows from one line to the next, in cell pixels: 16 of glyph, 2 of leading
MARGIN = 6                     # TEXT_MARGIN, playback.py:22

# One glyph per line: its 16 rows, top to bottom, two hex digits each.
_ROWS = (
    "00000000000000000000000000000000"  # space
    "00000010101010101000101000000000"  # !
    "00000028282800000000000000000000"  # "
    "0000000014247e2828fc485000000000"  # #
    "00000010385450701c14543810100000"  # $
    "00000060909064186c12120c00000000"  # %
    "0000001c202030304a4e643a00000000"  # &
    "00000010101000000000000000000000"  # '
    "00000c0808101010101008080c000000"  # (
    "00003010100808080808101030000000"  # )
    "00000010543838541000000000000000"  # *
    "0000000000101010fe10101000000000"  # +
    "00000000000000000000101020000000"  # ,
    "00000000000000007c00000000000000"  # -
    "00000000000000000000101000000000"  # .
    "00000002040408081010202040000000"  # /
    "0000003c2442424a4242243c00000000"  # 0
    "00000070101010101010107c00000000"  # 1
    "0000003c420202040810207e00000000"  # 2
    "0000003c4202021c0202423c00000000"  # 3
    "0000000c0c143424447e040400000000"  # 4
    "0000007c40407c060202463c00000000"  # 5
    "0000001c22405c664242263c00000000"  # 6
    "0000007e060404080810102000000000"  # 7
    "0000003c4242423c4242423c00000000"  # 8
    "0000003c644242463a02443800000000"  # 9
    "00000000000010100000101000000000"  # :
    "00000000000010100000101020000000"  # ;
    "0000000000021c60601c020000000000"  # <
    "000000000000007e007e000000000000"  # =
    "00000000004038060638400000000000"  # >
    "0000001c22020c181000101000000000"  # ?
    "000000001c26424e52524e60201c0000"  # @
    "0000001818182424243c424200000000"  # A
    "0000007c4242427c4242427c00000000"  # B
    "0000001c224040404040221c00000000"  # C
    "00000078444242424242447800000000"  # D
    "0000007e4040407e4040407e00000000"  # E
    "0000007e4040407e4040404000000000"  # F
    "0000001c224040464242221c00000000"  # G
    "000000424242427e4242424200000000"  # H
    "0000007c101010101010107c00000000"  # I
    "0000001c040404040404443800000000"  # J
    "0000004244485070484c444200000000"  # K
    "00000040404040404040407e00000000"  # L
    "0000004266665a5a5a42424200000000"  # M
    "000000626252525a4a4a464600000000"  # N
    "0000003c244242424242243c00000000"  # O
    "0000007c4242427c4040404000000000"  # P
    "0000003c244242424242263c04040000"  # Q
    "0000007c4242427c4442424200000000"  # R
    "0000003c4240603c0202423c00000000"  # S
    "000000fe101010101010101000000000"  # T
    "00000042424242424242423c00000000"  # U
    "00000042422424242418181800000000"  # V
    "000000829292aaaaaa6c444400000000"  # W
    "00000042242418181824244200000000"  # X
    "00000082442828101010101000000000"  # Y
    "0000007e060408181020607e00000000"  # Z
    "00001810101010101010101018000000"  # [
    "00000040202010100808040402000000"  # \
    "00003010101010101010101030000000"  # ]
    "00000030488400000000000000000000"  # ^
    "0000000000000000000000000000fe00"  # _
    "00001008000000000000000000000000"  # `
    "00000000003844043c44443c00000000"  # a
    "00004040407844444444447800000000"  # b
    "00000000003864404040603c00000000"  # c
    "00000404043c44444444443c00000000"  # d
    "00000000003864447c40443800000000"  # e
    "00000c10107c10101010101000000000"  # f
    "00000000003c44444444443c04241800"  # g
    "00004040405864444444444400000000"  # h
    "00001000007010101010107c00000000"  # i
    "00000800003808080808080808083000"  # j
    "00004040404448506050484400000000"  # k
    "00007010101010101010100c00000000"  # l
    "00000000007c54545454545400000000"  # m
    "00000000005864444444444400000000"  # n
    "00000000003844444444443800000000"  # o
    "00000000007844444444447840404000"  # p
    "00000000003c44444444443c04040400"  # q
    "00000000005c62404040404000000000"  # r
    "00000000003844403804443800000000"  # s
    "00000010107c10101010101c00000000"  # t
    "00000000004444444444443c00000000"  # u
    "00000000004444282828101000000000"  # v
    "0000000000828254546c282800000000"  # w
    "00000000004428281028284400000000"  # x
    "00000000004444282828301010206000"  # y
    "00000000007c04081020407c00000000"  # z
    "00001c1010101060101010101c000000"  # {
    "00001010101010101010101010100000"  # |
    "000070101010100c1010101070000000"  # }
    "00000000000000324c00000000000000"  # ~
)
FONT = bytes.fromhex("".join(_ROWS))
assert len(FONT) == GLYPHS * CELL_H


def glyph(byte: int) -> bytes:
    """The 16 rows of the glyph drawn for this byte value."""
    k = (byte if FIRST <= byte <= LAST else ord("?")) - FIRST
    return FONT[k * CELL_H:(k + 1) * CELL_H]


def default_scale(width: int) -> int:
    """The reference's font size is ``width // 60`` pixels (playback.py:215); rounded to whole multiples of the
    16-pixel cell, at least one: 1 at its 1000-pixel screen, 2 from 1440 up."""
    return max(1, (int(width) // 60 + 8) // 16)


def default_placement(width: int) -> tuple[int, int, int]:
    """(x, y, scale) of the HUD on a frame this wide: the reference's margin, the scale of `default_scale`."""
    return MARGIN, MARGIN, default_scale(width)


def c_header() -> str:
    """csrc/sc_font.h, to the byte."""
    out = ["// The HUD font (sc_hud.h): 95 glyphs, ASCII 0x20..0x7E, 8 x 16 pixels, one byte per row, most significant bit",
           "// leftmost.  Generated from sand_crate_amd/hud_font.py, which is the source of truth and carries the licence",
           "// notice of the face the glyphs were drawn from:  python -m sand_crate_amd.hud_font > sand_crate_amd/csrc/sc_font.h",
           "#pragma once",
           "",
           "namespace sc {",
           "",
           f"constexpr int kFontFirst = 0x{FIRST:02X}, kFontLast = 0x{LAST:02X}, kFontRows = {CELL_H}, kFontCols = {CELL_W};",
           "",
           f"constexpr unsigned char kFontTable[{GLYPHS * CELL_H}] = {{"]
    for k in range(GLYPHS):
        rows = ", ".join(f"0x{b:02X}" for b in FONT[k * CELL_H:(k + 1) * CELL_H])
        out.append(f"    {rows},  // 0x{FIRST + k:02X}")
    out += ["};", "", "}  // namespace sc", ""]
    return "\n".join(out)


def specimen(per_row: int = 8) -> str:
    """docs/hud_font.txt: every glyph as ASCII art, `per_row` cells side by side."""
    out = [f"The HUD font of sand_crate_amd/hud_font.py: {GLYPHS} glyphs in cells of {CELL_W} x {CELL_H} pixels "
           "(# = white, . = untouched).", ""]
    for k0 in range(0, GLYPHS, per_row):
        codes = range(FIRST + k0, min(FIRST + k0 + per_row, LAST + 1))
        out.append("  ".join(f"0x{c:02X} {chr(c)}".ljust(CELL_W) for c in codes).rstrip())
        for r in range(CELL_H):
            out.append("  ".join("".join("#" if glyph(c)[r] & (0x80 >> b) else "." for b in range(CELL_W)) for c in codes))
        out.append("")
    return "\n".join(out)


if __name__ == "__main__":
    sys.stdout.write(specimen() if "--specimen" in sys.argv[1:] else c_header())
