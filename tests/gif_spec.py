"""The GIF bitstream of `sc_gif_encode_device` / `sc_render_gif` (sand_crate_amd/csrc/sc_gif.h) and the file
`sand_crate_amd.gif.GifWriter` writes, written once in Python/NumPy.

The device output equals `image_data(idx)` byte for byte; a GifWriter's file equals `file(...)`.

palette  256 entries: entry 0 is (0, 0, 0), entry k is (k, k, 255) for k = 1..255.
indices  of a frame of tests/render_spec.py: background -> 0, a disc of colour byte c -> max(c, 1), a wall -> 255.  The
         only loss: (0, 0, 255), a pressure of 1 and above, is stored as (1, 1, 255).
LZW      minimum code size 8: clear = 256, end = 257, first free code 258.  The indices in row-major order are cut into
         chunks of 1024 pixels (the last may be shorter), each coded on its own: a clear code at the current width, then
         width = 9, next = 258, an empty dictionary.  Greedy longest match; each time a code goes out because the match
         cannot be extended, the new string gets code `next`, then `if next == 1 << width: width += 1`, `next += 1`.  At
         the chunk's end the pending prefix goes out and the same two steps run once more without adding a string (a
         decoder adds one there).  The next clear code -- or the end code after the last chunk -- uses that width; the
         width before the very first clear is 9.  A chunk adds at most 1023 strings: next <= 1282, width <= 11, the
         dictionary is never full.
packing  LSB first into one bit stream for the whole frame (chunks are not byte-aligned), the last byte zero-padded.
data     0x08, the packed bytes in sub-blocks of 255 each preceded by its length (the last shorter, never empty), 0x00.
file     GIF89a; logical screen descriptor (W, H uint16 LE, 0xF7, 0, 0); the palette; the NETSCAPE2.0 application
         extension with the loop count; per frame a graphic control extension 21 F9 04 00 <delay_cs uint16> 00 00, an image
         descriptor 2C 0 0 W H 00 and the image data; 0x3B.

`decode` is an ordinary GIF LZW decoder (it knows nothing of the chunks), so that tests can read files without PIL.

The product never imports this module.
"""
from __future__ import annotations

import struct

import numpy as np

CHUNK = 1024
CLEAR, END, FIRST = 256, 257, 258


def palette() -> np.ndarray:
    """256 x 3 uint8."""
    k = np.arange(256, dtype=np.uint8)
    pal = np.stack([k, k, np.full(256, 255, dtype=np.uint8)], axis=1)
    pal[0] = 0
    return pal


def indices(rgb_frame) -> np.ndarray:
    """H x W uint8 palette indices of an H x W x 3 frame of render_spec.render."""
    rgb = np.asarray(rgb_frame, dtype=np.uint8)
    return np.where(rgb[..., 2] == 0, 0, np.maximum(rgb[..., 0], 1)).astype(np.uint8)


def lzw_codes(idx) -> list[tuple[int, int]]:
    """(code, width in bits) of every code of the frame: clears, data codes, the end code."""
    flat = np.asarray(idx, dtype=np.uint8).reshape(-1).tolist()
    assert flat, "a frame has at least one pixel"
    out = []
    width = 9
    for at in range(0, len(flat), CHUNK):
        chunk = flat[at:at + CHUNK]
        out.append((CLEAR, width))
        width, nxt, table = 9, FIRST, {}
        prefix = chunk[0]
        for byte in chunk[1:]:
            key = (prefix << 8) | byte
            code = table.get(key)
            if code is not None:
                prefix = code
                continue
            out.append((prefix, width))
            table[key] = nxt
            if nxt == 1 << width:
                width += 1
            nxt += 1
            prefix = byte
        out.append((prefix, width))
        if nxt == 1 << width:
            width += 1
        nxt += 1
    out.append((END, width))
    return out


def pack(codes) -> bytes:
    out = bytearray()
    acc = nbits = 0
    for code, width in codes:
        acc |= code << nbits
        nbits += width
        while nbits >= 8:
            out.append(acc & 0xFF)
            acc >>= 8
            nbits -= 8
    if nbits:
        out.append(acc)
    return bytes(out)


def image_data(idx) -> bytes:
    stream = pack(lzw_codes(idx))
    out = bytearray([8])
    for at in range(0, len(stream), 255):
        block = stream[at:at + 255]
        out.append(len(block))
        out += block
    out.append(0)
    return bytes(out)


def header(width: int, height: int, loop: int = 0) -> bytes:
    return (b"GIF89a" + struct.pack("<HHBBB", width, height, 0xF7, 0, 0) + palette().tobytes()
            + b"\x21\xFF\x0BNETSCAPE2.0\x03\x01" + struct.pack("<H", loop) + b"\x00")


def frame(width: int, height: int, data: bytes, delay_cs: int = 1) -> bytes:
    return (b"\x21\xF9\x04\x00" + struct.pack("<H", delay_cs) + b"\x00\x00"
            + b"\x2C" + struct.pack("<HHHHB", 0, 0, width, height, 0) + data)


def file(list_of_idx, delay_cs: int = 1, loop: int = 0, size=None) -> bytes:
    """The whole file; `size` = (width, height) is needed only when there are no frames."""
    frames = [np.asarray(i, dtype=np.uint8) for i in list_of_idx]
    width, height = size if size is not None else (frames[0].shape[1], frames[0].shape[0])
    out = header(width, height, loop)
    for idx in frames:
        assert idx.shape == (height, width)
        out += frame(width, height, image_data(idx), delay_cs)
    return out + b"\x3B"


def _lzw_decode(stream: bytes, min_size: int, pixels: int) -> np.ndarray:
    clear, end = 1 << min_size, (1 << min_size) + 1
    total = 8 * len(stream)
    pos, width = 0, min_size + 1
    table = [bytes([k]) for k in range(clear)] + [b"", b""]
    prev = None
    out = bytearray()
    while True:
        assert pos + width <= total, "the stream ends without an end code"
        code = (int.from_bytes(stream[pos >> 3:(pos >> 3) + 3], "little") >> (pos & 7)) & ((1 << width) - 1)
        pos += width
        if code == clear:
            del table[clear + 2:]
            width, prev = min_size + 1, None
            continue
        if code == end:
            break
        if prev is None:
            entry = table[code]
        else:
            assert code <= len(table), "a code beyond the dictionary"
            entry = table[code] if code < len(table) else prev + prev[:1]
            if len(table) < 4096:
                table.append(prev + entry[:1])
                if len(table) == 1 << width and width < 12:
                    width += 1
        out += entry
        prev = entry
    pad = total - pos
    assert pad < 8 and (pad == 0 or stream[-1] >> (8 - pad) == 0), "bits after the end code"
    assert len(out) == pixels, f"{len(out)} pixels decoded, {pixels} expected"
    return np.frombuffer(bytes(out), dtype=np.uint8)


def decode(file_bytes: bytes):
    """-> (list of H x W uint8 index arrays, palette 256 x 3, delays in cs, loop count or None).  Reads the files
    `file` describes: a global palette, full-size frames that are not interlaced."""
    b = bytes(file_bytes)
    assert b[:6] == b"GIF89a"
    width, height, flags, _, _ = struct.unpack("<HHBBB", b[6:13])
    assert flags & 0x80
    n = 2 << (flags & 7)
    pal = np.frombuffer(b[13:13 + 3 * n], dtype=np.uint8).reshape(n, 3).copy()
    at = 13 + 3 * n
    frames, delays, loop = [], [], None

    def sub_blocks(at):
        data = bytearray()
        while b[at]:
            data += b[at + 1:at + 1 + b[at]]
            assert len(b) > at + b[at]
            at += 1 + b[at]
        return bytes(data), at + 1

    while b[at] != 0x3B:
        if b[at] == 0x21:
            label = b[at + 1]
            data, at = sub_blocks(at + 2)
            if label == 0xF9:
                delays.append(struct.unpack("<H", data[1:3])[0])
            elif label == 0xFF and data[:11] == b"NETSCAPE2.0":
                loop = struct.unpack("<H", data[12:14])[0]
        else:
            assert b[at] == 0x2C
            x, y, w, h, f = struct.unpack("<HHHHB", b[at + 1:at + 10])
            assert (x, y, w, h, f) == (0, 0, width, height, 0)
            min_size = b[at + 10]
            data, at = sub_blocks(at + 11)
            frames.append(_lzw_decode(data, min_size, width * height).reshape(height, width))
    assert at == len(b) - 1
    return frames, pal, delays, loop
