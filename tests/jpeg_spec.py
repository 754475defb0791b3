"""The bitstream of `sc_jpeg_encode_device` (sand_crate_amd/csrc/sc_jpeg.h), written once in NumPy.

The device output equals `encode(rgb, quality)` byte for byte.  The rule:

container  baseline sequential JPEG (SOF0), 8-bit, JFIF APP0; three components Y, Cb, Cr (ids 1, 2, 3), all 4:4:4
           (H = V = 1); Y uses quantisation / Huffman tables 0, Cb and Cr tables 1.  Markers: SOI, APP0, DQT (both
           tables in one segment), SOF0, DHT (DC0, AC0, DC1, AC1 in one segment), DRI, SOS, entropy-coded data, EOI.
padding    a width or height that is not a multiple of 8 replicates the last column / row.
colour     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
           Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
           Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16     (floor shifts), then each minus 128.
DCT        A[u][x] = round(4096 / 2 c(u) cos((2x + 1) u pi / 16)), c(0) = 1/sqrt(2), c(u > 0) = 1.  Per block s[y][x]:
           rows T[y][u] = sum_x A[u][x] s[y][x], T1 = (T + 256) >> 9; columns U[v][u] = sum_y A[v][y] T1[y][u]
           (the DCT scaled by 2^15; int32 holds every value).
quantise   q = sign(U) ((|U| + Q 2^14) // (Q 2^15)); Q from the Annex K.1 tables scaled by the IJG quality rule
           (s = 5000 / quality below 50, else 200 - 2 quality; Q = clip((base s + 50) // 100, 1, 255)), quality 1..100.
entropy    the Annex K.3 Huffman tables; coefficients in zig-zag order with ZRL (16 zeros) and EOB.
restarts   DRI = one MCU row (ceil(W / 8) MCUs); the DC predictors restart at 0 on every row.  Each row's bits are
           padded to a byte with 1-bits, 0xFF data bytes get a 0x00 after them, and RST0..RST7 (in turn) follow every
           row but the last.

The product never imports this module.
"""
from __future__ import annotations

import struct

import numpy as np

# Annex K.1
LUMA_Q = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64).reshape(8, 8)
CHROMA_Q = np.full((8, 8), 99, dtype=np.int64)
CHROMA_Q[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# Annex K.3: (BITS, HUFFVAL) of DC luminance, AC luminance, DC chrominance, AC chrominance
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6"
    "a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))

# ZIGZAG[k] = the natural (row-major) index of the k-th coefficient in zig-zag order
ZIGZAG = np.array([
    0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
    47, 55, 62, 63], dtype=np.int64)


def dct_matrix() -> np.ndarray:
    u = np.arange(8)[:, None]
    x = np.arange(8)[None, :]
    c = np.where(u == 0, 1 / np.sqrt(2), 1.0)
    return np.round(4096 * 0.5 * c * np.cos((2 * x + 1) * u * np.pi / 16)).astype(np.int64)


A = dct_matrix()


def quant_tables(quality: int) -> np.ndarray:
    """2 x 8 x 8 (luminance, chrominance), natural order."""
    if not 1 <= quality <= 100:
        raise ValueError("quality must be 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.stack([np.clip((base * s + 50) // 100, 1, 255) for base in (LUMA_Q, CHROMA_Q)])


def huffman_codes(bits, vals) -> dict:
    """symbol -> (code, length), Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _table(bits, vals, size):
    codes = huffman_codes(bits, vals)
    code = np.zeros(size, dtype=np.int64)
    length = np.zeros(size, dtype=np.int64)
    for sym, (c, n) in codes.items():
        code[sym], length[sym] = c, n
    return code, length


DC_TABLES = [_table(DC_BITS[t], DC_VALS[t], 12) for t in range(2)]
AC_TABLES = [_table(AC_BITS[t], AC_VALS[t], 256) for t in range(2)]


def ycc(rgb) -> np.ndarray:
    """H x W x 3 uint8 RGB -> 3 x H' x W' int64 level-shifted Y, Cb, Cr, padded to multiples of 8 by edge replication."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError("rgb must be an H x W x 3 uint8 array")
    h, w = rgb.shape[:2]
    p = np.pad(rgb, ((0, -h % 8), (0, -w % 8), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr]) - 128


def blocks(rgb) -> np.ndarray:
    """The 8 x 8 sample blocks in coding order (MCU rows, MCUs, Y Cb Cr): rows x mcus x 3 x 8 x 8 int64."""
    c = ycc(rgb)
    _, H, W = c.shape
    return c.reshape(3, H // 8, 8, W // 8, 8).transpose(1, 3, 0, 2, 4)


def dct(s) -> np.ndarray:
    """The integer DCT of blocks s (... x 8 x 8): U, the DCT scaled by 2^15."""
    T = np.einsum("ux,...yx->...yu", A, s)
    T1 = (T + 256) >> 9
    return np.einsum("vy,...yu->...vu", A, T1)


def float_dct(s) -> np.ndarray:
    """The exact DCT-II of blocks s (unscaled)."""
    u = np.arange(8)[:, None]
    x = np.arange(8)[None, :]
    M = 0.5 * np.where(u == 0, 1 / np.sqrt(2), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.einsum("vy,...yx,ux->...vu", M, np.asarray(s, dtype=np.float64), M)


def quantise(U, quality: int) -> np.ndarray:
    """q of blocks U (rows x mcus x 3 x 8 x 8), natural order."""
    Q = quant_tables(quality)[[0, 1, 1]][None, None]  # per component
    a = np.abs(U)
    return np.sign(U) * ((a + Q * (1 << 14)) // (Q * (1 << 15)))


def coefficients(rgb, quality: int) -> np.ndarray:
    """The quantised coefficients in coding order and zig-zag order: rows x mcus x 3 x 64 int64."""
    q = quantise(dct(blocks(rgb)), quality)
    return q.reshape(q.shape[:3] + (64,))[..., ZIGZAG]


def bit_length(v) -> np.ndarray:
    """The magnitude category of v: bits of |v| (0 for 0)."""
    a = np.abs(np.asarray(v, dtype=np.int64))
    n = np.zeros(a.shape, dtype=np.int64)
    while (a >> n).any():
        n += (a >> n) > 0
    return n


def _extra(v, size):
    """The `size` extra bits of value v: v if positive, v - 1 (low bits) if negative."""
    return np.where(v < 0, v - 1, v) & ((np.int64(1) << size) - 1)


def row_symbols(zz) -> tuple:
    """The codes of one MCU row (mcus x 3 x 64 zig-zag coefficients) in order: (value, length) int64 arrays, each
    value the Huffman code followed by its extra bits."""
    m = zz.shape[0]
    zz = zz.reshape(m * 3, 64)
    nb = m * 3
    comp = np.tile([0, 1, 1], m)  # table of each block
    dc = zz[:, 0]
    pred = np.concatenate([np.zeros(3, dtype=np.int64), dc[:-3]])[:nb]
    diff = dc - pred
    cat = bit_length(diff)
    dcode = np.where(comp == 0, DC_TABLES[0][0][cat], DC_TABLES[1][0][cat])
    dlen = np.where(comp == 0, DC_TABLES[0][1][cat], DC_TABLES[1][1][cat])
    keys = [np.arange(nb) * 256]
    vals = [(dcode << cat) | _extra(diff, cat)]
    lens = [dlen + cat]
    blk, pos = np.nonzero(zz[:, 1:])
    pos = pos + 1
    if len(blk):
        first = np.r_[True, blk[1:] != blk[:-1]]
        prev = np.where(first, 0, np.r_[0, pos[:-1]])
        run = pos - prev - 1
        q = zz[blk, pos]
        size = bit_length(q)
        sym = ((run & 15) << 4) | size
        c = comp[blk]
        acode = np.where(c == 0, AC_TABLES[0][0][sym], AC_TABLES[1][0][sym])
        alen = np.where(c == 0, AC_TABLES[0][1][sym], AC_TABLES[1][1][sym])
        keys.append(blk * 256 + 2 * pos + 1)
        vals.append((acode << size) | _extra(q, size))
        lens.append(alen + size)
        nz = run >> 4  # ZRLs in front of each coefficient
        if nz.any():
            zb = np.repeat(np.arange(len(blk)), nz)
            zc = comp[blk[zb]]
            keys.append(blk[zb] * 256 + 2 * pos[zb])
            vals.append(np.where(zc == 0, AC_TABLES[0][0][0xF0], AC_TABLES[1][0][0xF0]))
            lens.append(np.where(zc == 0, AC_TABLES[0][1][0xF0], AC_TABLES[1][1][0xF0]))
    last = np.zeros(nb, dtype=np.int64)
    if len(blk):
        np.maximum.at(last, blk, pos)
    eob = np.nonzero(last < 63)[0]
    keys.append(eob * 256 + 255)
    vals.append(np.where(comp[eob] == 0, AC_TABLES[0][0][0], AC_TABLES[1][0][0]))
    lens.append(np.where(comp[eob] == 0, AC_TABLES[0][1][0], AC_TABLES[1][1][0]))
    order = np.argsort(np.concatenate(keys), kind="stable")
    return np.concatenate(vals)[order], np.concatenate(lens)[order]


def pack_bits(vals, lens) -> np.ndarray:
    """MSB-first bit packing, the last byte padded with 1-bits: uint8 bytes (unstuffed)."""
    total = int(lens.sum())
    start = np.cumsum(lens) - lens
    idx = np.repeat(np.arange(len(lens)), lens)
    k = np.arange(total) - np.repeat(start, lens)  # bit of its code, from the first
    bits = np.ones(total + (-total % 8), dtype=np.uint8)
    bits[:total] = (vals[idx] >> (lens[idx] - 1 - k)) & 1
    return np.packbits(bits)


def stuff(data) -> bytes:
    """A 0x00 after every 0xFF."""
    data = np.asarray(data, dtype=np.uint8)
    ff = data == 0xFF
    out = np.zeros(len(data) + int(ff.sum()), dtype=np.uint8)
    pos = np.arange(len(data)) + np.cumsum(ff) - ff
    out[pos] = data
    return out.tobytes()


def entropy_rows(zz) -> list:
    """The padded, unstuffed bytes of every MCU row (restart interval)."""
    return [pack_bits(*row_symbols(row)) for row in zz]


def _segment(marker: int, body: bytes) -> bytes:
    return struct.pack(">HH", marker, len(body) + 2) + body


def header(width: int, height: int, quality: int) -> bytes:
    """SOI through SOS."""
    Q = quant_tables(quality).reshape(2, 64)[:, ZIGZAG]
    out = b"\xff\xd8"
    out += _segment(0xFFE0, b"JFIF\x00\x01\x01\x00" + struct.pack(">HHBB", 1, 1, 0, 0))
    out += _segment(0xFFDB, b"".join(bytes([t]) + bytes(Q[t].astype(np.uint8)) for t in range(2)))
    out += _segment(0xFFC0, struct.pack(">BHHB", 8, height, width, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    dht = b""
    for t in range(2):
        dht += bytes([0x00 | t]) + bytes(DC_BITS[t]) + bytes(DC_VALS[t])
        dht += bytes([0x10 | t]) + bytes(AC_BITS[t]) + bytes(AC_VALS[t])
    out += _segment(0xFFC4, dht)
    out += _segment(0xFFDD, struct.pack(">H", (width + 7) // 8))
    out += _segment(0xFFDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def encode(rgb, quality: int = 95) -> bytes:
    """The JPEG file of an H x W x 3 uint8 RGB image."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError("each side must be 1..65535")
    zz = coefficients(rgb, quality)
    rows = entropy_rows(zz)
    parts = [header(w, h, quality)]
    for r, data in enumerate(rows):
        parts.append(stuff(data))
        if r + 1 < len(rows):
            parts.append(bytes([0xFF, 0xD0 + (r & 7)]))
    parts.append(b"\xff\xd9")
    return b"".join(parts)
