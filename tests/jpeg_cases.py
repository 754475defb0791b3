"""The images the JPEG encoder is tested on (tests/test_gpu_jpeg_cases.py), each built to put one edge of the bitstream
of tests/jpeg_spec.py, or of the kernels of sand_crate_amd/csrc/sc_jpeg.h that reproduce it, to the test;
tests/test_jpeg_cases_cpu.py proves on the CPU, from jpeg_spec alone, that each has the property it is named for.

`cases()` -> {name: (H x W x 3 uint8 image, quality)}.  Everything is seeded and small (the strips, 0.44 MB each, are the
largest); the searches run through jpeg_spec on the CPU and take a few seconds together.

symbols_qQ    blocks of a single AC coefficient: zig-zag position 1..63 (run (p - 1) & 15 behind (p - 1) >> 4 ZRLs), four
              magnitudes of each size 1..10, in Y (grey), Cb or Cr (the other two components held at 128), at qualities
              100, 98, 95, 90, 75 and 50: the float inverse DCT of value * Q[p], plus 128, rounded and clipped.  A
              greedy minimal subset of them (about 90 of 50,000), those of one quality in one image.  They code all 160
              (run, size) AC symbols of the luminance table and all 160 of the chrominance table -- there is no
              exception: run 11, size 10 in luminance (0xBA), which 512, 768 and 1023 miss (rounding adds a +-1 in
              front, or the block clips), is reached by 520 at position 12 at quality 100 --, one, two and three ZRLs in front of a coefficient, and blocks with and without EOB.
extreme_K     K = grey, cb, cr: the sign patterns of the (0,4), (4,0) and (4,4) basis functions in white / black, blue /
              yellow, red / cyan, both polarities, at quality 100: quantised values of +-1020 in Y, Cb, Cr, the edge of
              the "below 1024" on which the buffers of sc_jpeg.h are sized
dc11_K        flat blocks of the same two colours in turn: DC differences of +-2040, category 11, in either DC table
dc_ladder     flat blocks whose level steps by 1, 2, 4, .. 64 and 113 in Y, then Cb, then Cr: DC categories 4..10 (the
              symbols images code 0..3)
long_N_mcus   binary noise (each channel 0 or 255) at quality 100, 65 and 129 MCUs a row: the longest blocks the spec
              produces, 800 bits on average (uniform noise: 700; the bound: 1660).  The longest block found has
              LONGEST_BLOCK = 894 bits, the longest round of 64 blocks LONGEST_ROUND = 51,425 bits.
rounds_grey_M grey 128, M MCUs wide: every block is all zero, 6 bits for Y and 4 each for Cb and Cr, so a row has 14 M
              bits and k_jpeg_rows' rounds of 64 blocks end at known bits.  M = 21: 63 blocks, one round, a block
              short.  22: the second round holds two blocks and 8 bits and completes no word.  42, 43: 126 and 129
              blocks.  64: 192, three rounds exactly.  65: the third round ends at bit 896 = 28 x 32 and a fourth
              follows.  16: the row is 7 words, nothing is left for the tail.  4: 7 bytes, no padding, a partial word.
rounds_noise_W noise at quality 75 of the same widths 8 M, and 8 M - 7 (replicated columns): the DC prediction crosses
              the rounds with differences that are neither zero nor the DC value
pad_P         a row of 1 to 6 MCUs of noise at quality 100 whose last byte takes P = 0..7 padding bits
stuff_*       rows (twice each, so that a restart marker follows the first) of noise at quality 100 whose padded bytes
              number 255, 256, 257 (k_jpeg_stuff's step of 256 and its neighbours), 258 (with them, every residue mod
              4) and 512; whose last byte is 0xFF (FF 00 FF D0); with 0xFF at offsets of every residue mod 4; with 0xFF
              at offset 255, and at 256; with FF FF (bytes 3 and 4: the block {1: 127, 4: 16} behind an all-zero MCU,
              a size-7 value of all ones running into a 16-bit code); with FF FF FF (bytes 7, 8, 9: 255 at run 12, then
              a coefficient at run 15, at quality 95 behind three all-zero MCUs -- at quality 100 the rounding of the
              samples scatters +-1 coefficients that break the runs).  A run of four was not sought.
rows_H        8 pixels wide, H = 512, 513, 1024, 1025 high, noise at quality 50: 64, 65, 128 and 129 restart intervals
              for k_jpeg_scan's step of 64, RST0..7 in turn
edge_HxW      all 64 sizes (8 + i) x (8 + j), noise at quality 90: every replication residue in both directions
tail_K        sizes whose block count 3 ceil(W / 8) ceil(H / 8) is K = 0, 1, 31 mod 32: the dead threads at the end of
              k_jpeg_dct's last workgroup of 32 blocks
strip_HxW     9 x 16384 and 16384 x 9, noise at quality 75: the largest side sc_jpeg_bound accepts; 6144 blocks (96
              rounds) in a row, 2048 rows

The helpers `symbol_set`, `block_bits`, `row_bits`, `round_bits` and `row_bytes` say what an image makes the entropy coder
emit; they are written from jpeg_spec's coefficients, bit_length, tables, row_symbols and pack_bits.
"""
from __future__ import annotations

import functools

import numpy as np

import jpeg_spec as J

BLOCK_BITS_BOUND = 22 + 63 * 26  # kJpegBlockBits of sc_jpeg.h
ROUND = 64  # blocks per round of k_jpeg_rows
SYMBOL_QUALITIES = (100, 98, 95, 90, 75, 50)
LONGEST_BLOCK, LONGEST_ROUND = 894, 51425  # bits, measured on the `long` cases
AC_SYMBOLS = frozenset((run << 4) | size for run in range(16) for size in range(1, 11))  # the 160 (run, size)


# ---- what an image makes the entropy coder emit, from jpeg_spec ----------------------------------

def _coded(img, quality: int):
    """Per MCU row and block in coding order: the zig-zag coefficients (rows x blocks x 64), each block's Huffman table
    (blocks), its DC difference, and for every AC coefficient its zero run (-1 where the coefficient is zero)."""
    zz = J.coefficients(img, quality)
    rows, mcus = zz.shape[:2]
    zz = zz.reshape(rows, 3 * mcus, 64)
    tab = np.tile([0, 1, 1], mcus)
    dc = zz[..., 0]
    diff = dc.copy()
    diff[:, 3:] -= dc[:, :-3]
    pos = np.arange(64)
    nz = zz != 0
    nz[..., 0] = True  # the run counts from the DC coefficient
    last = np.maximum.accumulate(np.where(nz, pos, 0), axis=-1)
    run = np.full(zz.shape, -1, dtype=np.int64)
    run[..., 1:] = np.where(nz[..., 1:], pos[1:] - last[..., :-1] - 1, -1)
    return zz, tab, diff, run


def symbol_set(img, quality: int) -> set:
    """The (table, kind, symbol) an image codes: ("dc", category), ("ac", (run & 15) << 4 | size), ("zrl", how many ZRL
    codes stand in front of one coefficient, 1..3) and ("eob", whether the block ends in an EOB code)."""
    zz, tab, diff, run = _coded(img, quality)
    out = set()
    for t in (0, 1):
        sel = tab == t
        out |= {(t, "dc", int(c)) for c in np.unique(J.bit_length(diff[:, sel]))}
        z, r = zz[:, sel], run[:, sel]
        at = r >= 0
        out |= {(t, "ac", int(s)) for s in np.unique(((r[at] & 15) << 4) | J.bit_length(z[at]))}
        out |= {(t, "zrl", int(n)) for n in np.unique(r[at] >> 4) if n > 0}
        out |= {(t, "eob", bool(e)) for e in np.unique(z[..., 63] == 0)}
    return out


def block_bits(img, quality: int) -> np.ndarray:
    """The bits of every block (its DC code, AC codes, ZRLs and EOB): rows x blocks."""
    zz, tab, diff, run = _coded(img, quality)
    cat = J.bit_length(diff)
    dc_len = np.stack([J.DC_TABLES[t][1] for t in (0, 1)])
    ac_len = np.stack([J.AC_TABLES[t][1] for t in (0, 1)])
    bits = dc_len[tab[None, :], cat] + cat
    size = J.bit_length(zz)
    t3 = np.broadcast_to(tab[None, :, None], zz.shape)
    at = run >= 0
    ac = np.zeros(zz.shape, dtype=np.int64)
    ac[at] = ac_len[t3[at], ((run[at] & 15) << 4) | size[at]] + size[at] + (run[at] >> 4) * ac_len[t3[at], 0xF0]
    bits = bits + ac.sum(axis=-1)
    return bits + np.where(zz[..., 63] == 0, ac_len[tab, 0x00][None, :], 0)


def row_bits(img, quality: int) -> np.ndarray:
    """The bits of every MCU row before padding."""
    return block_bits(img, quality).sum(axis=1)


def round_bits(img, quality: int) -> np.ndarray:
    """The running bit count of every row after each 64 blocks, and at its end: rows x ceil(blocks / 64)."""
    total = np.cumsum(block_bits(img, quality), axis=1)
    ends = np.r_[np.arange(ROUND, total.shape[1], ROUND), total.shape[1]] - 1
    return total[:, ends]


def row_bytes(img, quality: int) -> list:
    """The padded bytes of every MCU row, before stuffing (uint8 arrays)."""
    return J.entropy_rows(J.coefficients(img, quality))


def max_ac(img, quality: int) -> int:
    """The largest magnitude among the quantised AC coefficients."""
    return int(np.abs(J.coefficients(img, quality)[..., 1:]).max())


# ---- building blocks ------------------------------------------------------------------------------

_u = np.arange(8)[:, None]
_x = np.arange(8)[None, :]
_M = 0.5 * np.where(_u == 0, 1 / np.sqrt(2), 1.0) * np.cos((2 * _x + 1) * _u * np.pi / 16)


def idct(C) -> np.ndarray:
    """The float inverse DCT of coefficient blocks C (... x 8 x 8, natural order)."""
    return np.einsum("vy,...vu,ux->...yx", _M, np.asarray(C, dtype=np.float64), _M)


def component_rgb(comp: int, samples) -> np.ndarray:
    """... x 8 x 8 x 3 uint8 RGB whose component `comp` (0 Y, 1 Cb, 2 Cr) has the given samples (0..255) while the other
    two are 128.  Grey for Y; the JFIF inverse, rounded and clipped, for Cb and Cr."""
    s = np.asarray(samples, dtype=np.float64)
    ycc = [np.full(s.shape, 128.0) for _ in range(3)]
    ycc[comp] = s
    y, cb, cr = ycc
    rgb = np.stack([y + 1.402 * (cr - 128), y - 0.344136 * (cb - 128) - 0.714136 * (cr - 128), y + 1.772 * (cb - 128)],
                   axis=-1)
    return np.clip(np.rint(rgb), 0, 255).astype(np.uint8)


def coefficient_blocks(comp, pos, value, quality: int) -> np.ndarray:
    """N blocks (N x 8 x 8 x 3) of component comp[i] whose zig-zag coefficient pos[i] would quantise to value[i] at
    `quality`, were it not for rounding and clipping: the inverse DCT of value * Q[pos], plus 128."""
    comp, pos, value = np.asarray(comp), np.asarray(pos), np.asarray(value)
    Q = J.quant_tables(quality).reshape(2, 64)
    nat = J.ZIGZAG[pos]
    C = np.zeros((len(pos), 64))
    C[np.arange(len(pos)), nat] = value * Q[np.minimum(comp, 1), nat]
    s = np.clip(np.rint(idct(C.reshape(-1, 8, 8)) + 128), 0, 255)
    out = np.empty((len(pos), 8, 8, 3), dtype=np.uint8)
    for c in range(3):
        out[comp == c] = component_rgb(c, s[comp == c])
    return out


def grey_block(coefs: dict, quality: int = 100) -> np.ndarray:
    """An 8 x 8 x 3 grey block with the zig-zag coefficients {position: quantised value}."""
    Q = J.quant_tables(quality).reshape(2, 64)[0]
    C = np.zeros(64)
    for p, v in coefs.items():
        C[J.ZIGZAG[p]] = v * Q[J.ZIGZAG[p]]
    s = np.clip(np.rint(idct(C.reshape(8, 8)) + 128), 0, 255).astype(np.uint8)
    return np.repeat(s[:, :, None], 3, axis=2)


def strip(blocks) -> np.ndarray:
    """8 x 8N x 3: the blocks (N x 8 x 8 x 3) side by side, one MCU each."""
    return np.concatenate(list(blocks), axis=1)


def noise(seed: int, h: int, w: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def grey(h: int, w: int, value: int = 128) -> np.ndarray:
    return np.full((h, w, 3), value, dtype=np.uint8)


# ---- symbols --------------------------------------------------------------------------------------

def _block_cover(img, quality: int) -> np.ndarray:
    """For a strip of N MCUs: N x 522 bools, the AC symbols (table * 256 + symbol), ZRL counts (512 + table * 3 + n - 1)
    and EOB states (518 + table * 2 + present) that each MCU codes."""
    zz, tab, _, run = _coded(img, quality)
    zz, run = zz[0], run[0]
    n = zz.shape[0] // 3
    cover = np.zeros((n, 522), dtype=bool)
    blk, pos = np.nonzero(run >= 0)
    r, t = run[blk, pos], tab[blk]
    cover[blk // 3, t * 256 + (((r & 15) << 4) | J.bit_length(zz[blk, pos]))] = True
    z = r >> 4 > 0
    cover[blk[z] // 3, 512 + t[z] * 3 + (r[z] >> 4) - 1] = True
    cover[np.arange(3 * n) // 3, 518 + tab * 2 + (zz[:, 63] == 0)] = True
    return cover


def symbol_images() -> dict:
    """{quality: image}: a greedy minimal subset of the single-coefficient blocks, those of one quality side by side in
    MCU rows of 8."""
    meta, cover = [], []
    for q in SYMBOL_QUALITIES:
        comp, pos, size = (a.ravel() for a in np.meshgrid(np.arange(3), np.arange(1, 64), np.arange(1, 11), indexing="ij"))
        # four magnitudes of each size: the smallest, one just above it, the middle, the largest; the sign
        # alternates
        low = 1 << (size - 1)
        mags = np.stack([low, low + (low >> 6), np.maximum(3 * low >> 1, 1), (1 << size) - 1])
        sign = np.where((pos + size) & 1, -1, 1)
        value = (mags * sign).ravel()
        comp, pos = np.tile(comp, 4), np.tile(pos, 4)
        top = np.abs(value) >= 512  # size 10 sits at the edge of clipping: both signs
        comp, pos, value = np.r_[comp, comp[top]], np.r_[pos, pos[top]], np.r_[value, -value[top]]
        blocks = coefficient_blocks(comp, pos, value, q)
        cover.append(_block_cover(strip(blocks), q))
        meta += [(q, b) for b in blocks]
    cover = np.concatenate(cover)
    left = cover.any(axis=0)
    chosen = []
    while left.any():
        gain = cover[:, left].sum(axis=1)
        best = int(gain.argmax())
        chosen.append(best)
        left &= ~cover[best]
    out = {}
    for q in SYMBOL_QUALITIES:
        blocks = [meta[i][1] for i in sorted(chosen) if meta[i][0] == q]
        if not blocks:
            continue
        blocks += [grey(8, 8)] * (-len(blocks) % 8)
        out[q] = np.concatenate([strip(blocks[k:k + 8]) for k in range(0, len(blocks), 8)], axis=0)
    return out


# ---- extremes -------------------------------------------------------------------------------------

EXTREME_BASES = ((0, 4), (4, 0), (4, 4))  # (v, u): their sign patterns quantise to +-1020 at quality 100
EXTREME_COLOURS = {"grey": ((255, 255, 255), (0, 0, 0)), "cb": ((0, 0, 255), (255, 255, 0)),
                   "cr": ((255, 0, 0), (0, 255, 255))}  # (high, low) of Y, Cb, Cr


def sign_pattern(v: int, u: int) -> np.ndarray:
    """8 x 8 bools: where the (v, u) basis function is positive."""
    return np.outer(_M[v], _M[u]) > 0


def extreme_image(kind: str) -> np.ndarray:
    """8 x 48: the sign patterns of the three bases in the two colours of `kind`, then the same inverted."""
    high, low = (np.array(c, dtype=np.uint8) for c in EXTREME_COLOURS[kind])
    blocks = [np.where((sign_pattern(v, u) ^ flip)[:, :, None], high, low) for flip in (False, True)
              for v, u in EXTREME_BASES]
    return strip(blocks)


def dc11_image(kind: str) -> np.ndarray:
    """16 x 64: flat blocks of the two colours of `kind` in turn, the largest DC steps (category 11)."""
    high, low = (np.array(c, dtype=np.uint8) for c in EXTREME_COLOURS[kind])
    row = strip([np.broadcast_to(high if k & 1 else low, (8, 8, 3)) for k in range(8)])
    return np.concatenate([row, row[:, ::-1]], axis=0)


DC_LADDER = (128, 129, 127, 131, 123, 139, 107, 171, 58)  # steps of 1, 2, 4, .. 64 and 113: x 8, categories 4..10


def dc_ladder_image() -> np.ndarray:
    """8 x 216: flat blocks whose Y, then Cb, then Cr steps through DC_LADDER (quality 100: DC = 8 (level - 128))."""
    levels = np.broadcast_to(np.array(DC_LADDER, dtype=np.float64)[:, None, None], (len(DC_LADDER), 8, 8))
    return strip(np.concatenate([component_rgb(c, levels) for c in range(3)]))


# ---- searches over noise strips --------------------------------------------------------------------

class Pool:
    """`count` noise strips of `mcus` MCUs (one image, a strip per MCU row; rows are coded independently)."""

    def __init__(self, seed: int, mcus: int, count: int, quality: int = 100):
        self.img = noise(seed, 8 * count, 8 * mcus)
        self.zz = J.coefficients(self.img, quality)
        self.bits = row_bits(self.img, quality)
        self.nbytes = (self.bits + 7) >> 3

    def strip(self, r: int) -> np.ndarray:
        return self.img[8 * r:8 * r + 8]

    def bytes(self, r: int) -> np.ndarray:
        return J.pack_bits(*J.row_symbols(self.zz[r]))

    def first(self, ok):
        """The first strip whose padded bytes satisfy ok(bytes)."""
        for r in range(len(self.bits)):
            if ok(self.bytes(r)):
                return self.strip(r)
        raise AssertionError("no strip found")


def twice(strip_) -> np.ndarray:
    """The strip as two MCU rows, so that a restart marker follows the first."""
    return np.concatenate([strip_, strip_], axis=0)


def pad_cases() -> dict:
    """{pad: strip}: rows of 1 to 6 MCUs of noise whose last byte has `pad` padding bits, at quality 100."""
    out = {}
    for mcus in (1, 2, 3, 4, 5, 6, 1, 2):  # the pad wanted from strips of each width in turn
        pool = Pool(500 + len(out), mcus, 64)
        out[len(out)] = pool.strip(int(np.nonzero(-pool.bits % 8 == len(out))[0][0]))
    return out


FF_FF_BLOCK = {1: 127, 4: 16}  # behind 16 bits: f8, then seven 1-bits and the nine that begin a 16-bit code, then 13
# 255 at run 12 and a coefficient at run 15: a code that ends in 1-bits, eight 1-bits, a code that begins with eleven.
# At quality 100 the rounding of the samples adds stray +-1 coefficients that break the runs; quality 95 (Q >= 2
# nearly everywhere) keeps the block clean.
FF_FF_FF_BLOCKS = ({13: 255, 29: 3}, {13: 255, 29: 1}, {13: 255, 30: 1})
FF_FF_FF_QUALITY = 95


def ff_run_image(blocks, n: int, quality: int) -> np.ndarray:
    """A row that holds n 0xFF bytes in a row: one of the grey blocks behind 0 to 3 grey-128 MCUs (14 bits each, so
    the block starts at an even bit), whichever comes first."""
    for coefs in blocks:
        for lead in range(4):
            img = strip([grey(8, 8)] * lead + [grey_block(coefs, quality)])
            if bytes([0xFF] * n) in row_bytes(img, quality)[0].tobytes():
                return img
    raise AssertionError(f"no run of {n} 0xFF bytes")


def stuffing_cases() -> dict:
    out = {}
    one = Pool(600, 1, 400)  # about 262 bytes a row
    two = Pool(601, 2, 400)  # about 525
    for n in (255, 256, 257, 258):
        out[f"stuff_len_{n}"] = twice(one.strip(int(np.nonzero(one.nbytes == n)[0][0])))
    out["stuff_len_512"] = twice(two.strip(int(np.nonzero(two.nbytes == 512)[0][0])))
    out["stuff_last_ff"] = twice(one.first(lambda b: b[-1] == 0xFF))
    out["stuff_ff_at_every_mod_4"] = twice(two.first(lambda b: len(set((np.nonzero(b == 0xFF)[0] & 3).tolist())) == 4))
    for at in (255, 256):
        out[f"stuff_ff_at_{at}"] = twice(two.first(lambda b: b[at] == 0xFF))
    out["stuff_ff_ff"] = twice(ff_run_image((FF_FF_BLOCK,), 2, 100))
    out["stuff_ff_ff_ff"] = twice(ff_run_image(FF_FF_FF_BLOCKS, 3, FF_FF_FF_QUALITY))
    return out


# ---- long, rounds, rows, edges, strips --------------------------------------------------------------

def binary_noise(seed: int, h: int, w: int) -> np.ndarray:
    """Each channel 0 or 255."""
    return (np.random.RandomState(seed).randint(0, 2, (h, w, 3)) * 255).astype(np.uint8)


ROUND_MCUS = (4, 16, 21, 22, 42, 43, 64, 65)
ROW_HEIGHTS = (512, 513, 1024, 1025)
EDGE_SIZES = tuple((8 + i, 8 + j) for i in range(8) for j in range(8))  # (H, W)
TAIL_SIZES = {0: (59, 28), 1: (5, 83), 31: (20, 51)}  # blocks mod 32 -> (H, W): 96, 33 and 63 blocks
STRIP_SIZES = ((9, 16384), (16384, 9))  # (H, W)


@functools.lru_cache(maxsize=None)
def round_noise(w: int) -> np.ndarray:
    """9 x w noise in which the blocks that open a round of the first row (64, 65, 66, 128, ..) have a DC difference that
    is neither zero nor the DC value itself at quality 75: the predictor, which lies in the round before, counts."""
    for seed in range(800, 864):
        img = noise(seed + w, 9, w)
        zz, _, diff, _ = _coded(img, 75)
        opening = [k for first in range(ROUND, zz.shape[1], ROUND) for k in range(first, min(first + 3, zz.shape[1]))]
        if (diff[0, opening] != 0).all() and (diff[0, opening] != zz[0, opening, 0]).all():
            return img
    raise AssertionError("no such noise")


def grey_row_bits(mcus: int) -> int:
    """The bits of a row of all-zero MCUs: 6 for Y (a 2-bit DC code, a 4-bit EOB), 4 each for Cb and Cr."""
    return 14 * mcus


def blocks_of(h: int, w: int) -> int:
    return 3 * -(-w // 8) * -(-h // 8)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for q, img in symbol_images().items():
        out[f"symbols_q{q}"] = (img, q)
    for kind in EXTREME_COLOURS:
        out[f"extreme_{kind}"] = (extreme_image(kind), 100)
        out[f"dc11_{kind}"] = (dc11_image(kind), 100)
    out["dc_ladder"] = (dc_ladder_image(), 100)
    out["long_65_mcus"] = (binary_noise(700, 24, 520), 100)
    out["long_129_mcus"] = (binary_noise(701, 8, 1025), 100)
    for m in ROUND_MCUS:
        out[f"rounds_grey_{m}"] = (grey(16, 8 * m), 75)
        out[f"rounds_noise_{8 * m}"] = (round_noise(8 * m), 75)
        out[f"rounds_noise_{8 * m - 7}"] = (round_noise(8 * m - 7), 75)
    for pad, img in pad_cases().items():
        out[f"pad_{pad}"] = (img, 100)
    for name, img in stuffing_cases().items():
        out[name] = (img, FF_FF_FF_QUALITY if name == "stuff_ff_ff_ff" else 100)
    for h in ROW_HEIGHTS:
        out[f"rows_{h}"] = (noise(1000 + h, h, 8), 50)
    for h, w in EDGE_SIZES:
        out[f"edge_{h}x{w}"] = (noise(1100 + 8 * h + w, h, w), 90)
    for k, (h, w) in TAIL_SIZES.items():
        out[f"tail_{k}"] = (noise(1200 + k, h, w), 90)
    for h, w in STRIP_SIZES:
        out[f"strip_{h}x{w}"] = (noise(1300 + (h > w), h, w), 75)
    out = {name: (np.ascontiguousarray(img), q) for name, (img, q) in out.items()}
    for img, _ in out.values():
        img.setflags(write=False)
    return out
