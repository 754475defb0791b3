"""The index images the GIF encoder is tested on (tests/test_gpu_gif.py), each built to put one property of the bitstream
of tests/gif_spec.py to the test; tests/test_gif_cpu.py proves on the CPU that each has the property it is named for.

`cases()` -> {name: H x W uint8}.  Everything is seeded; the searches are small (a few hundred chunks of 1024 pixels).

sizes    frames of 1, 1023, 1024, 1025 and 2049 pixels (one pixel, one short chunk, one full chunk, a full chunk and a
         pixel, two and a pixel) and 31 x 33, of noise
flat     one value: the longest matches, the fewest codes
noise    uniform over 0..255: codes of 9, 10 and 11 bits
mixed    flat, ramp and noise chunks in turn: clear codes of 9, 10 and 11 bits
last_K   a frame whose last chunk emits exactly K data codes; K = 255 and 767 raise the width just before the end code,
         254 / 256 and 766 / 768 are the neighbours that do not, or did already
full_K   the same counts in a full chunk of 1024 pixels (a run of one value, then noise) that a short chunk follows, so
         that it is the next clear code that moves to the new width
packed_L the packed stream is exactly L bytes long: 254, 255, 256 and 510, the edges of the sub-blocks of 255
"""
from __future__ import annotations

import functools

import numpy as np

CHUNK = 1024
BUMP_COUNTS = (254, 255, 256, 766, 767, 768)
PACKED_LENGTHS = (254, 255, 256, 510)
SIZES = ((1, 1), (1, 1023), (1, 1024), (1, 1025), (3, 683), (31, 33))


def chunk_counts(pixels) -> list[int]:
    """How many data codes a chunk emits after each of its pixels (entry n - 1: the chunk cut after n pixels)."""
    pixels = [int(p) for p in pixels]
    assert 1 <= len(pixels) <= CHUNK
    table, out = {}, []
    prefix, emitted, nxt = pixels[0], 0, 258
    out.append(1)
    for byte in pixels[1:]:
        key = (prefix << 8) | byte
        code = table.get(key)
        if code is None:
            table[key] = nxt
            nxt += 1
            emitted += 1
            prefix = byte
        else:
            prefix = code
        out.append(emitted + 1)  # the pending prefix goes out at the end
    return out


def noise(seed: int, n: int) -> np.ndarray:
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8)


def last_chunk_with(count: int) -> np.ndarray:
    """1 x n noise (one chunk) that emits exactly `count` data codes."""
    counts = chunk_counts(noise(100, CHUNK))
    n = counts.index(count) + 1  # the count grows by 0 or 1 per pixel: every value up to the last is met
    return noise(100, CHUNK)[:n].reshape(1, n)


def full_chunk_with(count: int) -> np.ndarray:
    """1024 pixels, a run of one value and then noise, that emit exactly `count` data codes."""
    for seed in range(200, 264):
        tail = noise(seed, CHUNK)
        for run in range(max(CHUNK - count - 10, 0), min(CHUNK - count + 60, CHUNK)):
            chunk = np.concatenate([np.full(run, 77, dtype=np.uint8), tail[:CHUNK - run]])
            if chunk_counts(chunk)[-1] == count:
                return chunk
    raise AssertionError(f"no run + noise chunk with {count} codes")


def packed_length(idx) -> int:
    import gif_spec as G
    return len(G.pack(G.lzw_codes(idx)))


def frames_with_packed_lengths(lengths) -> dict:
    """{L: 1 x n noise whose packed stream has exactly L bytes}; the noise length is searched, seed after seed."""
    found = {}
    for seed in range(300, 364):
        row = noise(seed, 700)
        for n in range(150, 700):
            size = packed_length(row[:n])
            if size in lengths and size not in found:
                found[size] = row[:n].reshape(1, n).copy()
            if size > max(lengths):
                break
        if len(found) == len(lengths):
            return found
    raise AssertionError(f"packed lengths found: {sorted(found)} of {sorted(lengths)}")


def mixed_chunks() -> np.ndarray:
    """Flat, ramp, noise, flat, ramp, noise and a short tail: 6 x 1024 + 100 pixels as 1 x n."""
    flat = np.full(CHUNK, 200, dtype=np.uint8)
    ramp = (np.arange(CHUNK) % 256).astype(np.uint8)
    parts = [flat, ramp, noise(400, CHUNK), flat, ramp, noise(401, CHUNK), noise(402, 100)]
    return np.concatenate(parts).reshape(1, -1)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for k, (h, w) in enumerate(SIZES):
        out[f"size_{h}x{w}"] = noise(10 + k, h * w).reshape(h, w)
    out["flat_3x683"] = np.full((3, 683), 131, dtype=np.uint8)
    out["flat_zero_1x1024"] = np.zeros((1, 1024), dtype=np.uint8)
    out["noise_40x64"] = noise(20, 40 * 64).reshape(40, 64)
    out["mixed"] = mixed_chunks()
    for count in BUMP_COUNTS:
        out[f"last_{count}"] = last_chunk_with(count)
        out[f"full_{count}"] = np.concatenate([full_chunk_with(count), noise(30, 7)]).reshape(1, CHUNK + 7)
    for size, idx in frames_with_packed_lengths(PACKED_LENGTHS).items():
        out[f"packed_{size}"] = idx
    for idx in out.values():
        idx.setflags(write=False)
    return out
