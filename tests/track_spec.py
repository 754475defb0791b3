"""The packed frame of the tracker (format 1) in NumPy: the rule the device reproduces byte for byte (sc_track_capture,
the log of sc_track_enable) and the player reads back (sc_track_load).  NumPy only.

All values little-endian.  A frame:
  header, 64 bytes    b"SCTK", u32 version = 1, i64 tick, i64 n, i32 n_segments, i32 flags (bit 0: the pressure was
                      valid), f64 lo = -0.25, f64 span = 1.5, zeros
  n_segments x 4 f64  the walls of that tick
  four planes, each zero-padded to a multiple of 8 bytes:  u32 id[n], u16 qx[n], u16 qy[n], u8 c[n]

A coordinate: q = floor((x - lo) * (65534 / span) + 0.5) clamped to 0..65534 -- float64, each operation rounded on its
own -- and 65535 when x is not finite; back: lo + q * (span / 65534), +inf for 65535.  The colour byte is the
renderer's (render_spec.colour): 255 - trunc(P * 255) clipped, NaN and +inf 0, -inf 255, and 255 for a slot without a
valid pressure; back: P = (255 - c + 0.5) / 255.  Records may stand in any order (ids are unique, the draw order is by
id): `canonical` orders them by id."""
import struct

import numpy as np

MAGIC = b"SCTK"
VERSION = 1
HEADER = 64
LO, SPAN = -0.25, 1.5
CODES = 65534                       # codes 0..CODES span [LO, LO + SPAN]
NOT_FINITE = 65535
STEP = SPAN / CODES
HALF_STEP = STEP / 2                # 1.14444e-5: the error of a coordinate inside the range, up to rounding
ROUNDING = 2.0 ** -50               # ... which is a few ulps of 1.25 (the subtraction, the product, the sum; lo + q * step)
_HEADER = struct.Struct("<4sIqqiidd")


def pad8(b: int) -> int:
    return (int(b) + 7) & ~7


def planes(n: int, n_segments: int):
    """-> byte offsets of (id, qx, qy, c, end of the frame)."""
    o_id = HEADER + 32 * int(n_segments)
    o_qx = o_id + pad8(4 * n)
    o_qy = o_qx + pad8(2 * n)
    o_c = o_qy + pad8(2 * n)
    return o_id, o_qx, o_qy, o_c, o_c + pad8(n)


def frame_bytes(n: int, n_segments: int) -> int:
    return planes(n, n_segments)[4]


def quantise(v) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = (v - LO) * (CODES / SPAN)       # two roundings: the subtraction, the product
        q = np.floor(t + 0.5)                # a third: the sum
        q = np.where(q >= CODES, float(CODES), np.where(q > 0.0, q, 0.0))
    return np.where(np.isfinite(v), q, float(NOT_FINITE)).astype(np.uint16)


def dequantise(q) -> np.ndarray:
    q = np.asarray(q, dtype=np.uint16)
    return np.where(q == NOT_FINITE, np.inf, LO + q.astype(np.float64) * STEP)


def colour(pressure) -> np.ndarray:
    """render_spec.colour, restated: 255 - int(p * 255) clipped to a byte; NaN and +inf -> 0, -inf -> 255."""
    p = np.asarray(pressure, dtype=np.float64)
    with np.errstate(all="ignore"):
        cc = 255.0 - np.trunc(p * 255.0)
    return np.where(cc >= 255.0, 255.0, np.where(cc > 0.0, cc, 0.0)).astype(np.uint8)


def pressure_of(c) -> np.ndarray:
    return (255.0 - np.asarray(c, dtype=np.uint8).astype(np.float64) + 0.5) / 255.0


def pack(tick: int, xy, pressure, ids, segments, pressure_valid: bool = True, valid_slots=None) -> bytes:
    """The frame of particles `xy` (n x 2), `pressure` (n), `ids` (n) and walls `segments` (S x 2 x 2), in the order
    given.  Without `pressure_valid` every colour is 255; `valid_slots` (a bool mask) says which particles carry one."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 4)
    assert len(ids) == n and (n == 0 or (ids.min() >= 0 and ids.max() < 2 ** 31 - 1))
    c = colour(np.asarray(pressure, dtype=np.float64).reshape(-1)) if pressure_valid else np.full(n, 255, dtype=np.uint8)
    if pressure_valid and valid_slots is not None:
        c = np.where(np.asarray(valid_slots, dtype=bool), c, 255).astype(np.uint8)
    assert len(c) == n
    o_id, o_qx, o_qy, o_c, end = planes(n, len(seg))
    out = bytearray(end)
    _HEADER.pack_into(out, 0, MAGIC, VERSION, int(tick), n, len(seg), 1 if pressure_valid else 0, LO, SPAN)
    out[HEADER:o_id] = seg.astype("<f8").tobytes()
    out[o_id:o_id + 4 * n] = ids.astype("<u4").tobytes()
    out[o_qx:o_qx + 2 * n] = quantise(xy[:, 0]).astype("<u2").tobytes()
    out[o_qy:o_qy + 2 * n] = quantise(xy[:, 1]).astype("<u2").tobytes()
    out[o_c:o_c + n] = c.tobytes()
    return bytes(out)


def header(frame) -> dict:
    magic, version, tick, n, nseg, flags, lo, span = _HEADER.unpack_from(frame, 0)
    return dict(magic=magic, version=version, tick=tick, n=n, n_segments=nseg, flags=flags, lo=lo, span=span)


def parse(frame) -> dict:
    """-> tick, n, flags, segments (S x 2 x 2), ids (int64), qx, qy (uint16), c (uint8), xy (dequantised, n x 2), padding
    (the bytes between the planes' ends and the next multiple of 8, all of which are zero in a valid frame)."""
    h = header(frame)
    assert h["magic"] == MAGIC and h["version"] == VERSION and h["lo"] == LO and h["span"] == SPAN
    n, s = h["n"], h["n_segments"]
    o_id, o_qx, o_qy, o_c, end = planes(n, s)
    assert len(frame) == end and not any(frame[48:HEADER])
    buf = np.frombuffer(bytes(frame), dtype=np.uint8)
    seg = buf[HEADER:o_id].view("<f8").reshape(s, 2, 2).copy()
    ids = buf[o_id:o_id + 4 * n].view("<u4").astype(np.int64)
    qx = buf[o_qx:o_qx + 2 * n].view("<u2").copy()
    qy = buf[o_qy:o_qy + 2 * n].view("<u2").copy()
    c = buf[o_c:o_c + n].copy()
    padding = np.concatenate([buf[o_id + 4 * n:o_qx], buf[o_qx + 2 * n:o_qy], buf[o_qy + 2 * n:o_c], buf[o_c + n:end]])
    return dict(tick=h["tick"], n=n, flags=h["flags"], segments=seg, ids=ids, qx=qx, qy=qy, c=c,
                xy=np.stack([dequantise(qx), dequantise(qy)], axis=1), padding=padding)


def canonical(frame) -> bytes:
    """The same frame with its records in id order."""
    p = parse(frame)
    assert not p["padding"].any(), "the planes' padding must be zero"
    order = np.argsort(p["ids"], kind="stable")
    n, s = p["n"], len(p["segments"])
    o_id, o_qx, o_qy, o_c, end = planes(n, s)
    out = bytearray(frame)
    out[o_id:o_id + 4 * n] = p["ids"][order].astype("<u4").tobytes()
    out[o_qx:o_qx + 2 * n] = p["qx"][order].astype("<u2").tobytes()
    out[o_qy:o_qy + 2 * n] = p["qy"][order].astype("<u2").tobytes()
    out[o_c:o_c + n] = p["c"][order].tobytes()
    return bytes(out)
