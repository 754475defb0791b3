"""The raster rule of `sc_render` (sand_crate_amd/csrc/sc_render.h), written once in NumPy.

The device output equals `render(...)` bit for bit.  The rule follows the reference's viewer (``src/playback.py``):

view     cx = trunc(x (W - 1)); X = (cx - center_x) zoom + W/2 in float64 in that order; pixel column floor(X).  Rows
         the same with y, H, center_y; row 0 is the top (+y points down).  Defaults: center (W/2, H/2), zoom 1
         (crate_to_screen_coord, playback.py:208-213).
discs    R = floor(trunc(W particle_radius) zoom) (playback.py:195 uses screen_x for both axes).  Pixel (i, j) is covered
         iff (i - px)^2 + (j - py)^2 <= R^2 in integers, inside the frame only; R = 0 paints the centre pixel.  Particles
         whose x or y is not finite, or whose disc misses the frame (tested in float64), are skipped.
colour   c = 255 - trunc(p 255) clipped to [0, 255]: 0 for a pressure of NaN or +inf, 255 for -inf; the pixel is
         (c, c, 255) (playback.py:197-200).
order    among discs covering a pixel the highest id wins (the reference draws in array order).
walls    drawn last, white, endpoints mapped by the same view but not floored.  Pixel (i, j) is covered iff
         4 e <= w^2, e the squared distance to the segment in float64:  dx = bx - ax, dy = by - ay, L = dx dx + dy dy,
         t = 0 if L == 0 else clip(((i - ax) dx + (j - ay) dy) / L, 0, 1), qx = ax + t dx, qy = ay + t dy,
         e = (i - qx)(i - qx) + (j - qy)(j - qy).
empty    black.  Output: uint8 H x W x 3, row-major (pygame.image.tostring(..., 'RGB')).

The product never imports this module.
"""
from __future__ import annotations

import numpy as np


def screen(v, side: int, center: float, zoom: float):
    """Screen coordinate (not floored) of world coordinate(s) v along an axis of `side` pixels."""
    return (np.trunc(np.asarray(v, dtype=np.float64) * (side - 1)) - center) * zoom + side / 2


def disc_radius(width: int, particle_radius: float, zoom: float) -> int:
    return int(np.floor(np.trunc(width * particle_radius) * zoom))


def colour(pressure) -> np.ndarray:
    """c of playback.py:197-200 per particle (uint8)."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = 255.0 - np.trunc(np.asarray(pressure, dtype=np.float64) * 255.0)
    c = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 255.0))
    return c.astype(np.uint8)


def particle_keys(xy, pressure, ids, width, height, particle_radius, zoom=1.0, center=None):
    """The per-pixel key max((id + 1) << 8 | c) over the discs covering it (0: none), H x W uint64."""
    cx, cy = (width / 2, height / 2) if center is None else (float(center[0]), float(center[1]))
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    keys = np.zeros(height * width, dtype=np.uint64)
    R = disc_radius(width, particle_radius, zoom)
    ok = np.isfinite(xy[:, 0]) & np.isfinite(xy[:, 1])
    with np.errstate(invalid="ignore", over="ignore"):
        X = np.floor(screen(xy[:, 0], width, cx, zoom))
        Y = np.floor(screen(xy[:, 1], height, cy, zoom))
        ok &= (X + R >= 0) & (X - R <= width - 1) & (Y + R >= 0) & (Y - R <= height - 1)
    px, py = X[ok].astype(np.int64), Y[ok].astype(np.int64)
    key = ((ids[ok] + 1).astype(np.uint64) << np.uint64(8)) | colour(np.asarray(pressure)[ok]).astype(np.uint64)
    for ey in range(-R, R + 1):
        for ex in range(-R, R + 1):
            if ex * ex + ey * ey > R * R:
                continue
            i, j = px + ex, py + ey
            inside = (i >= 0) & (i < width) & (j >= 0) & (j < height)
            np.maximum.at(keys, j[inside] * width + i[inside], key[inside])
    return keys.reshape(height, width)


def wall_mask(segments, width, height, zoom=1.0, center=None, segment_width=2):
    """H x W bool: pixels some wall segment covers."""
    cx, cy = (width / 2, height / 2) if center is None else (float(center[0]), float(center[1]))
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 2)
    mask = np.zeros((height, width), dtype=bool)
    w2 = float(segment_width) * float(segment_width)
    jj, ii = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    for (x0, y0), (x1, y1) in seg:
        ax, bx = screen([x0, x1], width, cx, zoom)
        ay, by = screen([y0, y1], height, cy, zoom)
        if not np.isfinite([ax, ay, bx, by]).all():
            continue  # (the formula gives NaN for every pixel: nothing covered)
        dx, dy = bx - ax, by - ay
        L = dx * dx + dy * dy
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            t = np.zeros_like(ii) if L == 0 else np.clip(((ii - ax) * dx + (jj - ay) * dy) / L, 0.0, 1.0)
            qx = ax + t * dx
            qy = ay + t * dy
            e = (ii - qx) * (ii - qx) + (jj - qy) * (jj - qy)
            mask |= 4.0 * e <= w2
    return mask


def render(xy, pressure, ids, segments, width, height, particle_radius, zoom=1.0, center=None, segment_width=2):
    """The frame: H x W x 3 uint8."""
    keys = particle_keys(xy, pressure, ids, width, height, particle_radius, zoom, center)
    c = (keys & np.uint64(0xFF)).astype(np.uint8)
    img = np.zeros((height, width, 3), dtype=np.uint8)
    hit = keys != 0
    img[hit, 0] = c[hit]
    img[hit, 1] = c[hit]
    img[hit, 2] = 255
    img[wall_mask(segments, width, height, zoom, center, segment_width)] = 255
    return img
