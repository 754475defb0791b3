"""The pixel rule of the debug arrows (sc_set_arrows; sand_crate_amd/csrc/sc_arrows.h), written once in NumPy.

A device frame with arrows equals `draw(the frame without them, ...)` bit for bit when the arrows come from a list.

arrow    (start s, end e) in world units.  Screen points S = render_spec.screen(s), E = render_spec.screen(e) per axis,
         not floored: crate_to_screen_coord applied to `start` and to `start + direction` (playback.py:100-104).
skipped  an arrow with a world or screen number that is not finite, and one with a = E - S, L2 = ax ax + ay ay == 0
         (the reference draws a 4-pixel blob there; a resting particle should draw nothing).
covered  L = sqrt(L2), n = (-ay, ax); for pixel (i, j): p = (i - Sx, j - Sy), t = px ax + py ay, w = px nx + py ny, all
         float64, each operation rounded on its own, in this order.  The pixel is covered iff
           body (only when L2 >= 4):  0 <= t <= L2 - 2 L  and  w w <= L2
           head:                      L2 - 2 L <= t <= L2  and  |w| <= L2 - t
         pygame_utils.draw_arrow with the viewer's body_width = 2, head_width = 4, head_height = 2 as closed
         point-in-shape tests multiplied through by L: a rectangle of half-width 1 from S to 2 px before E, a triangle of
         half-width 2 there with its tip on E; arrows shorter than the head have no body.  The rule is ours (pygame's
         scanline filler is not pinned), as the disc rule is.
colour   (0, 255, 0) (DEBUG_ARROWS_COLOR), palette index 1 in a frame of indices; over discs and walls, under the HUD
         text; pixels outside the frame are dropped.
scaling  playback.py:99 compresses a direction before it is drawn: d' = d / (|d| + 0.001)^0.3, |d| = sqrt(dx dx + dy dy),
         e = s + d' (`compress`, `ends`).
box      the device looks only at the hull of S and E widened by 3 px and clipped to the frame (`box`).  Every pixel
         the rule covers lies inside it while the screen numbers stay below 2^40 or so; when they are so large that L2
         overflows the rule's comparisons are all false and nothing is drawn.
banded   `arrow_masks` leaves undecided every pixel with an inequality within slack max(1, L) of equality -- slack px in
         pixel units: what the velocity mode is compared with, whose `pow` runs on the device and need not be NumPy's
         to the last bit (a few ulp in d' move E by about 1e-11 px on a 16384-px frame).

The product never imports this module.
"""
from __future__ import annotations

import numpy as np

import render_spec as R

GREEN = (0, 255, 0)
MARGIN = 3        # px around the hull of S and E: the device's box
WAVE_BOX = 256    # a clipped box of more pixels than this is drawn by a whole wave (sc_arrows.h: kArrowWaveBox)
MAX_ARROWS = 1 << 20


def compress(direction) -> np.ndarray:
    """d' of playback.py:99 for directions K x 2."""
    d = np.asarray(direction, dtype=np.float64).reshape(-1, 2)
    with np.errstate(all="ignore"):
        norm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        return d / np.power(norm + 0.001, 0.3)[:, None]


def ends(pairs) -> np.ndarray:
    """K x 2 x 2 (start, end) of K x 2 x 2 (start, direction): NaN entries dropped (playback.py:97), e = s + d'."""
    a = np.asarray(pairs, dtype=np.float64).reshape(-1, 2, 2)
    a = a[~np.isnan(a).any(axis=(1, 2))]
    with np.errstate(all="ignore"):
        return np.stack([a[:, 0], a[:, 0] + compress(a[:, 1])], axis=1)


def view_center(width, height, center):
    return (width / 2, height / 2) if center is None else (float(center[0]), float(center[1]))


def on_screen(arrow, width, height, zoom=1.0, center=None):
    """(Sx, Sy, Ex, Ey) of one (start, end), or None for an arrow that is skipped before L2 is looked at."""
    (sx, sy), (ex, ey) = np.asarray(arrow, dtype=np.float64).reshape(2, 2)
    if not np.isfinite([sx, sy, ex, ey]).all():
        return None
    cx, cy = view_center(width, height, center)
    with np.errstate(all="ignore"):
        S = (float(R.screen(sx, width, cx, zoom)), float(R.screen(sy, height, cy, zoom)),
             float(R.screen(ex, width, cx, zoom)), float(R.screen(ey, height, cy, zoom)))
    return S if np.isfinite(S).all() else None


def _terms(S, width, height):
    """What the inequalities compare, on the whole frame: (L2, L, t, w) -- or None when L2 == 0."""
    Sx, Sy, Ex, Ey = (np.float64(v) for v in S)
    with np.errstate(all="ignore"):
        ax, ay = Ex - Sx, Ey - Sy
        L2 = ax * ax + ay * ay
        if L2 == 0:
            return None
        L = np.sqrt(L2)
        nx, ny = -ay, ax
        jj, ii = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
        px, py = ii - Sx, jj - Sy
        t = px * ax + py * ay
        w = px * nx + py * ny
    return L2, L, t, w


def covered(arrow, width, height, zoom=1.0, center=None) -> np.ndarray:
    """H x W bool: the pixels one (start, end) covers."""
    S = on_screen(arrow, width, height, zoom, center)
    terms = None if S is None else _terms(S, width, height)
    if terms is None:
        return np.zeros((height, width), dtype=bool)
    L2, L, t, w = terms
    with np.errstate(all="ignore"):
        neck = L2 - 2.0 * L
        body = (L2 >= 4.0) & (0.0 <= t) & (t <= neck) & (w * w <= L2)
        head = (neck <= t) & (t <= L2) & (np.abs(w) <= L2 - t)
    return body | head


def mask(arrows, width, height, zoom=1.0, center=None) -> np.ndarray:
    """H x W bool: the pixels some arrow of K x 2 x 2 (start, end) covers."""
    out = np.zeros((height, width), dtype=bool)
    for arrow in np.asarray(arrows, dtype=np.float64).reshape(-1, 2, 2):
        out |= covered(arrow, width, height, zoom, center)
    return out


def arrow_masks(arrows, width, height, zoom=1.0, center=None, slack=1e-6):
    """(sure_in, sure_out), H x W bool each: pixels some arrow covers with every inequality of a covering shape more than
    slack max(1, L) inside, and pixels no arrow covers with, for every arrow and both shapes, some inequality more than
    that outside.  The rest is undecided."""
    sure_in = np.zeros((height, width), dtype=bool)
    maybe = np.zeros((height, width), dtype=bool)
    for arrow in np.asarray(arrows, dtype=np.float64).reshape(-1, 2, 2):
        S = on_screen(arrow, width, height, zoom, center)
        terms = None if S is None else _terms(S, width, height)
        if terms is None:
            continue  # (an arrow at the edge of being skipped -- L2 next to 0 -- is the caller's to avoid)
        L2, L, t, w = terms
        with np.errstate(all="ignore"):
            m = slack * max(1.0, L)
            # every comparison as a margin: positive inside.  t and w carry a factor L, w w and L2 - t as well
            neck = L2 - 2.0 * L
            body = np.minimum(np.minimum(t, neck - t), (L - np.abs(w)))
            head = np.minimum(np.minimum(t - neck, L2 - t), (L2 - t) - np.abs(w))
            if abs(L2 - 4.0) <= m:  # (the body's own switch next to equality: it may be there or not)
                maybe |= body >= -m
            elif L2 >= 4.0:
                sure_in |= body > m
                maybe |= body >= -m
            sure_in |= head > m
            maybe |= head >= -m
    return sure_in, ~maybe


def box(arrow, width, height, zoom=1.0, center=None):
    """(x0, y0, columns, rows) of the device's box of one (start, end) -- the hull of S and E widened by MARGIN, clipped to
    the frame -- or None when the arrow is skipped or the box is empty."""
    S = on_screen(arrow, width, height, zoom, center)
    if S is None or _terms(S, 1, 1) is None:
        return None
    Sx, Sy, Ex, Ey = S
    x0, x1 = max(np.ceil(min(Sx, Ex) - MARGIN), 0.0), min(np.floor(max(Sx, Ex) + MARGIN), width - 1.0)
    y0, y1 = max(np.ceil(min(Sy, Ey) - MARGIN), 0.0), min(np.floor(max(Sy, Ey) + MARGIN), height - 1.0)
    if not (x0 <= x1 and y0 <= y1):
        return None
    return int(x0), int(y0), int(x1) - int(x0) + 1, int(y1) - int(y0) + 1


def draw(frame, arrows, zoom=1.0, center=None) -> np.ndarray:
    """A copy of `frame` -- H x W x 3 RGB or H x W palette indices, uint8 -- with the arrows K x 2 x 2 (start, end) on it."""
    out = np.array(frame, dtype=np.uint8)
    assert out.ndim in (2, 3) and (out.ndim == 2 or out.shape[2] == 3)
    ink = mask(arrows, out.shape[1], out.shape[0], zoom, center)
    out[ink] = 1 if out.ndim == 2 else GREEN
    return out


def velocity_ends(xy, vxy, ids, scale, every) -> np.ndarray:
    """K x 2 x 2 (start, end) of the velocity mode: a particle whose id is a multiple of `every`, from its position along
    velocity * scale, compressed."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    vxy = np.asarray(vxy, dtype=np.float64).reshape(-1, 2)
    pick = np.asarray(ids, dtype=np.int64).reshape(-1) % int(every) == 0
    with np.errstate(all="ignore"):
        return np.stack([xy[pick], xy[pick] + compress(vxy[pick] * float(scale))], axis=1)


def indices(rgb_frame) -> np.ndarray:
    """H x W uint8 palette indices of a frame rendered while arrows are set: background 0, an arrow pixel 1, a wall or
    text 255, a disc of colour byte c max(c, 2)."""
    rgb = np.asarray(rgb_frame, dtype=np.uint8)
    arrow = (rgb[..., 0] == 0) & (rgb[..., 1] == 255) & (rgb[..., 2] == 0)
    return np.where(arrow, 1, np.where(rgb[..., 2] == 0, 0, np.maximum(rgb[..., 0], 2))).astype(np.uint8)


def palette() -> np.ndarray:
    """256 x 3 uint8: gif_spec's palette with entry 1 the arrows' green."""
    k = np.arange(256, dtype=np.uint8)
    pal = np.stack([k, k, np.full(256, 255, dtype=np.uint8)], axis=1)
    pal[0] = 0
    pal[1] = GREEN
    return pal
