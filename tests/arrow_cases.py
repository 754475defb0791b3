"""The named cases of the debug-arrow tests (tests/test_arrows_cpu.py proves each has the property it is named for,
tests/test_gpu_arrows.py draws them): views, lists of (start, direction) in world units as `Crate.render(arrows=...)`
takes them, and the uploaded states of the velocity mode.

Arrows are written down in cells: cell k of an axis is the world coordinate whose `trunc(x (side - 1))` is k, so the
screen point of cell k is (k - center) zoom + side / 2 exactly, and an arrow from cell p to cell q has the direction
that `arrow_spec.compress` turns into q - p cells (`uncompress` inverts playback.py:99; the half cell of room that
trunc leaves swallows its rounding).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import arrow_spec as A


@dataclass(frozen=True)
class Case:
    width: int
    height: int
    pairs: np.ndarray          # K x 2 x 2 (start, direction), world units
    zoom: float = 1.0
    center: tuple | None = None
    hud: bytes | None = None   # a HUD text drawn over the arrows (at text_spec's default place, scale 1)

    @property
    def view(self) -> dict:
        return dict(zoom=self.zoom, center=self.center)

    @property
    def ends(self) -> np.ndarray:
        return A.ends(self.pairs)


def world(cell, side: int) -> float:
    """The world coordinate in the middle of cell `cell` of an axis of `side` pixels."""
    return (cell + (0.5 if cell >= 0 else -0.5)) / (side - 1)


def uncompress(dprime) -> np.ndarray:
    """d with compress(d) == dprime up to rounding: |d| solves m / (m + 0.001)^0.3 = |dprime| (bisection)."""
    dprime = np.asarray(dprime, dtype=np.float64)
    r = float(np.hypot(*dprime))
    if r == 0.0:
        return np.zeros(2)
    lo, hi = 0.0, max(1.0, r) ** 2 + 1.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid / (mid + 0.001) ** 0.3 < r:
            lo = mid
        else:
            hi = mid
    return dprime * (hi / r)


def cells(width: int, height: int, arrows) -> np.ndarray:
    """(start, direction) pairs of arrows given as (from cell x, from cell y, to cell x, to cell y)."""
    out = []
    for x0, y0, x1, y1 in arrows:
        s = np.array([world(x0, width), world(y0, height)])
        e = np.array([world(x1, width), world(y1, height)])
        out.append([s, uncompress(e - s)])
    return np.array(out, dtype=np.float64).reshape(-1, 2, 2)


def to_cells(pairs, width: int, height: int) -> np.ndarray:
    """K x 4: the cells (from x, from y, to x, to y) the spec's view truncates each arrow of `pairs` to."""
    e = A.ends(pairs)
    with np.errstate(all="ignore"):
        return np.trunc(np.stack([e[:, 0, 0] * (width - 1), e[:, 0, 1] * (height - 1),
                                  e[:, 1, 0] * (width - 1), e[:, 1, 1] * (height - 1)], axis=1))


AXES = [(10, 10, 16, 10), (40, 10, 34, 10), (10, 30, 10, 36), (40, 36, 40, 30)]  # L = 6 along +x, -x, +y, -y
SHORT = [(16, 12, 17, 12), (22, 12, 22, 13), (28, 12, 27, 12), (34, 12, 34, 11), (40, 12, 41, 13), (20, 24, 20, 24)]


def _random_cells(seed: int, n: int, width: int, height: int, reach: int):
    rs = np.random.RandomState(seed)
    x0, y0 = rs.randint(0, width, n), rs.randint(0, height, n)
    return np.stack([x0, y0, x0 + rs.randint(-reach, reach + 1, n), y0 + rs.randint(-reach, reach + 1, n)], axis=1).tolist()


def _nonfinite() -> np.ndarray:
    good = cells(64, 48, [(20, 20, 30, 26)])[0]
    nan, inf = float("nan"), float("inf")
    bad = [[[nan, 0.5], [0.1, 0.0]], [[0.5, 0.5], [0.1, nan]],     # a NaN: dropped on the host (playback.py:97)
           [[inf, 0.5], [0.1, 0.0]], [[0.5, -inf], [0.0, 0.1]],    # an infinite start
           [[0.5, 0.5], [inf, 0.0]], [[0.5, 0.5], [0.1, -inf]]]    # an infinite direction: the end is not finite
    return np.array(bad[:3] + [good] + bad[3:], dtype=np.float64)


def _edges() -> np.ndarray:
    w, h = 64, 48
    half = [(-4, 20, 5, 24), (58, 20, 68, 16), (30, -5, 26, 4), (30, 43, 34, 52), (3, 3, -6, -6), (60, 44, 70, 54)]
    outside = [(-30, 20, -12, 20), (80, 20, 100, 30), (30, -40, 30, -10), (30, 60, 20, 80), (-9, -9, -5, -5),
               (71, 10, 67, 20)]  # the last: its box starts one column right of the frame
    huge = np.array([[[0.5, 0.5], [1e300, 0.0]], [[0.5, 0.5], [-1e300, 1e300]], [[1e300, -1e300], [0.01, 0.01]],
                     [[-1e300, 0.5], [1e300, 0.0]],
                     [[0.3, 0.6], [1e4, 0.0]], [[0.7, 0.2], [-3e3, 2e3]]])  # the last two: far, but L2 stays finite
    return np.concatenate([cells(w, h, half + outside), huge])


def _pile() -> np.ndarray:
    rs = np.random.RandomState(5)
    n = 4096
    to = np.stack([32 + rs.randint(-7, 8, n), 24 + rs.randint(-7, 8, n)], axis=1)
    return cells(64, 48, [(32, 24, int(x), int(y)) for x, y in to])


LAYERS_TEXT = b"Tick: 12\nwalls < arrows < text"


def cases() -> dict[str, Case]:
    return {
        # axis-aligned from integer S (W and H even, zoom 1): the |w| and t equalities land exactly on pixels
        "axes": Case(64, 48, cells(64, 48, AXES)),
        # odd W and H: half-integer S
        "odd_zoom_2.5": Case(61, 37, cells(61, 37, [(20, 14, 26, 14), (22, 18, 19, 23), (30, 20, 24, 12), (18, 10, 18, 15),
                                                   (27, 13, 31, 17), (24, 16, 24, 16)]), zoom=2.5, center=(25.0, 16.5)),
        "odd_zoom_0.4": Case(61, 37, cells(61, 37, [(0, 0, 40, 30), (60, 0, 20, 36), (30, 18, 60, 18), (10, 30, 10, 5),
                                                   (45, 30, 50, 33), (5, 5, 7, 5)]), zoom=0.4, center=(40.0, 10.0)),
        "diagonal": Case(128, 96, cells(128, 96, [(10, 10, 30, 30), (60, 40, 40, 60), (100, 80, 90, 70), (20, 80, 45, 55),
                                                  (64, 48, 65, 49), (64, 20, 66, 22)])),
        "random": Case(128, 96, cells(128, 96, _random_cells(3, 60, 128, 96, 25))),
        "random_zoomed": Case(127, 95, cells(127, 95, _random_cells(4, 60, 127, 95, 25)), zoom=1.37, center=(70.25, 41.5)),
        # one cell at a zoom of nearly 2, exactly 2 and a little more: L on both sides of where the body starts
        "L_below_2": Case(64, 48, cells(64, 48, SHORT), zoom=2.0 - 1e-7, center=(30.0, 20.0)),
        "L_exactly_2": Case(64, 48, cells(64, 48, SHORT), zoom=2.0, center=(30.0, 20.0)),
        "L_above_2": Case(64, 48, cells(64, 48, SHORT), zoom=2.0 + 1e-7, center=(30.0, 20.0)),
        "nonfinite": Case(64, 48, _nonfinite()),
        "edges": Case(64, 48, _edges()),
        # the whole frame diagonally, and clipped boxes of 16 x 16 = 256 pixels (a thread), 17 x 16 (the wave), and
        # 7 x 36 = 252 against 7 x 37 = 259
        "whole_frame": Case(128, 96, cells(128, 96, [(0, 0, 127, 95)])),
        "box_at_threshold": Case(128, 96, cells(128, 96, [(20, 20, 29, 29), (20, 60, 49, 60)])),
        "box_over_threshold": Case(128, 96, cells(128, 96, [(20, 20, 30, 29), (20, 60, 50, 60)])),
        "box_both": Case(128, 96, cells(128, 96, [(20, 20, 29, 29), (60, 20, 70, 29), (20, 60, 49, 60), (70, 70, 100, 70)])),
        "pile": Case(64, 48, _pile()),
        # over discs, the thick wall at the frame's edge and the HUD text: walls < arrows < text
        "layers": Case(160, 120, cells(160, 120, [(1, 1, 150, 60), (2, 14, 120, 14), (40, 2, 40, 110), (155, 110, 20, 30),
                                                  (8, 8, 60, 30), (0, 60, 159, 60)]), hud=LAYERS_TEXT),
    }


@dataclass(frozen=True)
class VelocityCase:
    width: int
    height: int
    zoom: float
    center: tuple
    xy: np.ndarray      # n x 2, uploaded through Crate.particles: ids are 0 .. n - 1
    vxy: np.ndarray
    every: int
    scale: float

    @property
    def view(self) -> dict:
        return dict(zoom=self.zoom, center=self.center)

    @property
    def ends(self) -> np.ndarray:
        return A.velocity_ends(self.xy, self.vxy, np.arange(len(self.xy)), self.scale, self.every)


def velocity_state(n: int = 600, seed: int = 21):
    """Positions all over the world and a little beyond, velocities of every direction; some particles at rest (no
    arrow), and one velocity that is not finite."""
    rs = np.random.RandomState(seed)
    xy = rs.rand(n, 2) * 1.1 - 0.05
    vxy = (rs.rand(n, 2) - 0.5) * 1.2
    vxy[::17] = 0.0
    vxy[5, 0] = np.inf
    return xy, vxy


def velocity_cases() -> dict[str, VelocityCase]:
    xy, vxy = velocity_state()
    view = dict(width=160, height=120, zoom=1.37, center=(83.3, 57.6))
    return {f"every{every}_scale{scale}": VelocityCase(xy=xy, vxy=vxy, every=every, scale=scale, **view)
            for every in (1, 3) for scale in (0.04, 0.3)}


def undecided_share(ends, width, height, zoom, center) -> tuple[int, int]:
    """(undecided pixels, sure_in pixels) of arrow_masks."""
    sure_in, sure_out = A.arrow_masks(ends, width, height, zoom, center)
    assert not (sure_in & sure_out).any()
    return int((~sure_in & ~sure_out).sum()), int(sure_in.sum())


def trunc_room(ends, width, height) -> float:
    """How far the nearest `e (side - 1)` of the arrows' finite ends is from a whole number: the view truncates there, so
    an end that close to one could land a cell away when its last bits differ."""
    e = np.asarray(ends, dtype=np.float64).reshape(-1, 2, 2)[:, 1]
    with np.errstate(all="ignore"):
        v = np.concatenate([e[:, 0] * (width - 1), e[:, 1] * (height - 1)])
    v = v[np.isfinite(v) & (np.abs(v) < 1e9)]
    return float(np.min(np.abs(v - np.round(v)))) if len(v) else 1.0
