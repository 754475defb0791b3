"""Worlds in which one of the wall pass's shortcuts decides the result (tests/test_gpu_walls.py, tests/test_wall_cases_cpu.py,
tests/golden/make_golden.py: tick_walls_*).

The device skips most of the wall and crossing work of a tick, each shortcut argued exact in a comment:
  far_box / ccd_skip2  a particle whose segment boxes all lie beyond far_box = r + 2d (K1: wslot -1) and that moves less
                       than 2d skips the crossing test (sc_tiled.h: pass_b_finish; sandcrate_hip.hip: build_world);
  near_now             a wave whose particles all move less than kNearSteps = 8 cells tests only the segments within
                       far_box + 6d of its block's box; the box spans the block's first and last particle (one strip:
                       their x; more: the full width), widened by d in y (sc_tiled.h: k_pass_b);
  near_next / strayed  the fused next-tick wall pass looks only at segments within far_box + 8d of the box, unless a
                       particle of the wave moved more than 8 cells in a coordinate;
  floor_div            row / column as floor(p * (1/d)), floor(p / d) inside a 1e-12 band (sc_kernels.h);
  t_wall               contact as s <= t_wall, the largest s with sqrt(s) <= 1.2 r (crate.py:229);
  one_each, 1/V        wave-wide ballots that fall back when any lane differs.
Each builder returns a Case whose particles sit where the argument is tight.  Forces are zeroed in most worlds
(`QUIET`: no pressure -- ignored_pressure above any density --, no tension, viscosity or gravity), so that a particle's
path is the velocity the case gave it; the junction world keeps them on.  The cells per tick of a velocity v are
v * DT / D = v / 5.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from oracle.neighbors import strip_sort
from oracle.scene import OracleCrate
from oracle.world import World

TILE = 256        # particles per block of the tiled passes (sc_device.h: kTileW)
WAVE = 64
TILE_CAP_B = 960  # pass B keeps a tile of at most this many entries in LDS (sc_tiled.h: kTileCapB)
NEAR_STEPS = 8    # sc_tiled.h: kNearSteps

# A diameter whose contact threshold is NOT the rounded square: sq_threshold(1.2 r) = fl((1.2 r)^2) + 1 ulp here, so a
# squared distance of exactly t_wall touches (sqrt rule) where s <= fl((1.2 r)^2) would not.
D = 0.01012
R = D / 2
DT = 0.002 * D / 0.01
FAR_BOX = R + 2 * D


def cells(n):
    """The speed that moves a particle n cells per tick."""
    return n * D / DT


QUIET = dict(dt=DT, particle_radius=R, wall_collision_decay=0.5, pressure_amplifier=0.0, ignored_pressure=1000.0,
             collider_noise_level=0.1, viscosity=0.0, surface_smoothing=0.0, target_pressure=0.0, gravity=[0.0, 0.0],
             max_particles=100000)
LIVELY = dict(dt=DT, particle_radius=R, wall_collision_decay=0.3, pressure_amplifier=30.0, ignored_pressure=0.2,
              collider_noise_level=0.1, viscosity=4.0, surface_smoothing=80.0, target_pressure=-1.0,
              gravity=[1.5, -9.8], max_particles=100000)


@dataclass
class Case:
    name: str
    bodies: list            # rigid body configs, as in a scene's YAML
    coef: dict
    p: np.ndarray
    v: np.ndarray
    marks: dict = field(default_factory=dict)   # name -> indices (original order) of the particles a premise is about

    def oracle(self):
        return OracleCrate(World(self.bodies, [], dict(self.coef)))


def fixed(*segments, name="wall"):
    return {"fixed": {"name": name, "segments": [[list(map(float, a)), list(map(float, b))] for a, b in segments]}}


BOX = fixed(((0, 0), (1, 0)), ((1, 0), (1, 1)), ((1, 1), (0, 1)), ((0, 1), (0, 0)), name="box")


# ------------------------------------------------------------------ geometry the premises use
def sq_threshold(x):
    """sandcrate_hip.hip: sq_threshold -- the largest s with sqrt(s) <= x."""
    t = x * x
    while math.sqrt(t) > x:
        t = float(np.nextafter(t, -np.inf))
    while math.sqrt(float(np.nextafter(t, np.inf))) <= x:
        t = float(np.nextafter(t, np.inf))
    return t


def squared_distances(p, segments):
    """geometry_utils.py:7-39 as the oracle evaluates it, before the sqrt: (P, S)."""
    a, b = segments[:, 0], segments[:, 1]
    ab = (b - a)[None]
    ap = p[:, None] - a[None]
    t = np.clip((ap * ab).sum(2) / (ab * ab).sum(2), 0, 1)
    pc = ab * t[:, :, None] + a[None] - p[:, None]
    return pc[..., 0] * pc[..., 0] + pc[..., 1] * pc[..., 1]


def block_boxes(p, d=D):
    """The box of every block as k_pass_b forms it, from the oracle's strip sort of the (fixed) positions p:
    -> order, rows, and per block (x0, x1, y0, y1, one_strip)."""
    rows, order = strip_sort(p, d)
    boxes = []
    for b0 in range(0, len(order), TILE):
        blk = order[b0:b0 + TILE]
        first, last = p[blk[0]], p[blk[-1]]
        one = rows[min(b0 + TILE, len(order)) - 1] == rows[b0]
        x0, x1 = (first[0], last[0]) if one else (-d / 2, 1 + d / 2)
        boxes.append((x0, x1, first[1] - d, last[1] + d, bool(one)))
    return order, rows, boxes


def box_gap(box, seg):
    """Per-axis gap between a block's box and a segment's bounding box (k_pass_b: box_gap)."""
    x0, x1, y0, y1 = box[:4]
    (ax, ay), (bx, by) = seg
    ox = max(min(ax, bx) - x1, x0 - max(ax, bx), 0.0)
    oy = max(min(ay, by) - y1, y0 - max(ay, by), 0.0)
    return ox, oy


def block_of(order, i):
    return int(np.flatnonzero(order == i)[0]) // TILE


# ------------------------------------------------------------------ builders of background particles
def strip(rs, row, n, x0, x1, lo=0.15, hi=0.85):
    """n particles in one row of cells, evenly over [x0, x1] in x (jittered), y inside the row."""
    x = np.linspace(x0, x1, n) + (rs.rand(n) - 0.5) * (x1 - x0) / n * 0.5
    y = (row + lo + rs.rand(n) * (hi - lo)) * D
    return np.column_stack((x, y))


def last_in_row(p, idx):
    """Of the particles idx (one row), the last in the (row, x) order and the first."""
    k = idx[np.argsort(p[idx, 0], kind="stable")]
    return int(k[-1]), int(k[0])


# ------------------------------------------------------------------ case 1: far_box and ccd_skip2
def far_box_case():
    """Particles whose segment boxes are just beyond far_box (K1 calls them far), moving just over 2d toward a wall (the
    crossing test must still run: ccd_skip2) and just under (they cannot reach the padded segment); and particles just
    inside far_box moving under 2d into the wall (not far: the test runs although the step is short)."""
    rs = np.random.RandomState(101)
    walls = [fixed(((0.5, 0.1), (0.5, 0.9)), name="vertical"), fixed(((0.1, 0.5), (0.4, 0.5)), name="horizontal")]
    pts, vel = [], []
    marks = {"beyond_cross": [], "beyond_short": [], "inside_cross": []}
    specs = [("beyond_cross", 2.05, 2.3), ("beyond_cross", 2.2, 2.6), ("beyond_cross", 2.6, 2.95),
             ("beyond_short", 2.05, 1.95), ("beyond_short", 2.4, 1.9),
             ("inside_cross", 1.5, 1.8), ("inside_cross", 1.1, 1.9), ("inside_cross", 1.9, 1.97)]
    for k, (kind, gap, step) in enumerate(specs):
        for side in (-1, 1):
            # vertical wall at x = 0.5: gap r + gap*d from it, moving toward it
            y = 0.15 + 0.04 * k + (0.3 if side > 0 else 0.0)
            marks[kind].append(len(pts))
            pts.append((0.5 + side * (R + gap * D), y))
            vel.append((-side * cells(step), cells(0.03) * (rs.rand() - 0.5)))
            # horizontal wall at y = 0.5 (x in [0.1, 0.4])
            marks[kind].append(len(pts))
            pts.append((0.12 + 0.017 * k + (0.14 if side > 0 else 0.0), 0.5 + side * (R + gap * D)))
            vel.append((cells(0.03) * (rs.rand() - 0.5), -side * cells(step)))
    special = np.array(pts)
    # slow background away from the walls, so that the blocks are full
    bg = np.column_stack((0.6 + rs.rand(700) * 0.35, 0.05 + rs.rand(700) * 0.9))
    p = np.vstack((special, bg))
    v = np.vstack((np.array(vel), (rs.rand(700, 2) - 0.5) * cells(0.5)))
    return Case("far_box", [BOX] + walls, dict(QUIET), p, v, {k: np.array(x) for k, x in marks.items()})


# ------------------------------------------------------------------ case 2: near_now (this tick's crossing test)
def near_now_case(coef=None, with_pile=True):
    """Blocks of one strip (rows of 256), of four strips (rows of 64) and a dense pile whose tiles exceed kTileCapB.
    In each, one particle of an otherwise still block
      band_*      moves 7.8 cells and crosses a segment whose gap from the block's box lies in (far_box + 5d, far_box + 6d]
                  -- inside near_now, outside a mask one cell smaller;
      fallback_*  moves 12 cells and crosses a segment far outside near_now: only the wave's fallback to every segment
                  sees it.
    band_multi sits in the last row of its block with a larger y than the block's last particle: its segment is near
    only through the box's +d in y."""
    rs = np.random.RandomState(202)
    parts, segs, marks = [], [], {}
    base = 0

    def add(arr):
        nonlocal base
        parts.append(arr)
        idx = np.arange(base, base + len(arr))
        base += len(arr)
        return idx

    # one-strip blocks: rows 20 and 23, 256 each
    r20 = add(strip(rs, 20, TILE, 0.15, 0.45))
    r23 = add(strip(rs, 23, TILE, 0.15, 0.45))
    # four-strip blocks: rows 40-43 and 60-63, 64 each
    g40 = [add(strip(rs, 40 + k, TILE // 4, 0.15, 0.45)) for k in range(4)]
    g60 = [add(strip(rs, 60 + k, TILE // 4, 0.15, 0.45)) for k in range(4)]
    # a dense pile in row 80: 5 blocks of one strip, tiles far beyond kTileCapB entries
    pile = add(np.column_stack((0.3 + rs.rand(5 * TILE) * 1.5 * D, (80.1 + rs.rand(5 * TILE) * 0.8) * D))[:5 * TILE * with_pile])
    p = np.vstack(parts)
    v = np.zeros_like(p)

    def vertical(x, y, half=2.5):
        segs.append(fixed(((x, y - half * D), (x, y + half * D)), name="v"))

    def horizontal(x, y, half=2.5):
        segs.append(fixed(((x - half * D, y), (x + half * D, y)), name="h"))

    # band, one strip, to the right: the last particle of row 20's block
    i, _ = last_in_row(p, r20)
    v[i] = (cells(7.8), 0.0)
    vertical(p[i, 0] + R + 7.5 * D, p[i, 1])
    marks["band_strip"] = [i]
    # band, one strip, to the left: the first particle of row 23's block
    _, i = last_in_row(p, r23)
    v[i] = (-cells(7.8), 0.0)
    vertical(p[i, 0] - R - 7.5 * D, p[i, 1])
    marks["band_strip"].append(i)
    # fallback, one strip: a particle in the middle of row 20 moving 12 cells up (-y)
    i = int(r20[100])
    v[i] = (0.0, -cells(12))
    horizontal(p[i, 0], p[i, 1] - R - 11 * D)
    marks["fallback_strip"] = [i]
    # fallback, four strips: a particle of row 42 moving 12 cells down (+y)
    i = int(g40[2][30])
    v[i] = (0.0, cells(12))
    horizontal(p[i, 0], p[i, 1] + R + 11 * D)
    marks["fallback_multi"] = [i]
    # band, four strips: the block's last particle (largest x in row 63) sits low in its row; another particle of that
    # row sits high and moves 7.8 cells down to a segment r + 7.2 d below the box's bottom edge (y_last + d)
    last, _ = last_in_row(p, g60[3])
    p[last, 1] = (63 + 0.05) * D
    i = int(g60[3][20])
    p[i, 1] = (63 + 0.95) * D
    v[i] = (0.0, cells(7.8))
    horizontal(p[i, 0], p[last, 1] + D + R + 7.2 * D)
    marks["band_multi"] = [i]
    marks["band_pile"], marks["fallback_pile"] = [], []
    if with_pile:
        # the pile: its second block's last particle crosses a band segment to the right, its fourth block's last particle
        # a far segment to the left
        order, _, _ = block_boxes(p)
        b5_last, b7_last = int(order[6 * TILE - 1]), int(order[8 * TILE - 1])
        assert b5_last in pile and b7_last in pile
        v[b5_last] = (cells(7.8), 0.0)
        vertical(p[b5_last, 0] + R + 7.5 * D, p[b5_last, 1])
        v[b7_last] = (-cells(12), 0.0)
        vertical(p[b7_last, 0] - R - 11 * D, p[b7_last, 1])
        marks["band_pile"] = [b5_last]
        marks["fallback_pile"] = [b7_last]
    marks["band"] = marks["band_strip"] + marks["band_multi"] + marks["band_pile"]
    marks["fallback"] = marks["fallback_strip"] + marks["fallback_multi"] + marks["fallback_pile"]
    marks["pile"] = list(pile)
    return Case("near_now", [BOX] + segs, dict(coef or QUIET), p, v, {k: np.array(x) for k, x in marks.items()})


# ------------------------------------------------------------------ case 3: near_next / strayed (fused wall pass)
def near_next_case():
    """Particles that land within 1.2 r of a segment far from their block's start-of-tick box:
      strayed_*  move 12-13 cells in one coordinate (the wave must fall back to every segment) and land 1.1 r from a
                 segment beyond far_box + 8 d of the box -- or cross its padded twin and stop on it;
      near_*     move 5 cells and land 1.1 r from a segment between far_box and far_box + 8 d of the box."""
    rs = np.random.RandomState(303)
    rows = [strip(rs, 30, TILE, 0.15, 0.45), strip(rs, 33, TILE, 0.15, 0.45), strip(rs, 36, TILE, 0.15, 0.45)]
    rows += [strip(rs, 50 + k, TILE // 4, 0.15, 0.45) for k in range(4)]
    p = np.vstack(rows)
    v = np.zeros_like(p)
    idx = np.split(np.arange(len(p)), np.cumsum([len(r) for r in rows])[:-1])
    segs, marks = [], {"strayed_land": [], "strayed_cross": [], "near_land": []}
    i, _ = last_in_row(p, idx[0])            # 12 cells right, lands 1.1 r from the wall
    v[i] = (cells(12), 0.0)
    segs.append(fixed(((p[i, 0] + 12 * D + 1.1 * R, p[i, 1] - 3 * D), (p[i, 0] + 12 * D + 1.1 * R, p[i, 1] + 3 * D))))
    marks["strayed_land"].append(i)
    _, i = last_in_row(p, idx[1])            # 5 cells left, lands 1.1 r from the wall
    v[i] = (-cells(5), 0.0)
    segs.append(fixed(((p[i, 0] - 5 * D - 1.1 * R, p[i, 1] - 3 * D), (p[i, 0] - 5 * D - 1.1 * R, p[i, 1] + 3 * D))))
    marks["near_land"].append(i)
    i, _ = last_in_row(p, idx[2])            # 12 cells right into a wall r + 10.5 d away: stops on the padded twin
    v[i] = (cells(12), cells(0.4))
    segs.append(fixed(((p[i, 0] + R + 10.5 * D, p[i, 1] - 3 * D), (p[i, 0] + R + 10.5 * D, p[i, 1] + 3 * D))))
    marks["strayed_cross"].append(i)
    i = int(idx[5][17])                      # four strips: 13 cells down, lands 1.1 r above a horizontal wall
    v[i] = (0.0, cells(13))
    y = p[i, 1] + 13 * D + 1.1 * R
    segs.append(fixed(((p[i, 0] - 3 * D, y), (p[i, 0] + 3 * D, y))))
    marks["strayed_land"].append(i)
    i = int(idx[3][40])                      # four strips: 5 cells up, lands 1.1 r below a horizontal wall
    v[i] = (0.0, -cells(5))
    y = p[i, 1] - 5 * D - 1.1 * R
    segs.append(fixed(((p[i, 0] - 3 * D, y), (p[i, 0] + 3 * D, y))))
    marks["near_land"].append(i)
    return Case("near_next", [BOX] + segs, dict(QUIET), p, v, {k: np.array(x) for k, x in marks.items()})


# ------------------------------------------------------------------ case 4: floor_div
def floor_edges(n_lo=5, n_hi=95, d=D):
    """Coordinates at or next to k d where floor(p * (1/d)) != floor(p / d): the product alone would misplace them."""
    inv = 1.0 / d
    out = []
    for k in range(n_lo, n_hi):
        q = k * d
        for s in range(-3, 4):
            x = q
            for _ in range(abs(s)):
                x = float(np.nextafter(x, np.inf if s > 0 else -np.inf))
            if math.floor(x * inv) != math.floor(x / d):
                out.append(x)
    return np.unique(np.array(out))


def floor_case():
    """Positions whose row (y) or column (x) the product 1/d would get wrong, among ordinary ones; all at rest."""
    rs = np.random.RandomState(404)
    e = floor_edges()
    ny = np.column_stack((0.05 + rs.rand(len(e)) * 0.9, e))
    nx = np.column_stack((e, 0.05 + rs.rand(len(e)) * 0.9))
    both = np.column_stack((e, rs.permutation(e)))
    bg = 0.05 + rs.rand(600, 2) * 0.9
    p = np.vstack((ny, nx, both, bg))
    v = np.zeros_like(p)
    v[-600:] = (rs.rand(600, 2) - 0.5) * cells(0.5)
    k = len(e)
    marks = {"edge_y": np.r_[0:k, 2 * k:3 * k], "edge_x": np.r_[k:3 * k]}
    return Case("floor", [BOX], dict(QUIET), p, v, marks)


# ------------------------------------------------------------------ case 5: t_wall
T_WALL = sq_threshold(R * 1.2)
R12SQ = (R * 1.2) * (R * 1.2)


def threshold_points(segments, rs, per=8):
    """Points near 1.2 r from segments, searched on a grid of a few ulps in x and y:
      beyond a segment's end, with squared distance s == t_wall (touch; s <= fl((1.2 r)^2) would say no), s one ulp
      above it (no touch) and s == fl((1.2 r)^2) (touch either way) -- kinds 0, 1, 2;
      at a segment's interior, the nearest s at or below t_wall and the nearest above it -- kinds 3 (touch) and 4.
    (An interior point's s is a coarser lattice -- the closest point is rounded too --, it seldom lands on t_wall.)
    -> points (P, 2) and their kinds; `per` of each kind."""
    R12 = R * 1.2
    up = float(np.nextafter(T_WALL, np.inf))
    pts, kind = [], []
    got = np.zeros(5, dtype=int)
    for _ in range(20000):
        if got.min() >= per:
            break
        k = rs.randint(len(segments))
        a, b = segments[k]
        t = (b - a)
        L = math.hypot(*t)
        nrm = np.array([-t[1], t[0]]) / L
        end = got[:3].min() < per and (got[3:].min() >= per or rs.rand() < 0.5)
        if not end:                    # interior
            base = a + t * (0.2 + 0.6 * rs.rand())
            dirn = nrm * (1 if rs.rand() < 0.5 else -1)
        else:                          # beyond an end, in a random direction away from the segment
            base, away = (a, -t / L) if rs.rand() < 0.5 else (b, t / L)
            ang = (rs.rand() - 0.5) * 0.9 * math.pi
            c, s = math.cos(ang), math.sin(ang)
            dirn = np.array([c * away[0] - s * away[1], s * away[0] + c * away[1]])
        q0 = base + dirn * R12
        qx = q0[0] + np.arange(-8, 9) * np.spacing(q0[0])
        qy = q0[1] + np.arange(-8, 9) * np.spacing(q0[1])
        grid = np.stack(np.meshgrid(qx, qy), -1).reshape(-1, 2)
        others = np.delete(squared_distances(grid[:1], segments)[0], k)
        if (others < (3 * R) ** 2).any():
            continue
        s2 = squared_distances(grid, segments[k:k + 1])[:, 0]
        if end:
            cls = np.select([s2 == T_WALL, s2 == up, s2 == R12SQ], [0, 1, 2], -1)
            open_kinds = [w for w in range(3) if got[w] < per and (cls == w).any()]
            if not open_kinds:
                continue
            which = open_kinds[rs.randint(len(open_kinds))]
            q = grid[rs.choice(np.flatnonzero(cls == which))]
        else:
            which = 3 if got[3] <= got[4] else 4
            cand = np.flatnonzero(s2 <= T_WALL) if which == 3 else np.flatnonzero(s2 > T_WALL)
            if len(cand) == 0:
                continue
            q = grid[cand[np.argmax(s2[cand])]] if which == 3 else grid[cand[np.argmin(s2[cand])]]
        got[which] += 1
        pts.append(q)
        kind.append(which)
    return np.array(pts), np.array(kind)


def threshold_case(coef=None):
    """Particles whose contact with a segment (interior or end) is decided by the last ulp of the sqrt rule, moving
    slowly toward their segment (a contact turns them round), among ordinary particles."""
    rs = np.random.RandomState(505)
    walls = [fixed(((0.2, 0.2), (0.2, 0.7)), name="vertical"), fixed(((0.35, 0.8), (0.8, 0.8)), name="horizontal"),
             fixed(((0.4, 0.3), (0.75, 0.62)), name="slanted")]
    segs = np.array([w["fixed"]["segments"][0] for w in walls])
    q, kind = threshold_points(segs, rs)
    # toward the nearest segment: from q to its closest point
    k = np.argmin(squared_distances(q, segs), axis=1)
    a, b = segs[k, 0], segs[k, 1]
    t = np.clip(((q - a) * (b - a)).sum(1) / ((b - a) ** 2).sum(1), 0, 1)
    c = a + (b - a) * t[:, None]
    vq = (c - q) / np.linalg.norm(c - q, axis=1)[:, None] * cells(0.05)
    bg = 0.05 + rs.rand(500, 2) * 0.9
    d2 = squared_distances(bg, segs).min(1)
    bg = bg[d2 > (2 * R) ** 2]
    p = np.vstack((q, bg))
    v = np.vstack((vq, (rs.rand(len(bg), 2) - 0.5) * cells(0.5)))
    marks = {name: np.flatnonzero(kind == w) for w, name in enumerate(("t_wall", "above", "r12sq", "inside", "outside"))}
    return Case("threshold", [BOX] + walls, dict(coef or QUIET), p, v, marks)


# ------------------------------------------------------------------ case 6: junctions, SC_MAX_SEGMENTS / SC_MAX_BODIES
J1, J2, J3 = (0.3, 0.35), (0.62, 0.35), (0.45, 0.7)


def _off(j, dx, dy):
    return (j[0] + dx, j[1] + dy)


def junction_bodies():
    """8 bodies, 16 segments: the box and seven fans whose segments share three junction points (4, 5 and 3 segments
    meet there), two of them motored (translating and spinning about a junction)."""
    return [
        BOX,
        fixed((J1, _off(J1, 0.1, 0)), (J2, _off(J2, 0, 0.1)), name="b1"),
        fixed((J1, _off(J1, 0, 0.1)), (J2, _off(J2, -0.1, 0)), name="b2"),
        {"motored": {"name": "b3", "segments": [[[0.0, 0.0], [-0.07, 0.07]], [[J3[0] - J1[0], J3[1] - J1[1]],
                                                                             [J3[0] - J1[0] + 0.1, J3[1] - J1[1]]]],
                     "velocity_func": "lambda t: np.array([0.3 * np.cos(t * 5), -0.2])",
                     "angular_velocity_func": "lambda t: 1.0 + 0.5 * np.sin(t * 3)",
                     "scale": [1.0, 1.0], "rotation": 0.0, "position": list(J1)}},
        fixed((J1, _off(J1, 0.07, -0.07)), (J3, _off(J3, -0.1, 0)), name="b4"),
        {"motored": {"name": "b5", "segments": [[[0.0, 0.0], [0.07, 0.07]], [[0.0, 0.0], [0.07, -0.07]]],
                     "velocity_func": "lambda t: np.array([-0.25, 0.15 * np.sin(t * 4)])",
                     "angular_velocity_func": "lambda t: -3.0",
                     "scale": [1.0, 1.0], "rotation": 0.0, "position": list(J2)}},
        fixed((J2, _off(J2, 0, -0.1)), name="b6"),
        fixed((J3, _off(J3, 0, -0.1)), name="b7"),
    ]


def junction_case(coef=None, n_bg=500, seed=606):
    """Rings of particles around the three junctions (V from 0 to 5 contacts, from bodies whose slot-overwrite rule gives
    different contact velocities), particles along single segments and in the box's corners (V = 1, 2), and a
    background; forces on."""
    rs = np.random.RandomState(seed)
    ring = []
    for j in (J1, J2, J3):
        for rad in (0.5, 0.8, 1.05, 1.3, 1.6, 2.1):
            ang = rs.rand() * 2 * math.pi + np.arange(16) * (2 * math.pi / 16)
            ring.append(np.column_stack((j[0] + rad * R * np.cos(ang), j[1] + rad * R * np.sin(ang))))
    ring = np.vstack(ring)
    side = np.column_stack((0.2 + rs.rand(60) * 0.6, np.full(60, 0.9 * R)))              # along the bottom wall
    side2 = np.column_stack((np.full(60, 1 - 0.95 * R), 0.2 + rs.rand(60) * 0.6))        # along the right wall
    corner = np.array([[0.9 * R, 0.85 * R], [1 - 0.8 * R, 0.9 * R], [0.7 * R, 1 - R], [1 - R, 1 - 0.9 * R]])
    bg = 0.03 + rs.rand(n_bg, 2) * 0.94
    p = np.vstack((ring, side, side2, corner, bg))
    v = (rs.rand(len(p), 2) - 0.5) * cells(2.0)
    case = Case("junctions", junction_bodies(), dict(coef or LIVELY), p, v)
    # the hard wall fix puts a particle in a right-angled corner ON the corner's point at r from both lines: two of them
    # there would be at distance 0 from each other (NaN in the reference).  One per such point.
    from oracle.tick import hard_wall_fix, wall_contacts
    orc = case.oracle()
    for b in orc.rigid_bodies:
        b.advance(orc.coef["dt"])
    V, u, _ = wall_contacts(p, orc.segments, orc.body_states(), R)
    fx = hard_wall_fix(p, V, u, R)
    _, first = np.unique(np.round(fx / (R * 1e-3)), axis=0, return_index=True)
    keep = np.sort(first)
    case.p, case.v = p[keep], v[keep]
    case.marks = {"ring": np.flatnonzero(keep < len(ring))}
    return case


def wave_mixes(order, V):
    """Per wave of the sorted order: the set of contact counts among its lanes that touch a wall."""
    out = []
    for w0 in range(0, len(order), WAVE):
        vv = V[order[w0:w0 + WAVE]]
        out.append(set(int(x) for x in vv[vv > 0]))
    return out


def edges_case():
    """The searched positions of the threshold and floor cases in one world, forces on (tick_walls_edges)."""
    th, fl = threshold_case(LIVELY), floor_case()
    e = len(fl.p) - 600
    return Case("edges", th.bodies, dict(LIVELY), np.vstack((th.p, fl.p[:e])), np.vstack((th.v, fl.v[:e])))


CASES = {"far_box": far_box_case, "near_now": near_now_case, "near_next": near_next_case, "floor": floor_case,
         "threshold": threshold_case, "junctions": junction_case}


# ------------------------------------------------------------------ the oracle on a case
def first_tick(case, eta=None):
    """Bodies advanced once (crate.py:363-365 runs before the tick's core), then the oracle's tick core:
    -> (segments, body states, tick_core output)."""
    from oracle.tick import tick_core
    orc = case.oracle()
    for b in orc.rigid_bodies:
        b.advance(orc.coef["dt"])
    seg, st = orc.segments, orc.body_states()
    return seg, st, tick_core(case.p, case.v, seg, st, orc.coef, eta_u01=eta)


def crossed(out, segments, idx, coef):
    """The segments whose padded twins particle idx's step of this tick crosses."""
    from oracle.tick import continuous_collision_factors
    p = out["fixed_positions"][idx:idx + 1]
    v = out["v_after_bounce"][idx:idx + 1]
    return [k for k in range(len(segments))
            if continuous_collision_factors(p, v, segments[k:k + 1], coef["particle_radius"], coef["dt"])[0] < 1]


def touching(p, segments):
    """The segments within 1.2 r of each point, by the reference's sqrt rule."""
    return np.sqrt(squared_distances(p, segments)) <= R * 1.2
