"""tests/render_cases.py without a GPU: every case's claims hold on tests/render_spec.py, and every case can tell a wrong
renderer from a right one.

`draw` below is the raster rule once more with a knob on every comparison; with no knob turned it equals
render_spec.render on every case, and so it does with the box the host puts around a wall (render_prepare: the hull of
a, b and the rounded a + (b - a), widened by segment_width + 1), which therefore cuts off no pixel of any case.  Each
entry of VARIANTS turns one knob the wrong way.  CAUGHT_BY is the whole table -- which groups of cases draw a different
frame under which variant -- and test_variant_table holds the computed table to it: every variant changes a frame, every
group changes under some variant.

  variant                                   caught by
  floor_for_trunc      floor(x (W - 1))     negative, clip, view, wall_shapes (a particle or a wall's end at a coordinate
                                            below zero that is no whole number)
  trunc_for_floor      trunc of the screen  view, radii at zoom 1.2 (a screen coordinate that is negative and fractional)
                       coordinate
  disc_strict          ex^2 + ey^2 < R^2    every group with a disc (at R = 0 the centre pixel goes)
  wall_strict          4 e < w^2            wall_ties, wall_shapes, and the frames with the crate's box: far, view,
                                            frame_sizes, pressures
  radius_plus_one      R + 1                every group with a disc
  radius_minus_one     R - 1                every group with a disc of R >= 1
  clip_strict          X + R > 0 and        clip: the centres R outside an edge lose their one pixel; and wherever else
                       X - R < W - 1        a disc ends exactly on the frame's first or last column or row: radii,
                                            negative, view, frame_sizes
  lowest_id_wins       min instead of max   pressures, appended (discs of different colours overlap only there)
  box_margin_zero      the wall's box is    every group with a wall wider than a hairline
                       its hull
  all_slots_coloured   np = ns              appended alone
  no_slot_coloured     np = 0               pressures, appended
"""
import numpy as np
import pytest

import render_cases as K
import render_spec as S

GROUPS = tuple(K.GROUPS)


def draw(c, *, cell=np.trunc, pixel=np.floor, disc_strict=False, wall_strict=False, dR=0, clip_strict=False, lowest=False,
         box=None, pressure=None):
    """The frame of case `c` by render_spec's rule with these changes.  box: None for no box, or the margin as a
    function of segment_width."""
    W, H = c.width, c.height
    cx, cy = (W / 2, H / 2) if c.center is None else c.center
    xy = np.asarray(c.xy, dtype=np.float64).reshape(-1, 2)
    n = len(xy)
    if pressure is None:
        pressure = np.zeros(n) if c.pressure is None else c.pressure
    ids = np.arange(n)
    R = S.disc_radius(W, c.particle_radius, c.zoom) + dR
    keys = np.zeros(H * W, dtype=np.uint64)
    if R >= 0:
        ok = np.isfinite(xy[:, 0]) & np.isfinite(xy[:, 1])
        with np.errstate(invalid="ignore", over="ignore"):
            X = pixel((cell(xy[:, 0] * (W - 1)) - cx) * c.zoom + W / 2)
            Y = pixel((cell(xy[:, 1] * (H - 1)) - cy) * c.zoom + H / 2)
            if clip_strict:
                ok &= (X + R > 0) & (X - R < W - 1) & (Y + R > 0) & (Y - R < H - 1)
            else:
                ok &= (X + R >= 0) & (X - R <= W - 1) & (Y + R >= 0) & (Y - R <= H - 1)
        px, py = X[ok].astype(np.int64), Y[ok].astype(np.int64)
        order = (n - 1 - ids[ok]) if lowest else ids[ok]
        key = ((order + 1).astype(np.uint64) << np.uint64(8)) | S.colour(np.asarray(pressure)[ok]).astype(np.uint64)
        for ey in range(-R, R + 1):
            for ex in range(-R, R + 1):
                d2 = ex * ex + ey * ey
                if d2 >= R * R if disc_strict else d2 > R * R:
                    continue
                i, j = px + ex, py + ey
                inside = (i >= 0) & (i < W) & (j >= 0) & (j < H)
                np.maximum.at(keys, j[inside] * W + i[inside], key[inside])
    keys = keys.reshape(H, W)
    col = (keys & np.uint64(0xFF)).astype(np.uint8)
    img = np.zeros((H, W, 3), dtype=np.uint8)
    hit = keys != 0
    img[hit, 0] = col[hit]
    img[hit, 1] = col[hit]
    img[hit, 2] = 255
    # the walls
    w2 = float(c.segment_width) ** 2
    jj, ii = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    mask = np.zeros((H, W), dtype=bool)
    for (x0, y0), (x1, y1) in np.asarray(c.segments, dtype=np.float64).reshape(-1, 2, 2):
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            ax, bx = (cell(np.array([x0, x1]) * (W - 1)) - cx) * c.zoom + W / 2
            ay, by = (cell(np.array([y0, y1]) * (H - 1)) - cy) * c.zoom + H / 2
            if not np.isfinite([ax, ay, bx, by]).all():
                continue
            dx, dy = bx - ax, by - ay
            L = dx * dx + dy * dy
            t = np.zeros_like(ii) if L == 0 else np.clip(((ii - ax) * dx + (jj - ay) * dy) / L, 0.0, 1.0)
            qx, qy = ax + t * dx, ay + t * dy
            e = (ii - qx) * (ii - qx) + (jj - qy) * (jj - qy)
            covered = 4.0 * e < w2 if wall_strict else 4.0 * e <= w2
        if box is not None:  # render_prepare's box, wall_covers' first line
            m = box(c.segment_width)
            ex_, ey_ = ax + dx, ay + dy
            covered &= (ii >= min(ax, bx, ex_) - m) & (ii <= max(ax, bx, ex_) + m)
            covered &= (jj >= min(ay, by, ey_) - m) & (jj <= max(ay, by, ey_) + m)
        mask |= covered
    img[mask] = 255
    return img


def _stale(c):
    """np = ns: the slots behind the ticked ones take whatever the pressure buffer holds there -- here the first
    pressures over again."""
    if c.pressure is None:
        return None
    p = c.pressure.copy()
    p[c.ticked:] = np.resize(c.pressure[:c.ticked], len(p) - c.ticked)
    return p


VARIANTS = {
    "floor_for_trunc": lambda c: draw(c, cell=np.floor),
    "trunc_for_floor": lambda c: draw(c, pixel=np.trunc),
    "disc_strict": lambda c: draw(c, disc_strict=True),
    "wall_strict": lambda c: draw(c, wall_strict=True),
    "radius_plus_one": lambda c: draw(c, dR=1),
    "radius_minus_one": lambda c: draw(c, dR=-1),
    "clip_strict": lambda c: draw(c, clip_strict=True),
    "lowest_id_wins": lambda c: draw(c, lowest=True),
    "box_margin_zero": lambda c: draw(c, box=lambda w: 0.0),
    "all_slots_coloured": lambda c: draw(c, pressure=_stale(c)),
    "no_slot_coloured": lambda c: draw(c, pressure=np.zeros(len(c.xy))),
}

DISCS = {"radii", "clip", "negative", "far", "view", "frame_sizes", "pressures", "appended", "wall_shapes"}
CAUGHT_BY = {
    "floor_for_trunc": {"negative", "clip", "view", "wall_shapes"},
    "trunc_for_floor": {"view", "radii"},
    "disc_strict": DISCS,
    "wall_strict": {"wall_ties", "wall_shapes", "far", "view", "frame_sizes", "pressures"},
    "radius_plus_one": DISCS,
    "radius_minus_one": DISCS,
    "clip_strict": {"clip", "radii", "negative", "view", "frame_sizes"},
    "lowest_id_wins": {"pressures", "appended"},
    "box_margin_zero": {"wall_ties", "wall_shapes", "far", "view", "frame_sizes", "pressures"},
    "all_slots_coloured": {"appended"},
    "no_slot_coloured": {"pressures", "appended"},
}


@pytest.fixture(scope="module")
def frames():
    """render_spec's frame of every case, computed once."""
    out = {}
    for g in GROUPS:
        for c in K.group(g):
            img = c.spec()
            img.setflags(write=False)
            out[c.name] = img
    return out


def alone(c, k):
    """The frame of particle k of the case alone."""
    return S.render(c.xy[k:k + 1], np.zeros(1), np.array([k]), c.segments, c.width, c.height, c.particle_radius, **c.view)


# ---------------------------------------------------------------- the variant table
def test_the_rule_restated_equals_the_spec(frames):
    for g in GROUPS:
        for c in K.group(g):
            assert np.array_equal(draw(c), frames[c.name]), c.name


def test_the_walls_box_cuts_off_nothing(frames):
    """render_prepare's box (margin segment_width + 1) holds every pixel the exact test accepts; so would a margin of
    segment_width / 2 + 1, which is what the argument in csrc/sc_render.h needs."""
    for g in GROUPS:
        for c in K.group(g):
            assert np.array_equal(draw(c, box=lambda w: w + 1.0), frames[c.name]), c.name
            assert np.array_equal(draw(c, box=lambda w: w / 2 + 1.0), frames[c.name]), c.name


def test_variant_table(frames):
    table = {v: {g for g in GROUPS if any(not np.array_equal(wrong(c), frames[c.name]) for c in K.group(g))}
             for v, wrong in VARIANTS.items()}
    for v in VARIANTS:
        assert table[v], f"no case notices {v}"
    for g in GROUPS:
        assert any(g in table[v] for v in VARIANTS), f"{g} notices no variant"
    assert table == CAUGHT_BY, {v: sorted(table[v] ^ CAUGHT_BY[v]) for v in VARIANTS if table[v] != CAUGHT_BY[v]}


def test_which_frame_of_a_group_catches():
    """Inside the groups: the frames on the two sides of kRenderWaveRadius both notice R +- 1; every tie frame notices
    the strict wall test, and the frames beside a tie do not; the frames of clip notice the strict clip test."""
    for c in K.group("radii"):
        for v in ("radius_plus_one", "radius_minus_one", "disc_strict"):
            assert not np.array_equal(VARIANTS[v](c), c.spec()) or (v == "radius_minus_one" and c.R == 0), (c.name, v)
    ties = {"wall_ties_w0", "wall_ties_w2", "wall_ties_half_w1", "wall_ties_half_w3", "wall_ties_half_w5", "wall_ties_diagonal"}
    for c in K.group("wall_ties"):
        if c.name.startswith(("wall_ties_w", "wall_ties_half")):
            assert (c.name in ties) == (not np.array_equal(VARIANTS["wall_strict"](c), c.spec())), c.name
    for c in K.group("clip"):
        assert not np.array_equal(VARIANTS["clip_strict"](c), c.spec()), c.name


# ---------------------------------------------------------------- the claims, group by group
def test_radii(frames):
    cases = K.group("radii")
    assert [c.claims["R"] for c in cases] == [0, 1, 2, 3, 4, 5, 6, 4, 5]
    assert [c.claims["wave"] for c in cases] == [False] * 5 + [True, True, False, True]
    lit = [K.lit(frames[c.name]) for c in cases]
    assert lit[0] == len(np.unique(np.trunc(cases[0].xy * [K.W - 1, K.H - 1]), axis=0)) > 30  # R = 0: the centre pixels
    assert lit[:7] == sorted(lit[:7]) and len(set(lit[:7])) == 7
    for c in cases:  # a disc that lies wholly inside the frame has Gauss's count
        assert K.lit(alone(c, 0)) <= K.disc_count(c.R, 30, 20)


def test_clip(frames):
    for c in K.group("clip"):
        want = c.claims["lit"]
        X, Y = c.screen()
        assert np.array_equal(X, c.claims["X"]) and np.array_equal(Y, c.claims["Y"])
        for k in range(len(c.xy)):
            assert K.lit(alone(c, k)) == want[k], (c.name, k)
        assert K.lit(frames[c.name]) == want.sum() > 0  # the discs are disjoint


def test_negative(frames):
    c, = K.group("negative")
    assert [K.lit(alone(c, k)) for k in range(len(c.xy))] == c.claims["lit"]
    img = frames[c.name]
    assert K.lit(img) == sum(c.claims["lit"])
    assert img[5, 0].any() and img[5, 1].any() and not img[5, 2].any()  # column 0: the centre and its right neighbour
    assert img[11, 0].any() and not img[11, 1].any() and not img[23].any()  # column -1: its rim; column -2: nothing


def test_far(frames):
    c, = K.group("far")
    k = c.claims["ordinary"]
    assert np.isfinite(c.xy[k]).all() and len(k) == 10 and not np.isfinite(c.xy * 1e-290).all()
    rest = np.setdiff1d(np.arange(len(c.xy)), k)
    assert sorted(np.unique(np.abs(c.xy[rest][~np.isnan(c.xy[rest])])).tolist())[-4:] == [1e18, 1e300, 1.7e308, np.inf]
    want = S.render(c.xy[k], np.zeros(len(k)), k, c.segments, c.width, c.height, c.particle_radius, **c.view)
    assert np.array_equal(frames[c.name], want)
    none = S.render(c.xy[rest], np.zeros(len(rest)), rest, K.NO_WALLS, c.width, c.height, c.particle_radius, **c.view)
    assert not none.any()


def test_view(frames):
    a, b, z = K.group("view")
    assert (a.claims["R"], b.claims["R"], z.claims["R"]) == (3, 2, 0) and np.trunc(z.width * z.particle_radius) == 2
    assert a.claims["negative_fractional"] >= 3 and b.claims["negative_fractional"] >= 3
    for c in (a, b, z):
        img = frames[c.name]
        discs = (img[..., 2] == 255) & ~(img == 255).all(axis=2) | (img == 255).all(axis=2) & ~c.walls()
        assert discs.sum() >= 5, c.name


def test_wall_ties(frames):
    for c in K.group("wall_ties"):
        mask = frames[c.name].any(axis=2)
        assert np.array_equal(mask, c.walls())
        if "rows" in c.claims:
            assert np.flatnonzero(mask[:, c.claims["at_col"]]).tolist() == c.claims["rows"], c.name
            assert np.flatnonzero(mask[c.claims["at_row"], :]).tolist() == c.claims["cols"], c.name
        for i, j in c.claims.get("covered", ()):
            assert mask[j, i], (c.name, i, j)
        for i, j in c.claims.get("bare", ()):
            assert not mask[j, i], (c.name, i, j)
        if c.claims.get("every_row"):
            assert mask.any(axis=1).all() and not mask.all(axis=1).any()


def test_wall_shapes(frames):
    for c in K.group("wall_shapes"):
        mask = c.walls()
        assert (frames[c.name][mask] == 255).all()
        if "wall_pixels" in c.claims:
            assert mask.sum() == c.claims["wall_pixels"], c.name
        if c.claims.get("every_column"):
            assert mask.any(axis=0).all()
        if "segments" in c.claims:
            assert len(c.segments) == c.claims["segments"] == K.MAX_SEGMENTS
            each = [c.walls(s[None]) for s in c.segments]
            for k, m in enumerate(each):  # every one of the sixteen is alone on some pixels
                others = np.any([o for n, o in enumerate(each) if n != k], axis=0)
                assert (m & ~others).sum() >= 5, k
    point, far_end = K.group("wall_shapes")[0], K.group("wall_shapes")[3]
    assert np.array_equal(frames[point.name], frames[far_end.name])  # len2 = inf: t = 0, the blob of the near end


def test_frame_sizes(frames):
    cases = K.group("frame_sizes")
    assert [(c.width, c.height) for c in cases] == [(64, 48), (5, 3), (1, 1), (7, 2), (13, 1), (64, 48), (48, 64)]
    assert cases[0].width * cases[0].height == cases[6].width * cases[6].height
    for c in cases:
        assert bool(c.claims.get("black")) == (not frames[c.name].any()), c.name
    assert np.array_equal(frames["frame_1x1"], np.full((1, 1, 3), 255, dtype=np.uint8))


def test_pressures(frames):
    c, = K.group("pressures")
    xy, _, pr = K.oracle_tick()
    assert K.pressure_premises(xy, pr, np.arange(len(xy)), c) == c.claims["mixed"] >= 50
    img = frames[c.name]
    discs = (img[..., 2] == 255) & ~c.walls()
    red = img[..., 0][discs]
    assert (red == 0).sum() >= 50 and (red == 255).sum() >= 50 and ((red > 0) & (red < 255)).sum() >= 50


def test_appended(frames):
    c, = K.group("appended")
    old, new = K.appended_premises(c.xy, c.pressure, np.arange(len(c.xy)), c)
    img = frames[c.name]
    assert (img[new] == 255).all()
    before, = K.group("pressures")
    assert np.array_equal(img[old], S.render(before.xy, before.pressure, np.arange(len(before.xy)), K.NO_WALLS, c.width,
                                             c.height, c.particle_radius)[old])
    assert (img[old][:, 0] < 255).sum() >= 50
