"""The worlds of tests/wall_cases.py still mean what they claim (CPU only): the searched positions really sit on the
edges of floor(p * (1/d)) and of the sqrt rule, the fast particles really cross, and each segment a near-mask case is
about lies in the band of its block's box that the mask's argument is tight for.  tests/test_gpu_walls.py asserts the
same premises on the oracle's output before it compares the device with it; these keep a case from drifting into
testing nothing without a GPU to notice."""
import math

import numpy as np
import pytest

import wall_cases as wc
from oracle.neighbors import strip_sort

D, R = wc.D, wc.R
REACH_NOW = wc.FAR_BOX + (wc.NEAR_STEPS - 2) * D    # near_now's radius around the box (k_pass_b)
REACH_NEXT = wc.FAR_BOX + wc.NEAR_STEPS * D         # near_next's


def step_len(out, i, dt):
    return math.hypot(*(out["v_after_bounce"][i] * dt))


def far_from_all(p, segments, radius):
    """K1's `far`: every segment's bounding box is more than `radius` away in x or in y."""
    lo, hi = segments.min(1), segments.max(1)
    gap = np.maximum(np.maximum(lo - p, p - hi), 0.0)
    return bool(((gap[:, 0] > radius) | (gap[:, 1] > radius)).all())


def test_the_diameter_separates_the_sqrt_rule_from_the_rounded_square():
    assert wc.T_WALL > wc.R12SQ
    assert math.sqrt(wc.T_WALL) <= R * 1.2 < math.sqrt(float(np.nextafter(wc.T_WALL, np.inf)))


def test_far_box_case():
    case = wc.far_box_case()
    seg, _, out = wc.first_tick(case)
    dt = case.coef["dt"]
    fac, fx = out["ccd_factor"], out["fixed_positions"]
    assert len(case.marks["beyond_cross"]) >= 8 and len(case.marks["inside_cross"]) >= 8
    for i in case.marks["beyond_cross"]:            # far, a step over 2d but under 3d, and a crossing
        assert far_from_all(fx[i], seg, wc.FAR_BOX * (1 + 1e-5))
        assert 2 * D * 1.01 < step_len(out, i, dt) < 3 * D * 0.99 and fac[i] < 0.99
    for i in case.marks["beyond_short"]:            # far, just under 2d: cannot reach the padded segment
        assert far_from_all(fx[i], seg, wc.FAR_BOX * (1 + 1e-5))
        assert 1.8 * D < step_len(out, i, dt) < 2 * D * 0.99 and fac[i] == 1.0
    for i in case.marks["inside_cross"]:            # within far_box but beyond r + d; a step under 2d that crosses
        assert not far_from_all(fx[i], seg, wc.FAR_BOX * (1 - 1e-5))
        assert far_from_all(fx[i], seg, (R + D) * (1 + 1e-5))
        assert step_len(out, i, dt) < 2 * D * 0.99 and fac[i] < 0.99
    assert (out["wall_count"] == 0).all()


def test_near_now_case():
    case = wc.near_now_case()
    seg, _, out = wc.first_tick(case)
    dt = case.coef["dt"]
    fx = out["fixed_positions"]
    assert np.array_equal(fx, case.p)               # nobody touches a wall: the blocks are the ones built
    order, rows, boxes = wc.block_boxes(fx)
    steps = np.hypot(*(out["v_after_bounce"] * dt).T)
    kinds = set()
    for name in ("band_strip", "band_multi", "band_pile", "fallback_strip", "fallback_multi", "fallback_pile"):
        for i in case.marks[name]:
            b = wc.block_of(order, i)
            box = boxes[b]
            kinds.add((name.split("_")[0], box[4]))
            hit = wc.crossed(out, seg, i, case.coef)
            assert len(hit) == 1 and out["ccd_factor"][i] < 0.99, name
            gap = max(wc.box_gap(box, seg[hit[0]]))
            pos = int(np.flatnonzero(order == i)[0])
            wave = order[pos - pos % wc.WAVE:][:wc.WAVE]
            assert (steps[wave] < 8 * D * 0.99).sum() == len(wave) - (name.startswith("fallback"))
            if name.startswith("band"):             # 6-8 cells, a segment in (far_box + 5d, far_box + 6d] of the box
                assert 6 * D < steps[i] < 8 * D * 0.99
                assert REACH_NOW - D + 0.1 * D < gap <= REACH_NOW - 0.1 * D, (name, gap / D)
            else:                                   # 9-15 cells, a segment far outside near_now
                assert 9 * D < steps[i] < 15 * D and gap > REACH_NOW + 0.2 * D, (name, gap / D)
            if name == "band_multi":                # near only through the box's +d in y
                assert not box[4]
                no_pad = (box[0], box[1], box[2] + D, box[3] - D)
                assert max(wc.box_gap(no_pad, seg[hit[0]])) > REACH_NOW + 0.1 * D
            if name.endswith("pile"):               # the block's tile cannot be held in LDS
                x0, x1 = box[0], box[1]
                near_rows = np.abs(rows - rows[pos]) <= 1
                xs = fx[order][near_rows, 0]
                assert box[4] and ((xs >= x0 - D) & (xs <= x1 + D)).sum() > wc.TILE_CAP_B
    assert kinds == {("band", True), ("band", False), ("fallback", True), ("fallback", False)}


def test_near_next_case():
    from oracle.tick import tick_core
    case = wc.near_next_case()
    seg, st, out = wc.first_tick(case)
    fx = out["fixed_positions"]
    order, rows, boxes = wc.block_boxes(fx)
    out2 = tick_core(out["particles"], out["velocities"], seg, st, case.coef)   # fixed bodies: the same walls
    moved = np.abs(out["particles"] - fx).max(1)
    for name in ("strayed_land", "strayed_cross", "near_land"):
        for i in case.marks[name]:
            assert out2["wall_count"][i] == 1, name
            k = int(np.flatnonzero(wc.touching(out["particles"][i:i + 1], seg)[0])[0])
            gap = max(wc.box_gap(boxes[wc.block_of(order, i)], seg[k]))
            if name.startswith("strayed"):          # more than 8 cells in a coordinate; a segment beyond near_next
                assert moved[i] > 8 * D * 1.01 and gap > REACH_NEXT + 0.2 * D, (name, gap / D)
            else:                                   # fewer; a segment beyond far_box but inside near_next
                assert moved[i] < 8 * D and wc.FAR_BOX + 0.5 * D < gap < REACH_NEXT, (name, gap / D)
            assert (out["ccd_factor"][i] < 1) == (name == "strayed_cross")
    assert (out["wall_count"] == 0).all()
    assert {wc.block_boxes(fx)[2][wc.block_of(order, i)][4] for i in case.marks["strayed_land"]} == {True, False}


def test_floor_case():
    case = wc.floor_case()
    inv = 1.0 / D
    e = wc.floor_edges()
    assert len(e) >= 10
    assert all(math.floor(x * inv) != math.floor(x / D) for x in e)
    _, _, out = wc.first_tick(case)
    fx = out["fixed_positions"]
    assert np.array_equal(fx, case.p)
    for axis, name in ((1, "edge_y"), (0, "edge_x")):
        c = fx[case.marks[name], axis]
        assert (np.floor(c * inv) != np.floor(c / D)).all()
    rows, order = strip_sort(fx, D)
    assert np.array_equal(rows, np.floor(fx[order, 1] / D).astype(np.int64))
    assert not np.array_equal(rows, np.floor(fx[order, 1] * inv).astype(np.int64))


def test_threshold_case():
    case = wc.threshold_case()
    seg, _, out = wc.first_tick(case)
    V = out["wall_count"]
    q = case.p
    d2 = wc.squared_distances(q, seg)
    s = d2.min(1)
    near = np.argmin(d2, axis=1)
    a, b = seg[near, 0], seg[near, 1]
    tt = ((q - a) * (b - a)).sum(1) / ((b - a) ** 2).sum(1)
    for name, touch, end in (("t_wall", True, True), ("above", False, True), ("r12sq", True, True),
                             ("inside", True, False), ("outside", False, False)):
        idx = case.marks[name]
        assert len(idx) >= 8, name
        assert ((V[idx] == 1) if touch else (V[idx] == 0)).all(), name
        assert (((tt[idx] <= 0) | (tt[idx] >= 1)) == end).all(), name
        assert (np.abs(s[idx] - wc.T_WALL) < 400 * np.spacing(wc.T_WALL)).all(), name
    t = case.marks["t_wall"]
    assert (s[t] == wc.T_WALL).all() and (s[t] > wc.R12SQ).all()        # the rounded square would say no
    assert (s[case.marks["above"]] == np.nextafter(wc.T_WALL, 1)).all()
    assert np.array_equal(out["fixed_positions"], case.p)
    assert (out["v_after_bounce"][t] != out["v_after_viscosity"][t]).all(axis=1).any()   # a contact turns them round


def test_junction_case():
    case = wc.junction_case()
    seg, st, out = wc.first_tick(case)
    assert len(seg) == 16 and len(st) == 8
    V = out["wall_count"]
    assert {1, 2, 3, 4, 5} <= set(V.tolist())
    # the slot-overwrite rule gives different contact velocities across a particle's slots
    many = np.flatnonzero(V >= 3)
    wv = out["wall_vel"]
    assert any(len({tuple(wv[i, q]) for q in range(V[i])}) >= 2 for i in many)
    rows, order = strip_sort(out["fixed_positions"], D)
    mixes = wc.wave_mixes(order, V)
    assert any(m and m <= {1, 2, 4} and m & {2, 4} for m in mixes)          # all lanes on the 1/V fast path
    assert any(m & {1, 2, 4} and m & {3, 5} for m in mixes)                # fast and slow lanes in one wave
    assert any(m == {1} for m in mixes)                                    # one contact per lane
    assert any(1 in m and m & {2, 3, 4, 5} for m in mixes)                 # ... mixed with corners
    # three ticks without a particle at distance 0 from a wall or from another particle (NaN in the reference)
    from oracle.tick import tick_core
    orc = case.oracle()
    p, v = case.p, case.v
    for _ in range(3):
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        o = tick_core(p, v, orc.segments, orc.body_states(), orc.coef)
        assert not np.isnan(o["particles"]).any()
        p, v = o["particles"], o["velocities"]
