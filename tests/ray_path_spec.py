"""The rule of the device ray paths (sc_pairs_ray_paths_device, `Crate.ray_paths`), in NumPy, by brute force, on top of
tests/ray_spec.py: a ray is followed through `bounces` specular reflections, L = bounces + 1 legs, 0 <= bounces <= 15.
Every operation below is one float64 operation, rounded on its own, as in ray_spec; the directions are never
normalised.

Leg k has an origin o, a direction d, a budget m and an excluded object x.  Leg 0 has the caller's origin and
direction, m = max_t and nothing excluded, and its hit is exactly `ray_spec.rays`'.  A leg k >= 1 is hit by the same
rule -- the smallest key (t, kind, index), walls before discs, 0 <= t <= m -- with two changes:
    * the object the leg before it hit, disc j or wall s, takes no part;
    * a disc with cc <= 0 (the origin inside or on it) is hit at t = +0 only if b < 0, the ray heading inward;
      otherwise it is not hit: the ray is leaving it.  Discs with cc > 0 follow ray_spec's formula.
A leg starts ON the thing it has just left, and that thing is named, not nudged away from: no epsilon.

A leg that hit has the point P = (fl(ox + fl(t dx)), fl(oy + fl(t dy))) and the normal n there:
    disc with centre c: g = (fl(Px - cx), fl(Py - cy)), len = sqrt(fl(fl(gx gx) + fl(gy gy))), n = (fl(gx / len), fl(gy / len));
    wall A -> B: e = B - A, len = sqrt(fl(fl(ex ex) + fl(ey ey))), n0 = (fl(ey / len), fl(-ex / len)),
                 q = fl(fl(dx n0x) + fl(dy n0y)), n = -n0 if q > 0 else n0: the normal faces the side the ray came from.
A normal with a component that is not finite (len = 0: a hit from the disc's own centre) ends the path, end = 2; the leg
is written as computed.  The next leg: dn = fl(fl(dx nx) + fl(dy ny)); dn < 0: k2 = fl(2 dn),
d' = (fl(dx - fl(k2 nx)), fl(dy - fl(k2 ny))); otherwise d' = d, the ray is leaving already.  o' = P, m' = fl(m - t),
x' = the object hit.

`end` of a ray: 0 all L legs hit something; 1 a leg met nothing within its budget (t = +inf, hit = -1, P = n = NaN);
2 leg 0 is dead (t = NaN, hit = -1), a normal is not finite, or the next leg would be dead (a number of o' or d' not
finite, a' = 0); and, only when discs are looked for, ray_spec.status's two tests on (o', d', m'): -1, a coordinate c
of o' or of fl(o' + fl(m' d')) fails fl(|c| / s) < 2^31 or that end point is not finite, before -4,
fl(8192 dt) <= t_end with dt = fl(s / sqrt(a')) and t_end = min(m', the nearest wall of the next leg, x' left out).
The tests of the next leg are made only when there is one: after leg L - 1 the path ends with 0.  Every leg after the last
one written is t = NaN, hit = -1, P = n = NaN.  Leg 0's own domain and range failures stay statuses of the call:
`status` is ray_spec's.

`walk_paths` restates every leg's search as the kernel's walk (csrc/sc_rays.h: k_ray_paths): ray_spec.walk's cells,
from step 0 and with the leg's own dt.  `wrong=` switches on one named mistake: the cases say which they catch."""
import numpy as np

import ray_spec as RS

MAX_BOUNCES = 15                      # include/sandcrate_hip.h: SC_RAY_MAX_BOUNCES
ALL_HIT, NOTHING, DEAD = 0, 1, 2      # `end`; RS.OUTSIDE and RS.RANGE are the other two
WRONG = ("no_exclusion", "leg0_inside_rule", "budget_kept", "wall_normal_unflipped", "always_reflect", "walk_not_restarted")
WAVE_STEPS = 7                        # csrc/sc_rays.h: kRayWaveSteps
NAN, INF = np.float64("nan"), np.float64("inf")

status = RS.status


def disc_t(o, d, c, rho, m, later, wrong=None):
    """t of one ray o, d (2,) with budget m against centres c (n, 2): float64 (n,), +inf where there is no hit.  `later`:
    the continuation rule of a leg >= 1.  Also -> (b, cc), for the cases that ask which branch a hit took."""
    rho2 = np.float64(rho) * np.float64(rho)
    with np.errstate(all="ignore"):
        fx, fy = o[0] - c[:, 0], o[1] - c[:, 1]
        a = d[0] * d[0] + d[1] * d[1]
        b = fx * d[0] + fy * d[1]
        cc = (fx * fx + fy * fy) - rho2
        disc = b * b - a * cc
        t = cc / (-b + np.sqrt(disc))
        inside = (b < 0) if later and wrong != "leg0_inside_rule" else True
        t = np.where(cc <= 0, np.where(inside, 0.0, INF), np.where((b < 0) & (disc >= 0), t, INF))
        ok = np.isfinite(c).all(axis=1) & (t <= m)
    return np.where(ok, t, INF), b, cc


def nearest_wall(o, d, walls, m, skip=-1):
    """(t, s) of the nearest wall of one ray, wall `skip` left out: the lowest index among equals, (+inf, -1) for none."""
    if len(walls) == 0:
        return INF, -1
    t = RS.wall_t(o[None], d[None], walls, m)[0].copy()
    if skip >= 0:
        t[skip] = INF
    s = int(t.argmin())
    return (t[s], s) if t[s] < INF else (INF, -1)


def brute(o, d, m, pts, walls, rho, skip_wall, skip_disc, later, wrong, state):
    """The hit of one leg by brute force -> (t, hit): hit j >= 0, -2 - s, or -1 with t = +inf."""
    t, s = nearest_wall(o, d, walls, m, skip_wall)
    hit = -2 - s if s >= 0 else -1
    if len(pts):
        td = disc_t(o, d, pts, rho, m, later, wrong)[0]
        if skip_disc >= 0:
            td[skip_disc] = INF
        j = int(td.argmin())
        if td[j] < t:                                                  # (a wall wins a tie)
            t, hit = td[j], j
    return t, hit


def normal(o, d, t, hit, pts, walls, wrong=None):
    """-> (P (2,), n (2,)) of a leg that hit."""
    with np.errstate(all="ignore"):
        P = np.array([o[0] + t * d[0], o[1] + t * d[1]])
        if hit >= 0:
            gx, gy = P[0] - pts[hit, 0], P[1] - pts[hit, 1]
            length = np.sqrt(gx * gx + gy * gy)
            return P, np.array([gx / length, gy / length])
        a, b = walls[-2 - hit]
        ex, ey = b[0] - a[0], b[1] - a[1]
        length = np.sqrt(ex * ex + ey * ey)
        n0 = np.array([ey / length, -ex / length])
        q = d[0] * n0[0] + d[1] * n0[1]
        return P, -n0 if q > 0 and wrong != "wall_normal_unflipped" else n0


def reflect(d, n, wrong=None):
    with np.errstate(all="ignore"):
        dn = d[0] * n[0] + d[1] * n[1]
        if not (dn < 0 or wrong == "always_reflect"):
            return d
        k2 = np.float64(2.0) * dn
        return np.array([d[0] - k2 * n[0], d[1] - k2 * n[1]])


def next_leg_end(o, d, m, walls, skip_wall, s, discs):
    """The tests of a next leg (o, d, m): DEAD, RS.OUTSIDE, RS.RANGE, or None when it may be walked."""
    if not RS.live(o, d)[0]:
        return DEAD
    if not discs:
        return None
    with np.errstate(all="ignore"):
        end = np.array([o[0] + m * d[0], o[1] + m * d[1]])
        if (~(np.abs(o) / s < RS.DOMAIN)).any() or (~(np.abs(end) / s < RS.DOMAIN)).any():     # (inf and NaN too)
            return RS.OUTSIDE
        t_end = min(m, nearest_wall(o, d, walls, m, skip_wall)[0])
        dt = s / np.sqrt(d[0] * d[0] + d[1] * d[1])
        if np.float64(RS.MAX_STEPS) * dt <= t_end:
            return RS.RANGE
    return None


def paths(points, walls, origins, directions, rho, max_t, bounces, grid_radius=None, *, wrong=None, search=brute, state=None):
    """-> (t float64 (R, L), hit int64 (R, L), P float64 (R, L, 2), n float64 (R, L, 2), end int64 (R,)).  `points` (n, 2)
    or None / rho = 0: walls only; `walls` (S, 2, 2) or None.  The caller keeps to `status` = 0."""
    assert 0 <= bounces <= MAX_BOUNCES and wrong in (None,) + WRONG
    o_all, d_all = RS._f64(origins, (2,)), RS._f64(directions, (2,))
    walls = np.zeros((0, 2, 2)) if walls is None else RS._f64(walls, (2, 2))
    discs = bool(rho)
    pts = RS._f64(points, (2,)) if points is not None and discs else np.zeros((0, 2))
    s = np.float64(2 * rho if grid_radius is None else grid_radius)
    R, L = len(o_all), bounces + 1
    t_out, hit_out = np.full((R, L), NAN), np.full((R, L), -1, dtype=np.int64)
    P_out, n_out, end_out = np.full((R, L, 2), NAN), np.full((R, L, 2), NAN), np.zeros(R, dtype=np.int64)
    alive = RS.live(o_all, d_all)
    for r in range(R):
        if not alive[r]:
            end_out[r] = DEAD
            continue
        o, d, m = o_all[r], d_all[r], np.float64(max_t)
        skip_wall = skip_disc = -1
        for k in range(L):
            t, hit = search(o, d, m, pts, walls, rho, skip_wall, skip_disc, k > 0, wrong, state)
            t_out[r, k], hit_out[r, k] = t, hit
            if hit == -1:
                end_out[r] = NOTHING
                break
            P, n = normal(o, d, t, hit, pts, walls, wrong)
            P_out[r, k], n_out[r, k] = P, n
            if not np.isfinite(n).all():
                end_out[r] = DEAD
                break
            if k == L - 1:
                break                                                  # (ALL_HIT)
            o, d = P, reflect(d, n, wrong)
            m = m if wrong == "budget_kept" else m - t
            if wrong != "no_exclusion":
                skip_wall, skip_disc = (-2 - hit, -1) if hit <= -2 else (-1, hit)
            ended = next_leg_end(o, d, m, walls, skip_wall, s, discs)
            if ended is not None:
                end_out[r] = ended
                break
    return t_out, hit_out, P_out, n_out, end_out


def walk_paths(points, walls, origins, directions, rho, max_t, bounces, grid_radius=None, *, wrong=None, batch=WAVE_STEPS):
    """`paths` with every leg searched as the kernel walks it: the walls first, their nearest t caps the walk; then
    ray_spec.walk's steps from k = 0 with dt = fl(s / sqrt(a)) of THIS leg's direction, asking the stop question after
    every `batch`-th step.  `wrong="walk_not_restarted"` carries the step counter of the leg before over."""
    s = np.float64(2 * rho if grid_radius is None else grid_radius)
    h = s * np.float64(RS.CELL_FACTOR)
    cells = {}
    if points is not None and rho:
        for j, p in enumerate(RS._f64(points, (2,))):
            if np.isfinite(p).all():
                cells.setdefault((RS.cell_of(p[0], h), RS.cell_of(p[1], h)), []).append(j)
    state = dict(k=0)

    def search(o, d, m, pts, walls_, rho_, skip_wall, skip_disc, later, wrong_, state_):
        t, sw = nearest_wall(o, d, walls_, m, skip_wall)
        hit = -2 - sw if sw >= 0 else -1
        if not len(pts):
            return t, hit
        t_end = min(m, t)
        dt = s / np.sqrt(d[0] * d[0] + d[1] * d[1])
        best, who = INF, -1
        k = state_["k"] if later and wrong_ == "walk_not_restarted" else 0
        while np.float64(k) * dt <= t_end:
            assert k < RS.MAX_STEPS
            tm = np.float64(k + 0.5) * dt
            cx, cy = RS.cell_of(o[0] + tm * d[0], h), RS.cell_of(o[1] + tm * d[1], h)
            met = [j for iy in (-1, 0, 1) for ix in (-1, 0, 1) for j in cells.get((cx + ix, cy + iy), ()) if j != skip_disc]
            if met:
                td = disc_t(o, d, pts[met], rho_, m, later, wrong_)[0]
                for j, tj in zip(met, td):
                    if tj < best or (tj == best and tj < INF and j < who):
                        best, who = tj, j
            if (k + 1) % batch == 0 and best < np.float64(k + 1) * dt:
                break
            k += 1
        state_["k"] = k
        return (best, who) if best < t else (t, hit)

    return paths(points, walls, origins, directions, rho, max_t, bounces, grid_radius, wrong=wrong, search=search, state=state)


def branches(points, origins, directions, rho, max_t, result):
    """Of every leg >= 1 of `result` = paths(...) without walls' help: the discs j with cc <= 0 at the leg's origin, as
    {(r, k): [(j, b < 0)]} -- which of the two continuation branches the rule took there, hit or left alone."""
    pts = RS._f64(points, (2,))
    t, hit, P, n, end = result
    d_all = RS._f64(directions, (2,))
    found = {}
    for r in range(len(t)):
        d, m = d_all[r], np.float64(max_t)
        for k in range(1, t.shape[1]):
            if hit[r, k - 1] == -1 or not np.isfinite(n[r, k - 1]).all() or np.isnan(t[r, k]):
                break
            d, m = reflect(d, n[r, k - 1]), m - t[r, k - 1]
            _, b, cc = disc_t(P[r, k - 1], d, pts, rho, m, True)
            took = [(int(j), bool(b[j] < 0)) for j in np.nonzero(cc <= 0)[0] if j != hit[r, k - 1]]
            if took:
                found[(r, k)] = took
    return found
