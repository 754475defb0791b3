"""The rule of the device ray sensors (sc_pairs_rays_device, `Crate.ray_tensors`), in NumPy, by brute force: every ray
against every disc and every wall.  Every operation below is one float64 NumPy operation, rounded on its own -- the
library is built with -ffp-contract=off and evaluates the same expressions in the same order.

A ray is an origin o and a direction d, which nobody normalises: the parameter t is in units of |d|.  `max_t` is a finite
float >= 0, `rho` the disc radius, rho2 = fl(rho rho) squared once.

Disc j with a finite centre c:
    fx = ox - cx, fy = oy - cy
    a  = fl(fl(dx dx) + fl(dy dy))
    b  = fl(fl(fx dx) + fl(fy dy))
    cc = fl(fl(fl(fx fx) + fl(fy fy)) - rho2)
    cc <= 0: the origin is inside or on the disc, t = +0.0; otherwise b >= 0: no hit; otherwise
    disc = fl(fl(b b) - fl(a cc)), disc < 0: no hit; otherwise q = fl(-b + sqrt(disc)), t = fl(cc / q)
    (no cancellation: -b > 0); a hit iff t <= max_t.
Wall s from A to B, e = B - A, g = A - o:
    den = fl(fl(dx ey) - fl(dy ex)), den == 0: no hit (parallel and collinear rays miss)
    t = fl(fl(fl(gx ey) - fl(gy ex)) / den), u = fl(fl(fl(gx dy) - fl(gy dx)) / den)
    a hit iff 0 <= t <= max_t and 0 <= u <= 1, from either face; a t of -0.0 is +0.0.
The result of a ray is the hit with the smallest key (t, kind, index), kind 0 for walls and 1 for discs: `hit` = j >= 0
for disc j, -2 - s for wall s, -1 for none with t = +inf.  A ray whose origin or direction is not finite, or whose a is
0, is dead: t = NaN, hit = -1.  A disc whose centre is not finite is never hit.

`status` is what the call reports instead when it refuses (counts[1]; nothing else is written then): -1, the domain --
with s the grid's radius (2 rho unless given) a finite coordinate c of a point, of an origin or, when discs are looked
for, of a live ray's end point fl(o + fl(max_t d)) needs fl(|c| / s) < 2^31, and such an end point must be finite --,
and -4, the range: a live ray that looks for discs walks the grid in steps of dt = fl(s / sqrt(a)) up to
t_end = min(max_t, its nearest wall hit), and needs fl(MAX_STEPS dt) > t_end.  `walk` restates that walk: what the kernel
does instead of the brute force, and what it must not do."""
import numpy as np

MAX_STEPS = 8192                      # csrc/sc_rays.h: kRayMaxSteps
CELL_FACTOR = 1.0 + 2.0 ** -20        # csrc/sc_pairs.h: kPairsCellFactor
DOMAIN = 2.0 ** 31
RANGE, OUTSIDE = -4, -1               # counts[1]: sand_crate_amd/_native.py PAIRS_RANGE, PAIRS_DOMAIN
CHUNK = 1 << 22                       # ray-disc tests of one broadcast


def _f64(a, tail):
    return np.array(a, dtype=np.float64).reshape((-1,) + tail)


def live(origins, directions):
    """Which rays are alive: all four numbers finite and a != 0."""
    o, d = _f64(origins, (2,)), _f64(directions, (2,))
    with np.errstate(all="ignore"):
        a = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
    return np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (a != 0)


def disc_t(o, d, c, rho, max_t):
    """t of rays o, d (R, 2) against centres c (n, 2): float64 (R, n), +inf where there is no hit."""
    rho2 = np.float64(rho) * np.float64(rho)
    with np.errstate(all="ignore"):
        fx = o[:, None, 0] - c[None, :, 0]
        fy = o[:, None, 1] - c[None, :, 1]
        dx, dy = d[:, None, 0], d[:, None, 1]
        a = dx * dx + dy * dy
        b = fx * dx + fy * dy
        cc = (fx * fx + fy * fy) - rho2
        disc = b * b - a * cc
        q = -b + np.sqrt(disc)
        t = cc / q
        t = np.where(cc <= 0, 0.0, np.where((b < 0) & (disc >= 0), t, np.inf))
        ok = np.isfinite(c).all(axis=1)[None, :] & (t <= np.float64(max_t))
    return np.where(ok, t, np.inf)


def wall_t(o, d, walls, max_t):
    """t of rays o, d (R, 2) against walls (S, 2, 2): float64 (R, S), +inf where there is no hit."""
    with np.errstate(all="ignore"):
        ax, ay = walls[None, :, 0, 0], walls[None, :, 0, 1]
        ex, ey = walls[None, :, 1, 0] - ax, walls[None, :, 1, 1] - ay
        gx, gy = ax - o[:, None, 0], ay - o[:, None, 1]
        dx, dy = d[:, None, 0], d[:, None, 1]
        den = dx * ey - dy * ex
        t = (gx * ey - gy * ex) / den
        u = (gx * dy - gy * dx) / den
        ok = (den != 0) & (t >= 0) & (t <= np.float64(max_t)) & (u >= 0) & (u <= 1)
    return np.where(ok, t + 0.0, np.inf)                               # (-0.0 + 0.0 is +0.0)


def nearest_wall(o, d, walls, max_t):
    """-> (t (R,), s (R,)): every ray's nearest wall hit, the lowest index among equals; (+inf, -1) for none."""
    if len(walls) == 0:
        return np.full(len(o), np.inf), np.full(len(o), -1, dtype=np.int64)
    t = wall_t(o, d, walls, max_t)
    s = t.argmin(axis=1)                                               # (the first of equals)
    best = t[np.arange(len(o)), s]
    return best, np.where(best < np.inf, s, -1).astype(np.int64)


def rays(points, walls, origins, directions, rho, max_t):
    """-> (t float64 (R,), hit int64 (R,)).  `points` (n, 2) or None / rho = 0: walls only; `walls` (S, 2, 2) or None."""
    o, d = _f64(origins, (2,)), _f64(directions, (2,))
    walls = np.zeros((0, 2, 2)) if walls is None else _f64(walls, (2, 2))
    pts = np.zeros((0, 2)) if points is None or not rho else _f64(points, (2,))
    n_rays = len(o)
    t, s = nearest_wall(o, d, walls, max_t)
    hit = np.where(s >= 0, -2 - s, -1).astype(np.int64)
    if len(pts):
        step = max(1, CHUNK // len(pts))
        for lo in range(0, n_rays, step):
            rows = slice(lo, lo + step)
            td = disc_t(o[rows], d[rows], pts, rho, max_t)
            j = td.argmin(axis=1)                                      # (the lowest index among equals)
            tj = td[np.arange(len(j)), j]
            wins = tj < t[rows]                                        # (a wall wins a tie)
            t[rows] = np.where(wins, tj, t[rows])
            hit[rows] = np.where(wins, j, hit[rows])
    dead = ~live(o, d)
    t[dead] = np.nan
    hit[dead] = -1
    return t, hit


def outside(c, s):
    """pairs_outside of csrc/sc_pairs.h for coordinates c: finite, and fl(|c| / s) not below 2^31."""
    c = np.abs(np.asarray(c, dtype=np.float64))
    with np.errstate(all="ignore"):
        return (c < np.inf) & ~(c / np.float64(s) < DOMAIN)


def status(points, walls, origins, directions, rho, max_t, grid_radius=None):
    """0, or what the call reports instead of results: -1 (the domain) before -4 (the range)."""
    o, d = _f64(origins, (2,)), _f64(directions, (2,))
    walls = np.zeros((0, 2, 2)) if walls is None else _f64(walls, (2, 2))
    s = np.float64(2 * rho if grid_radius is None else grid_radius)
    discs = bool(rho)
    bad = outside(o, s).any()
    if points is not None:
        bad |= outside(_f64(points, (2,)), s).any()
    alive = live(o, d)
    if discs and alive.any():
        o, d = o[alive], d[alive]
        with np.errstate(all="ignore"):
            end = o + np.float64(max_t) * d
            bad |= (outside(end, s) | ~np.isfinite(end)).any()
    if bad:
        return OUTSIDE
    if discs and alive.any():
        t_end = np.minimum(np.float64(max_t), nearest_wall(o, d, walls, max_t)[0])
        with np.errstate(all="ignore"):
            dt = s / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
            if (np.float64(MAX_STEPS) * dt <= t_end).any():
                return RANGE
    return 0


def steps(origin, direction, walls, rho, max_t, grid_radius=None):
    """The steps the walk of one live ray through EMPTY space takes: the k with fl(k dt) <= t_end."""
    o, d = _f64(origin, (2,)), _f64(direction, (2,))
    walls = np.zeros((0, 2, 2)) if walls is None else _f64(walls, (2, 2))
    s = np.float64(2 * rho if grid_radius is None else grid_radius)
    t_end = min(np.float64(max_t), nearest_wall(o, d, walls, max_t)[0][0])
    dt = s / np.sqrt(d[0, 0] * d[0, 0] + d[0, 1] * d[0, 1])
    k = 0
    while np.float64(k) * dt <= t_end:
        k += 1
    return k


def cell_of(c, h):
    with np.errstate(all="ignore"):
        return int(np.floor(np.float64(c) / h))


def walk(points, walls, origins, directions, rho, max_t, grid_radius=None, *, block=3, stop="rule", batch=1):
    """The kernel's walk (csrc/sc_rays.h), a ray and a step at a time: the walls first, their nearest t caps the walk;
    step k covers t in [fl(k dt), fl((k + 1) dt)], dt = fl(s / sqrt(a)), and looks at the `block` x `block` cells
    round the cell of its midpoint fl(o + fl(fl((k + 0.5) dt) d)), cells of width h = fl(s (1 + 2^-20)); every member
    of those cells is tested by the rule above and the smallest key (t, j) kept; the walk ends after the first step with
    best t < fl((k + 1) dt) -- `stop="rule"` --, or when fl(k dt) > t_end.  -> (t, hit) as `rays`.
    `batch` = B asks that question only after every B-th step: the kernel's wave takes B = 7 steps at a time.
    `block=1` and `stop="first_hit"` (ends after the first step that has met any disc) are two wrong walks: the cases say
    which of them they catch.  The caller keeps to `status` = 0."""
    o, d = _f64(origins, (2,)), _f64(directions, (2,))
    walls = np.zeros((0, 2, 2)) if walls is None else _f64(walls, (2, 2))
    pts = np.zeros((0, 2)) if points is None or not rho else _f64(points, (2,))
    s = np.float64(2 * rho if grid_radius is None else grid_radius)
    h = s * np.float64(CELL_FACTOR)
    cells = {}
    for j, p in enumerate(pts):
        if np.isfinite(p).all():
            cells.setdefault((cell_of(p[0], h), cell_of(p[1], h)), []).append(j)
    t_out, s_out = nearest_wall(o, d, walls, max_t)
    hit_out = np.where(s_out >= 0, -2 - s_out, -1).astype(np.int64)
    alive = live(o, d)
    reach = range(-(block // 2), block // 2 + 1)
    for r in range(len(o)):
        if not alive[r]:
            t_out[r], hit_out[r] = np.nan, -1
            continue
        if not len(pts):
            continue
        t_end = min(np.float64(max_t), t_out[r])
        dt = s / np.sqrt(d[r, 0] * d[r, 0] + d[r, 1] * d[r, 1])
        best, who = np.inf, -1
        k = 0
        while np.float64(k) * dt <= t_end:
            assert k < MAX_STEPS
            tm = np.float64(k + 0.5) * dt
            cx, cy = cell_of(o[r, 0] + tm * d[r, 0], h), cell_of(o[r, 1] + tm * d[r, 1], h)
            met = [j for iy in reach for ix in reach for j in cells.get((cx + ix, cy + iy), ())]
            if met:
                td = disc_t(o[r:r + 1], d[r:r + 1], pts[met], rho, max_t)[0]
                for j, t in zip(met, td):
                    if t < best or (t == best and t < np.inf and j < who):
                        best, who = t, j
            if (k + 1) % batch == 0 and (best < np.float64(k + 1) * dt or (stop == "first_hit" and who >= 0)):
                break
            k += 1
        if best < t_out[r]:
            t_out[r], hit_out[r] = best, who
    return t_out, hit_out
