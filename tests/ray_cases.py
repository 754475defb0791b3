"""The named inputs of the ray sensors' tests: name -> Case(points (n, 2), walls (S, 2, 2), origins (R, 2), directions
(R, 2), rho, max_t, radius, claims).  Worlds of tens of points at the places where the kernel can go wrong.  `radius` is
the radius of the count whose grid the rays walk, None for 2 rho -- what `Crate.ray_tensors` counts at; a case with a
radius of its own runs through `Engine.pairs_rays` only.  `claims` says what the world is there for, in terms
tests/test_ray_cases_cpu.py proves from tests/ray_spec.py; tests/test_gpu_rays.py runs each on the device against the
spec.  The kinds of claim:

    "hit"             {r: hit}: the result of ray r, worked out by hand
    "t"               {r: t}: ... and its t, exactly
    "side"            {r: (ix, iy)}: the disc ray r hits has its centre in the cell (ix, iy) away from the cell of the
                      midpoint of the step that holds the hit -- a neighbour, never (0, 0)
    "grazed"          {r: (lo, hi)}: the distance of that centre from the ray, as a fraction of rho
    "disc_sign"       {(r, j): -1, 0 or 1}: the sign of the rule's `disc` for ray r and point j (0: EXACTLY zero)
    "rim"             [(r, j)]: the rule's cc is exactly zero: the origin lies on the rim
    "tie"             [(r, (kind, index), (kind, index))]: two candidates of ray r have the same t, bit for bit (kind 0:
                      wall, 1: disc); the first one wins
    "steps"           {r: k}: the steps the walk of ray r takes
    "status"          what the call reports instead of results (ray_spec.status); 0 when absent
    "block_1_fails"   the walk with a 1 x 1 block instead of 3 x 3 gets this case wrong
    "first_hit_fails" (B, ...): the walk that ends as soon as it has met any disc -- asking after every B-th step, as
                      `ray_spec.walk(stop="first_hit", batch=B)` does -- gets this case wrong, for each B listed; the
                      kernel's wave asks after every N.RAY_WAVE_STEPS-th
    "met_in_steps"    {j: k}: step k is the first whose 3 x 3 block holds the cell of point j (ray 0)
    "shared_bucket"   ((cx, cy), (cx, cy)): two occupied cells, far apart, that lie in one bucket of the count's table
    "negative_cells"  some point's cell index is negative in x and in y
"""
import collections
import functools

import numpy as np

from sand_crate_amd import _native as N

Case = collections.namedtuple("Case", "points walls origins directions rho max_t radius claims")

RHO = 0.25                                                         # every coordinate below is chosen for this radius:
S = 2 * RHO                                                        # the count's radius, and
H = S * N.PAIRS_CELL_FACTOR                                        # the cell's width
RAYS = (0, 1, 63, 64, 65, 129)                                     # none, one, and around 64 and 128
NAN, INF = float("nan"), float("inf")
NO_WALLS = np.zeros((0, 2, 2))
BOX = np.array([[[-1.0, -1.0], [5.0, -1.0]], [[5.0, -1.0], [5.0, 4.0]], [[5.0, 4.0], [-1.0, 4.0]], [[-1.0, 4.0], [-1.0, -1.0]]])
SIDES = {"N": (0, 1), "W": (-1, 0), "S": (0, -1), "E": (1, 0), "NE": (1, 1), "NW": (-1, 1), "SW": (-1, -1), "SE": (1, -1)}
assert N.RAY_BLOCK == 64 and N.RAY_MAX_STEPS == 8192 and N.PAIRS_MIN_BUCKETS == 256


def arr(a, tail):
    out = np.array(a, dtype=np.float64).reshape((-1,) + tail)
    out.setflags(write=False)
    return out


def case(points, walls, origins, directions, max_t, claims, rho=RHO, radius=None):
    return Case(arr(points, (2,)), arr(walls, (2, 2)), arr(origins, (2,)), arr(directions, (2,)), float(rho), float(max_t),
                radius, claims)


def turn(p, quarter_turns):
    """(x, y) -> (-y, x), `quarter_turns` times: the grid's cells go to cells."""
    p = np.array(p, dtype=np.float64)
    for _ in range(quarter_turns % 4):
        p = np.stack([-p[..., 1], p[..., 0]], axis=-1)
    return p


def cloud(seed, n, lo=(-0.5, -0.5), hi=(4.5, 3.5)):
    rs = np.random.RandomState(seed)
    return np.array(lo) + rs.rand(n, 2) * (np.array(hi) - np.array(lo))


def fan(seed, n, lo=(-0.5, -0.5), hi=(4.5, 3.5)):
    """n rays from random places inside the box in random directions, of lengths between 0.5 and 1.5."""
    rs = np.random.RandomState(seed)
    angle = rs.rand(n) * 2 * np.pi
    length = 0.5 + rs.rand(n)
    return cloud(seed + 1, n, lo, hi), np.stack([np.cos(angle), np.sin(angle)], axis=1) * length[:, None]


def shared_bucket_pair():
    """A cell (1, iy), iy in -1 .. 1 -- in the block of step 0 of a ray that starts in cell (0, 0) -- and a cell
    (ix, 0), 12 <= ix < 400, further along that ray, that lie in one bucket of a 256-bucket table: the first found."""
    for ix in range(12, 400):
        for iy in (-1, 0, 1):
            if N.pairs_bucket(1, iy, 256) == N.pairs_bucket(ix, 0, 256):
                return (1, iy), (ix, 0)
    raise AssertionError("no collision below 400 cells")


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    # -- the superset property: a grazed disc whose centre lies in a neighbour of the midpoint's cell, on each side.
    # Along +x at y = 0.3 from x = 0.05: an edge neighbour, centre (1.3, 0.5499) in cell (2, 1), hit in step 2 (midpoint
    # x = 1.3, cell (2, 0)); a corner neighbour, centre (0.51, 0.5499) in cell (1, 1), hit at t = 0.453 in step 0
    # (midpoint x = 0.3, cell (0, 0)).  Quarter turns give the other six.
    for name, (centre, quarter) in {"N": ((1.3, 0.5499), 0), "W": ((1.3, 0.5499), 1), "S": ((1.3, 0.5499), 2),
                                    "E": ((1.3, 0.5499), 3), "NE": ((0.51, 0.5499), 0), "NW": ((0.51, 0.5499), 1),
                                    "SW": ((0.51, 0.5499), 2), "SE": ((0.51, 0.5499), 3)}.items():
        out[f"grazed_{name}"] = case([turn(centre, quarter)], NO_WALLS, [turn((0.05, 0.3), quarter)], [turn((1.0, 0.0), quarter)],
                                     3.0, dict(hit={0: 0}, side={0: SIDES[name]}, grazed={0: (0.99, 1.0)}, block_1_fails=True))
    # -- a tangent ray: disc exactly 0, and the centre one ulp further from the ray and one ulp nearer
    for name, y, sign in (("at", 0.25, 0), ("outside", np.nextafter(0.25, 1.0), -1), ("inside", np.nextafter(0.25, 0.0), 1)):
        out[f"tangent_{name}"] = case([(0.25, y)], NO_WALLS, [(0.0, 0.0)], [(1.0, 0.0)], 2.0,
                                      dict(disc_sign={(0, 0): sign}, hit={0: -1 if sign < 0 else 0}))
    # -- the origin inside a disc, exactly on its rim, a disc behind it; a nearer disc of higher index behind the inside one
    out["origin_inside"] = case([(1.0, 0.0), (0.1, 0.05), (0.05, -0.1)], NO_WALLS, [(0.0, 0.0), (0.0, 0.0)], [(1.0, 0.0), (-1.0, 0.0)], 3.0,
                                dict(hit={0: 1, 1: 1}, t={0: 0.0, 1: 0.0}, tie=[(0, (1, 1), (1, 2))]))
    out["origin_on_rim"] = case([(0.25, 0.0)], NO_WALLS, [(0.0, 0.0), (0.0, 0.0), (0.5, 0.0)], [(1.0, 0.0), (-1.0, 0.0), (1.0, 0.0)], 3.0,
                                dict(rim=[(0, 0), (1, 0), (2, 0)], hit={0: 0, 1: 0, 2: 0}, t={0: 0.0, 1: 0.0, 2: 0.0}))
    out["disc_behind"] = case([(-1.0, 0.0)], NO_WALLS, [(0.0, 0.0), (0.0, 0.0)], [(1.0, 0.0), (-1.0, 0.0)], 3.0,
                              dict(hit={0: -1, 1: 0}, t={0: INF, 1: 0.75}))
    # -- max_t: a disc and a wall at t = 0.75 exactly, with max_t at it, one ulp below, and 0
    disc, wall = [(1.0, 0.0)], [[(0.75, -1.0), (0.75, 1.0)]]
    rays_o, rays_d = [(0.0, 0.0), (0.0, 2.0)], [(1.0, 0.0), (1.0, 0.0)]            # ray 0 meets both, ray 1 passes above
    below = np.nextafter(0.75, 0.0)
    out["max_t_at_disc"] = case(disc, NO_WALLS, rays_o, rays_d, 0.75, dict(hit={0: 0, 1: -1}, t={0: 0.75}))
    out["max_t_below_disc"] = case(disc, NO_WALLS, rays_o, rays_d, below, dict(hit={0: -1, 1: -1}))
    out["max_t_at_wall"] = case([], wall, rays_o, rays_d, 0.75, dict(hit={0: -2, 1: -1}, t={0: 0.75}))
    out["max_t_below_wall"] = case([], wall, rays_o, rays_d, below, dict(hit={0: -1, 1: -1}))
    out["max_t_zero"] = case([(0.1, 0.0), (1.0, 0.0)], [[(0.0, -1.0), (0.0, 1.0)], [(0.5, -1.0), (0.5, 1.0)]],
                             [(0.0, 0.0), (0.0, 0.5), (-0.2, 0.0)], [(1.0, 0.0)] * 3, 0.0,
                             dict(hit={0: -2, 1: -2, 2: -1}, t={0: 0.0, 1: 0.0}, tie=[(0, (0, 0), (1, 0))], steps={0: 1}))
    # -- a far disc met in an early step while the nearer one is met only later: the nearer one must win.
    # Through the 3 x 3 block: F = (1.45, 0.5499), cell (2, 1), is grazed at t = 1.39 and met in step 1 (block columns
    # 0 .. 2); N = (1.52, 0.3), cell (3, 0), is hit at t = 1.22 and met in step 2 only.  Both steps lie in the wave's
    # first batch of seven: this one tells a walk that asks after every step.
    out["far_first_block"] = case([(1.45, 0.5499), (1.52, 0.3)], NO_WALLS, [(0.05, 0.3)], [(1.0, 0.0)], 4.0,
                                  dict(hit={0: 1}, first_hit_fails=(1,)))
    # The same two discs with the origin five cells further back: F is met in step 6, the LAST step of the wave's first
    # batch, N in step 7, the first of the next; both are hit in step 7 (t = 3.84 and 3.72), so after the first batch
    # best t = 3.84 is not below fl(7 dt) = 3.5 and the walk must go on.  A kernel that ends after the first batch that
    # met a disc reports F.
    out["far_first_batch"] = case([(1.45, 0.5499), (1.52, 0.3)], NO_WALLS, [(0.05 - 5 * S, 0.3)], [(1.0, 0.0)], 6.0,
                                  dict(hit={0: 1}, first_hit_fails=(1, N.RAY_WAVE_STEPS), met_in_steps={0: 6, 1: 7}))
    # Through a shared bucket: F lies on the ray in a cell that shares its bucket with a cell of step 0's block; a kernel
    # without the own-cell test meets it there.  N, nearer, is met steps later.  What this can tell: such a kernel still
    # keeps the smallest key, so F's larger t loses and the answer stays right -- the own-cell test saves work here, it
    # does not decide the output; the case fails only for a kernel that ALSO ends at its first hit.  The stopping rule
    # on its own is what the two cases above tell.
    near, far = shared_bucket_pair()
    beside = {1: 1.1 * H, 0: 0.9 * H, -1: -0.9 * H}[near[1]]                       # in the near cell, out of the ray's reach
    out["far_first_bucket"] = case([((far[0] + 0.5) * H, 0.02), (3.3, 0.02), (1.5 * H, beside)], NO_WALLS, [(0.05, 0.02)],
                                   [(1.0, 0.0)], (far[0] + 2) * H, dict(hit={0: 1}, shared_bucket=(near, far)))
    # -- ties: two discs mirrored about an axis-parallel ray (the lower index wins, though the other's cell comes first
    # in raster order); a wall and a disc at the same t (the wall wins)
    out["mirrored_discs"] = case([(1.0, 0.125), (1.0, -0.125), (2.0, -0.125), (2.0, 0.125)], NO_WALLS, [(0.0, 0.0), (3.0, 0.0)],
                                 [(1.0, 0.0), (-1.0, 0.0)], 4.0, dict(hit={0: 0, 1: 2}, tie=[(0, (1, 0), (1, 1)), (1, (1, 2), (1, 3))]))
    out["wall_ties_disc"] = case(disc, wall, [(0.0, 0.0)], [(1.0, 0.0)], 4.0, dict(hit={0: -2}, t={0: 0.75}, tie=[(0, (0, 0), (1, 0))]))
    # -- walls before and behind a disc, met from either face (A -> B up, then down)
    up, down = [(0.5, -1.0), (0.5, 1.0)], [(0.5, 1.0), (0.5, -1.0)]
    far_up, far_down = [(2.0, -1.0), (2.0, 1.0)], [(2.0, 1.0), (2.0, -1.0)]
    for name, walls_, want in (("wall_before_disc_front", [up], -2), ("wall_before_disc_back", [down], -2),
                               ("wall_behind_disc_front", [far_up], 0), ("wall_behind_disc_back", [far_down], 0),
                               ("two_walls", [far_down, up], -3)):
        out[name] = case(disc, walls_, [(0.0, 0.0), (3.0, 0.0)], [(1.0, 0.0), (-1.0, 0.0)], 4.0, dict(hit={0: want}))
    # -- a wall's ends, u = 0 and u = 1 exactly, and just beyond them; parallel and collinear rays
    seg = [[(1.0, 0.0), (1.0, 1.0)]]
    out["wall_ends"] = case([], seg, [(0.0, 0.0), (0.0, 1.0), (0.0, np.nextafter(0.0, -1.0)), (0.0, np.nextafter(1.0, 2.0)), (0.0, 0.5)],
                            [(1.0, 0.0)] * 5, 4.0, dict(hit={0: -2, 1: -2, 2: -1, 3: -1, 4: -2}, t={0: 1.0, 1: 1.0, 4: 1.0}))
    out["wall_parallel"] = case([(1.0, 2.0)], seg, [(0.5, 0.0), (1.0, -1.0), (1.0, 0.5), (1.0, -1.0)],
                                [(0.0, 1.0), (0.0, 1.0), (0.0, -1.0), (0.0, 4.0)], 4.0, dict(hit={0: -1, 1: 0, 2: -1, 3: 0}))
    # -- rays along a cell boundary and diagonals through cell corners, in a cloud
    pts = cloud(21, 60)
    along = [[(-0.4, H), (1.0, 0.0)], [(2 * H, -0.4), (0.0, 1.0)], [(4.4, 3 * H), (-1.0, 0.0)], [(0.0, 0.0), (1.0, 1.0)],
             [(4 * H, 0.0), (-1.0, 1.0)], [(-H, -H), (0.5, 0.5)], [(3 * H, 3 * H), (-2.0, -2.0)], [(0.0, 6 * H), (1.0, -1.0)]]
    out["cell_boundaries"] = case(pts, BOX, [o for o, _ in along], [d for _, d in along], 8.0, {})
    # -- negative coordinates, where the unsigned cells wrap
    o, d = fan(31, 40, (-6.0, -5.0), (-1.0, -1.0))
    out["negative_cells"] = case(cloud(30, 70, (-6.0, -5.0), (-1.0, -1.0)), BOX - 5.5, o, d, 6.0, dict(negative_cells=True))
    # -- dead rays and points that are not finite
    pts = cloud(41, 50).copy()
    for r, p in {3: (NAN, 0.5), 11: (0.5, NAN), 17: (INF, 0.5), 23: (0.5, -INF), 29: (NAN, NAN), 37: (-INF, INF)}.items():
        pts[r] = p
    o, d = fan(42, 24)
    o, d = o.copy(), d.copy()
    d[2] = (0.0, 0.0)
    d[5] = (-0.0, 0.0)
    o[7], o[9], o[11] = (NAN, 1.0), (1.0, INF), (-INF, NAN)
    d[13], d[15], d[17] = (NAN, 1.0), (1.0, -INF), (INF, INF)
    d[19] = (1e-170, 1e-170)                                                       # a underflows to 0
    out["not_finite"] = case(pts, BOX, o, d, 3.0, dict(hit={r: -1 for r in (2, 5, 7, 9, 11, 13, 15, 17, 19)},
                                                      t={r: NAN for r in (2, 5, 7, 9, 11, 13, 15, 17, 19)}))
    # -- ray counts at the workgroup's edge
    pts = cloud(51, 90)
    for n in RAYS:
        o, d = fan(60 + n, n)
        out[f"rays_{n}"] = case(pts, BOX, o, d, 2.5, {})
    out["rays_of_nothing"] = case([], NO_WALLS, *fan(70, 5), 2.5, dict(hit={r: -1 for r in range(5)}, t={r: INF for r in range(5)}))
    # -- rho at half the grid's radius (every case above) and much below it; long rays through a dense cloud; long directions
    o, d = fan(81, 70)
    out["small_rho"] = case(cloud(80, 120), BOX, o, d * 4, 2.0, {}, rho=0.02, radius=0.5)
    out["dense"] = case(cloud(82, 128), BOX, o, d * 7, 1.0, {})
    out["particles_only"] = case(cloud(83, 100), NO_WALLS, o, d * 3, 1.0, {})
    # -- the cap: exactly RAY_MAX_STEPS steps through empty space are served, one step more is status -4
    last = (N.RAY_MAX_STEPS - 1) * S                                                # fl(k S) <= last for k < RAY_MAX_STEPS
    out["cap_served"] = case([(last + 0.2, 3.0), (0.0, -9.0)], NO_WALLS, [(0.0, 0.0), (0.0, 1.0), (0.0, 3.0)],
                             [(1.0, 0.0), (0.5, 0.0), (1.0, 0.0)], last,
                             dict(steps={0: N.RAY_MAX_STEPS, 1: N.RAY_MAX_STEPS // 2, 2: N.RAY_MAX_STEPS},
                                  hit={0: -1, 1: -1, 2: 0}, status=0))
    out["cap_exceeded"] = case([(last - 0.1, 0.0), (0.0, -9.0)], NO_WALLS, [(0.0, 0.0)], [(1.0, 0.0)], N.RAY_MAX_STEPS * S,
                               dict(steps={0: N.RAY_MAX_STEPS + 1}, status=N.PAIRS_RANGE))
    out["cap_kept_by_a_wall"] = case([(2.0, 0.0)], [[(9.0, -1.0), (9.0, 1.0)]], [(0.0, 0.0)], [(1.0, 0.0)], N.RAY_MAX_STEPS * S,
                                     dict(hit={0: 0}, steps={0: 19}, status=0))
    # -- an end point outside the domain: status -1
    out["end_outside"] = case([(2.0, 0.0)], NO_WALLS, [(0.0, 0.0)], [(1.0, 0.0)], 2.0 ** 31 * S, dict(status=N.PAIRS_DOMAIN))
    out["origin_outside"] = case([(2.0, 0.0)], NO_WALLS, [(0.0, 0.0), (-(2.0 ** 31) * S, 0.0)], [(1.0, 0.0), (0.0, 1.0)], 2.0,
                                 dict(status=N.PAIRS_DOMAIN))
    return out


def served():
    """The names of the cases that give results, sorted."""
    return sorted(name for name, c in cases().items() if not c.claims.get("status"))


def refused():
    return sorted(name for name, c in cases().items() if c.claims.get("status"))
