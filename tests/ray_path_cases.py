"""The named inputs of the ray paths' tests: name -> Case(points (n, 2), walls (S, 2, 2), origins (R, 2), directions
(R, 2), rho, max_t, bounces, particles, claims, catches).  Each world is the smallest that can show its mistake.
`particles` False looks at the walls alone, as `Crate.ray_paths(particles=False)` does.  `claims` says what the world is
there for, in terms tests/test_ray_path_cases_cpu.py proves from tests/ray_path_spec.py; `catches` names the `wrong=`
switches of the spec that change this case's result -- all of them, the CPU test checks the list both ways;
tests/test_gpu_ray_paths.py runs each case on the device against the spec.  The kinds of claim:

    "hits"        {r: [hit of leg 0, 1, ...]}: the legs of ray r that were written, worked out by hand
    "end"         {r: end}
    "t"           {(r, k): t}: leg k's t, exactly
    "t_sum"       {r: sum}: the t's of ray r add up to this, to a relative 1e-12
    "reversed"    [r]: the direction after leg 0 is -d, in both components exactly
    "kept"        [r]: the direction after leg 0 is d: the ray was leaving already
    "reflected"   [r]: ... is not d
    "inward"      [(r, k, j)]: leg k >= 1 of ray r starts inside or on disc j (cc <= 0) heading inward (b < 0): hit at t = 0
    "outward"     [(r, k, j)]: ... heading outward (b >= 0): disc j is not hit
    "tie"         [(r, k, (kind, index), (kind, index))]: two candidates of leg k have the same t, bit for bit (kind 0:
                  wall, 1: disc); the first one wins
    "excluded"    {(r, k): j}: leg k >= 1 of ray r has left disc j and by rounding starts in or on it heading inward
                  (cc <= 0, b < 0): the rule without the exclusion meets j again at t = 0
    "batch"       {(r, k): B}: leg k's hit lies in step floor(t / dt) of its walk, and that step in batch B of seven
    "leg0_steps"  {r: k}: leg 0 of ray r walks at least k steps, which a walk that is not restarted then skips
    "nan_normal"  [(r, k)]: the normal of leg k is NaN
    "all_legs"    every path has `bounces` + 1 legs that hit, both kinds of hit occur on legs >= 1 and no leg >= 1 has t = 0
"""
import collections
import functools

import numpy as np

import ray_cases as K
import ray_spec as RS

Case = collections.namedtuple("Case", "points walls origins directions rho max_t bounces particles claims catches")

RHO, S = K.RHO, K.S
NAN, INF = K.NAN, K.INF
NO_WALLS = K.NO_WALLS
ROOM = np.array([[[0.0, 0.0], [4.0, 0.0]], [[4.0, 0.0], [4.0, 3.0]], [[4.0, 3.0], [0.0, 3.0]], [[0.0, 3.0], [0.0, 0.0]]])
GROUP = 10.0                                                       # long_legs: 20 cells between its three worlds


def case(points, walls, origins, directions, max_t, bounces, claims, catches, rho=RHO, particles=True):
    return Case(K.arr(points, (2,)), K.arr(walls, (2, 2)), K.arr(origins, (2,)), K.arr(directions, (2,)), float(rho),
                float(max_t), int(bounces), bool(particles), claims, tuple(sorted(catches)))


def spec_args(c):
    """The arguments of `ray_path_spec.paths` for a case: walls alone are rho = 0 on a grid of the same radius."""
    return (c.points if c.particles else None, c.walls, c.origins, c.directions, c.rho if c.particles else 0.0, c.max_t, c.bounces,
            2 * c.rho)


def status(c):
    """What the call reports for leg 0 (ray_spec.status): 0 for every case here."""
    points, walls, origins, directions, rho, max_t, _, radius = spec_args(c)
    return RS.status(points, walls, origins, directions, rho, max_t, radius)


def mirror(x, y):
    """A wall through (x, y) that turns a ray coming straight down into one going along +x, up to rounding."""
    return [(x - 0.2, y + 0.2), (x + 0.2, y - 0.2)]


def turning_wall(at, d, want, half=0.3):
    """A wall through `at` that reflects the direction d into the direction `want`, of the same length, up to rounding."""
    n = np.array(want, dtype=np.float64) - np.array(d, dtype=np.float64)
    e = np.array([n[1], -n[0]]) / np.hypot(*n)
    return [tuple(np.array(at) - half * e), tuple(np.array(at) + half * e)]


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    # -- four walls and no particles: from (1, 1) along (0.8, 0.6) the sixteen legs hit walls 2, 1, 0, 3, 2, ...
    out["mirror_box"] = case([], ROOM, [(1.0, 1.0)], [(0.8, 0.6)], 40.0, 15,
                             dict(hits={0: [-4, -3, -2, -5] * 4}, end={0: 0}, t_sum={0: 38.75}),
                             ("no_exclusion", "wall_normal_unflipped"), particles=False)
    # -- one disc, rays along a diameter: the direction is reversed exactly, and leg 1 meets nothing
    out["head_on"] = case([(1.0, 0.0)], NO_WALLS, [(0.0, 0.0), (1.0, 1.0)], [(1.0, 0.0), (0.0, -0.5)], 3.0, 1,
                          dict(hits={0: [0, -1], 1: [0, -1]}, end={0: 1, 1: 1}, t={(0, 0): 0.75, (1, 0): 1.5, (0, 1): INF},
                               reversed=[0, 1]), ())
    # -- two discs, a ray along their line of centres: 0.75 to the first rim, 1.5 from rim to rim; the budget of 14.35
    # pays for legs 0 .. 9 (14.25) and runs out in leg 10
    out["ping_pong"] = case([(0.0, 0.0), (2.0, 0.0)], NO_WALLS, [(1.0, 0.0)], [(1.0, 0.0)], 14.35, 15,
                            dict(hits={0: [1, 0] * 5 + [-1]}, end={0: 1}, t={(0, 0): 0.75, (0, 1): 1.5, (0, 9): 1.5, (0, 10): INF}),
                            ("budget_kept", "walk_not_restarted"))
    # -- two discs 0.6 diameters apart, a 3-4-5 wedge in sixteenths: rho = 5/16, centres (-+3/16, 0), the rims cross at
    # (0, 1/4), exactly.  Ray 0 comes straight down on that point: both discs at t = 0.75, disc 0 wins; leg 1 starts on
    # the rim of disc 1 heading inward, leg 2 on the rim of disc 0 heading outward.  The others are aimed round it.
    aims = [(0.0, 0.25), (2.0 ** -40, 0.25), (-2.0 ** -40, 0.25), (2.0 ** -20, 0.25), (-2.0 ** -20, 0.25), (0.01, 0.25), (-0.01, 0.25)]
    out["overlap_wedge"] = case([(-0.1875, 0.0), (0.1875, 0.0)], NO_WALLS, [(x, 1.0) for x, _ in aims], [(0.0, -1.0)] * len(aims),
                                4.0, 3, dict(hits={0: [0, 1, -1]}, end={0: 1}, t={(0, 0): 0.75, (0, 1): 0.0},
                                             tie=[(0, 0, (1, 0), (1, 1))], inward=[(0, 1, 1)], outward=[(0, 2, 0)]),
                                ("leg0_inside_rule", "walk_not_restarted"), rho=0.3125)
    # -- leg 0 starts inside a disc: hit at t = 0; heading outward the direction is kept, heading inward it is reflected
    out["inside_out"] = case([(1.0, 1.0)], ROOM, [(1.1, 1.0)], [(1.0, 0.0)], 9.0, 1,
                             dict(hits={0: [0, -3]}, end={0: 0}, t={(0, 0): 0.0, (0, 1): 2.9}, kept=[0]), ("always_reflect", "wall_normal_unflipped"))
    out["inside_in"] = case([(1.0, 1.0)], ROOM, [(1.1, 1.0)], [(-1.0, 0.0)], 9.0, 1,
                            dict(hits={0: [0, -3]}, end={0: 0}, t={(0, 0): 0.0, (0, 1): 2.9}, reflected=[0], reversed=[0]), ("wall_normal_unflipped",))
    # -- the origin at a disc's centre: the normal is 0 / 0
    out["centre"] = case([(1.0, 1.0)], ROOM, [(1.0, 1.0)], [(1.0, 0.0)], 9.0, 2,
                         dict(hits={0: [0]}, end={0: 2}, t={(0, 0): 0.0}, nan_normal=[(0, 0)]), ())
    # -- tangent and near-tangent hits.  Rays 0 .. 5 run along +x, the centre at the ray's distance rho and ulps nearer:
    # their arithmetic is exact and the ray leaves by the rule's own b >= 0.  Rays 6 .. 9 are oblique and were SEARCHED
    # on the CPU (random origins and directions, one disc at the distance rho (1 - eps) from the ray, eps 0 .. 1e-12;
    # some 3 in a thousand qualify): there dn rounds to 0 and the direction is kept (ray 7: to -2^-53, it turns by an
    # ulp), while at the next origin cc of the disc just left rounds to <= 0 and b to < 0 -- only the exclusion keeps
    # leg 1 from meeting that disc again at t = 0.
    near = [0.25] + [float(np.nextafter(0.25, 0.0))] + [0.25 - 2.0 ** -k for k in (50, 44, 36, 28)]
    oblique = [((-4.785577556963419, -0.5814202329711267), (0.774107825340286, -0.931834547268954), (-3.8149674335142336, -1.358561282220448)),
               ((-3.843577823263926, -0.5248094983124938), (0.833811896770474, 0.7564594021223734), (-2.9785707816383677, 0.5975035598191087)),
               ((-3.633487509694149, -0.5868098597975022), (0.4519757126463183, 1.3731332036125325), (-3.3495844325657846, 1.0753109848535962)),
               ((-3.911572022989832, 0.8173918037822387), (-0.6050923190237285, 0.46371393191858906), (-5.635096637467545, 1.8232491393128032))]
    rays = range(len(near) + len(oblique))
    out["grazing"] = case([(0.25 + GROUP * i, y) for i, y in enumerate(near)] + [c for _, _, c in oblique], NO_WALLS,
                          [(GROUP * i, 0.0) for i in range(len(near))] + [o for o, _, _ in oblique],
                          [(1.0, 0.0)] * len(near) + [d for _, d, _ in oblique], 3.0, 2,
                          dict(hits={i: [i, -1] for i in rays}, end={i: 1 for i in rays}, t={(0, 0): 0.25},
                               kept=[0, 6, 8, 9], reflected=[7], excluded={(i, 1): i for i in list(rays)[len(near):]}),
                          ("no_exclusion",))
    # -- ray_cases' stop-rule shapes on leg 1: every ray comes straight down, 6 steps, on a wall that turns it along +x
    # at (-2.45 + GROUP g, 0.3).  Group 0 is far_first_batch (F met in step 6, N in step 7, both hit in step 7: the
    # second batch), group 1 far_first_block (F met in step 1, the nearer N only in step 2 of the same batch), group 2 a
    # disc hit in step 14, the third batch.
    pts = [(1.45, 0.5499), (1.52, 0.3), (1.45 - 5 * S + GROUP, 0.5499), (1.52 - 5 * S + GROUP, 0.3), (5.15 + 2 * GROUP, 0.3)]
    out["long_legs"] = case(pts, [mirror(-2.45 + GROUP * g, 0.3) for g in range(3)], [(-2.45 + GROUP * g, 3.3) for g in range(3)],
                            [(0.0, -1.0)] * 3, 12.0, 1,
                            dict(hits={0: [-2, 1], 1: [-3, 3], 2: [-4, 4]}, end={0: 0, 1: 0, 2: 0},
                                 batch={(0, 1): 1, (1, 1): 0, (2, 1): 2}, leg0_steps={0: 6, 1: 6, 2: 6}),
                            ("no_exclusion", "walk_not_restarted", "wall_normal_unflipped"))
    # -- a later leg that leaves the domain, walks past the cap, or both.  Ray 0 goes down left from the origin and is
    # turned straight up by wall 0; ray 1 goes right, is turned back by wall 1 and ends at wall 2.  `lid`, wall 3, lies
    # above ray 0's second leg: with it the leg's walk is short, and only its end point is too far.
    d0 = (-1.0, -1.0)
    turn = turning_wall((-0.5, -0.5), d0, (0.0, float(np.hypot(*d0))))
    sides = [turn, [(2.0, -1.0), (2.0, 1.0)], [(-3.0, -1.0), (-3.0, 1.0)]]
    lid = [(-2.0, 5.0), (1.0, 5.0)]
    far = 0.9 * 2.0 ** 31 * S
    two = dict(origins=[(0.0, 0.0), (0.0, 0.0)], directions=[d0, (1.0, 0.0)])
    out["leaves_domain"] = case([(0.5, 2.0)], sides + [lid], two["origins"], two["directions"], far, 1,
                                dict(hits={0: [-2], 1: [-3, -4]}, end={0: -1, 1: 0}), ("no_exclusion", "wall_normal_unflipped"))
    out["past_cap"] = case([(0.5, 2.0)], sides, two["origins"], two["directions"], 10000.0, 1,
                           dict(hits={0: [-2], 1: [-3, -4]}, end={0: -4, 1: 0}), ("no_exclusion", "wall_normal_unflipped"))
    out["leaves_domain_past_cap"] = case([(0.5, 2.0)], sides, two["origins"], two["directions"], far, 1,
                                         dict(hits={0: [-2], 1: [-3, -4]}, end={0: -1, 1: 0}), ("no_exclusion", "wall_normal_unflipped"))
    # -- ties on leg 1, after an exact reversal at the wall x = 0: a wall and a disc at t = 0.75, two mirrored discs
    out["ties_later"] = case([(1.0, 0.0), (1.0, 3.125), (1.0, 2.875)], [[(0.0, -1.0), (0.0, 4.0)], [(0.75, -1.0), (0.75, 1.0)]],
                             [(0.5, 0.0), (0.5, 3.0)], [(-1.0, 0.0), (-1.0, 0.0)], 4.0, 1,
                             dict(hits={0: [-2, -3], 1: [-2, 1]}, t={(0, 0): 0.5, (0, 1): 0.75}, reversed=[0, 1],
                                  tie=[(0, 1, (0, 1), (1, 0)), (1, 1, (1, 1), (1, 2))]), ("no_exclusion", "wall_normal_unflipped"))
    # -- dead rays and points that are not finite; no rays; no bounces
    c = K.cases()["not_finite"]
    dead = sorted(c.claims["hit"])
    out["dead_rows"] = case(c.points, c.walls, c.origins, c.directions, c.max_t, 2,
                            dict(end={r: 2 for r in dead}, t={(r, 0): NAN for r in dead}),
                            ("always_reflect", "budget_kept", "no_exclusion", "walk_not_restarted", "wall_normal_unflipped"))
    c = K.cases()["rays_0"]
    out["no_rays"] = case(c.points, c.walls, c.origins, c.directions, c.max_t, 3, {}, ())
    c = K.cases()["dense"]
    out["no_bounces"] = case(c.points, c.walls, c.origins, c.directions, c.max_t, 0, {}, ())
    # -- 4,096 points in the closed room, 256 rays from inside it and from outside every disc, 8 bounces
    rs = np.random.RandomState(7)
    pts = rs.rand(4096, 2) * [4.0, 3.0]
    starts = 0.05 + rs.rand(512, 2) * [3.9, 2.9]
    free = np.hypot(starts[:, None, 0] - pts[None, :, 0], starts[:, None, 1] - pts[None, :, 1]).min(axis=1) > 0.0101
    angle = rs.rand(256) * 2 * np.pi
    out["fuzz"] = case(pts, ROOM, starts[free][:256], np.stack([np.cos(angle), np.sin(angle)], axis=1), 20.0, 8,
                       dict(all_legs=True), ("no_exclusion", "wall_normal_unflipped", "walk_not_restarted"), rho=0.01)
    return out


def names():
    return sorted(cases())
