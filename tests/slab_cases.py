"""Small worlds in which one decision rule of the slab decomposition decides the result (tests/test_slab_cases_cpu.py,
tests/test_gpu_slab_cases.py), in the style of wall_cases.py and tile_cases.py.

The rules (sand_crate_amd/slab.py, sc_kernels.h: wall_and_cell, halo_pack_one):
  ownership   a particle belongs to the slab that floor(p / d) of its position at the start of the tick names -- the IEEE
              division, not floor_div's product p * (1 / d);
  pack        a slab [lo, hi) sends what it stores in columns < lo + 3 to the left and >= hi - 3 to the right, migrants
              included; the receiver keeps columns [lo - 3, hi + 3) and has one more column of grid on either side;
  reach       an owned particle i needs its neighbors j and their neighbors k AFTER the hard wall fix: three columns reach
              them as long as no fix exceeds r along the slab axis.  Where fixes do, i misses a particle only if i itself was
              put at least half a column beyond its slab's edge, or the missed one came from beyond the band to less than
              2.5 columns from the edge: the particle's owner reports either (F_HALO_REACH) from the fix it applied.
Every world is given for slabs of columns (x) and is transposed as a whole, gravity included, for slabs of rows (y).
All of them use d = 0.05: 20 columns, a few hundred particles at most, fixed bodies as plain segment lists.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

D = 0.05
R = D / 2
DT = 0.002 * D / 0.01
HALO = 3
COEF = dict(dt=DT, particle_radius=R, wall_collision_decay=0.2, pressure_amplifier=30.0, ignored_pressure=0.0,
            collider_noise_level=0.1, viscosity=8.0, surface_smoothing=100.0, target_pressure=-2.0, gravity=[0.0, 9.8],
            max_particles=4000)
BOX = [((0.0, 0.0), (0.0, 1.0)), ((0.0, 0.0), (1.0, 0.0)), ((1.0, 0.0), (1.0, 1.0)), ((0.0, 1.0), (1.0, 1.0))]
FILLERS = [(0.06, 0.2), (0.94, 0.2)]  # columns 1 and 18: the particles span the box whatever the case is about

# what the chain must do: equal the single domain bit for bit / report the fix that went too far / report the lost particle
EQUAL, REACH, CROSSED = "equal", "reach", "crossed"
MESSAGES = {REACH: "more than one radius along the slab axis", CROSSED: "crossed a whole slab in one tick"}
COLUMNS = 20


def up(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(x, np.inf))
    return x


def down(x, n=1):
    for _ in range(n):
        x = float(np.nextafter(x, -np.inf))
    return x


@dataclass
class Case:
    name: str
    points: list                     # (x, y) or (x, y, vx, vy), along-the-axis coordinate first
    cuts: list
    expect: str = EQUAL
    bodies: list = field(default_factory=list)    # each a list of segments ((ax, ay), (bx, by)), fixed
    marks: dict = field(default_factory=dict)     # name -> index of a particle a premise is about
    overlap_ok: bool = True          # every particle stays within the band margin of the overlapped message
    rebalance_every: int = 0
    raisers: list = field(default_factory=list)   # (mark, owning slab, arm) of every report of a wall fix that is due
    first_report_tick: int = 0       # the tick (from 0) whose exchange or wall pass reports

    def mirrored(self):
        """The same world reflected, x -> 1 - x: slab k becomes slab n - 1 - k, left becomes right."""
        n = self.n_slabs
        return Case(self.name + "_mirrored", [(1.0 - q[0], q[1]) + ((-q[2], q[3]) if len(q) == 4 else ()) for q in self.points],
                    [COLUMNS - c for c in reversed(self.cuts)], expect=self.expect,
                    bodies=[[((1.0 - a[0], a[1]), (1.0 - b[0], b[1])) for a, b in segs] for segs in self.bodies],
                    marks=dict(self.marks), overlap_ok=self.overlap_ok, rebalance_every=self.rebalance_every,
                    raisers=[(m, n - 1 - k, arm) for m, k, arm in self.raisers], first_report_tick=self.first_report_tick)

    @property
    def n_slabs(self):
        return len(self.cuts) + 1

    def world(self, axis="x"):
        """-> rigid body configs (as in a scene's YAML), coefficients, particles, velocities; axis "y": transposed."""
        pts = np.array([tuple(q) + (0.0, 0.0) * (len(q) == 2) for q in self.points + FILLERS], dtype=np.float64)
        p, v = pts[:, 0:2].copy(), pts[:, 2:4].copy()
        coef = dict(COEF, gravity=list(COEF["gravity"]))
        flip = (lambda q: [float(q[1]), float(q[0])]) if axis == "y" else (lambda q: [float(q[0]), float(q[1])])
        bodies = [{"fixed": {"name": f"body{k}", "segments": [[flip(a), flip(b)] for a, b in segs]}}
                  for k, segs in enumerate([BOX] + self.bodies)]
        if axis == "y":
            p, v = p[:, ::-1].copy(), v[:, ::-1].copy()
            coef["gravity"] = coef["gravity"][::-1]
        return bodies, coef, p, v


def vee(tip_x, tip_y, away, arms=2, length=0.1):
    """Segments that share the end point (tip_x, tip_y) and lead away from it towards `away` (+1 / -1 along x): for a
    particle just on the other side of the tip every one of them has the tip as its nearest point, so each is a contact
    of its own and the fix is `arms` times (r - distance), straight away from the tip."""
    ends = {2: (-1.0, 1.0), 3: (-1.0, 0.0, 1.0)}[arms]
    return [((tip_x, tip_y), (tip_x + away * length, tip_y + e * length)) for e in ends]


def post(x_wall, y, half=0.03):
    """A short wall across the axis: one contact, a fix of r - distance along x."""
    return [((x_wall, y - half), (x_wall, y + half))]


def speed(columns):
    return columns * D / DT


# ------------------------------------------------------------------ the cases
def on_the_cut():
    """Cut 12, whose lower edge is one of the coordinates where the product and the quotient floor differently: 12 d is
    0.6000000000000001, one ulp below is 0.6 with 0.6 * 20 = 12.0 and 0.6 / 0.05 = 11.999...; the same at 9 d, the edge
    of the band that slab 1 sends.  Each of these has a companion on either side so that a wrong owner changes a force."""
    c = 12
    edge, band = c * D, (c - HALO) * D
    xs = {"at": edge, "below": down(edge), "above": up(edge), "band_at": band, "band_below": down(band), "band_above": up(band)}
    pts, marks = [], {}
    for k, (name, x) in enumerate(xs.items()):
        y = 0.15 + 0.12 * k
        marks[name] = len(pts)
        pts += [(x, y), (x - 0.7 * D, y + 0.01), (x + 0.7 * D, y - 0.01)]
    return Case("on_the_cut", pts, [c], marks=marks)


def band_edges():
    """Chains without walls, 0.98 d apart.  i in the last owned column; k, the farthest particle i's result depends on, in
    column 11 (no chain reaches farther: 2 d); then l in column 12, the last one sent, and m in column 13, the first one
    that is not -- neither can matter to i.  Mirrored at the left edge of slab 1."""
    s = 0.98 * D
    pts, marks = [], {}
    for name, x0, sign, y in (("right", 9.95 * D, 1, 0.4), ("left", 10.05 * D, -1, 0.6)):
        for k, who in enumerate("ijklm"):
            marks[f"{name}_{who}"] = len(pts)
            pts.append((x0 + sign * k * s, y + 0.002 * k))
    return Case("band_edges", pts, [10], marks=marks)


def single_contact_reach():
    """The tight case of the three-column rule: i in column 9 and k in column 12, 2.97 d apart, each pushed towards j by ONE
    wall by 0.98 r; after the fix they are 1.99 d apart and j, half way, is a neighbor of both.  Mirrored for slab 1."""
    pts, marks, bodies = [], {}, []
    gap, span = 0.02 * R, 2.97 * D
    for name, xi, sign, y in (("right", 9.995 * D, 1, 0.5), ("left", 10.005 * D, -1, 0.3)):
        xk = xi + sign * span
        marks[f"{name}_i"], marks[f"{name}_j"], marks[f"{name}_k"] = len(pts), len(pts) + 1, len(pts) + 2
        pts += [(xi, y), ((xi + xk) / 2, y), (xk, y)]
        bodies += [post(xi - sign * gap, y), post(xk + sign * gap, y)]
    return Case("single_contact_reach", pts, [10], bodies=bodies, marks=marks)


def _joint_world(name, xi, xj, xk, i_side="joint", k_side="joint", raisers=(), mirrored=False):
    """i, j, k on one row at xi < xj < xk (before the fix).  i is pushed to the right and k to the left, by a joint of two
    segments whose tip is 0.1 r away (two contacts: 0.9 d) or by a post as far away (one contact: 0.45 d).
    `raisers`: (particle, slab that owns it, arm of the rule) for every report that is due -- "out": put half a column beyond
    its slab's edge, "in": come from beyond the band to less than 2.5 columns from the edge; none: the chain must equal."""
    y = 0.5
    wall = {"joint": vee, "post": lambda x, yy, away: post(x, yy)}
    bodies = [wall[i_side](xi - 0.1 * R, y, -1), wall[k_side](xk + 0.1 * R, y, +1)]
    case = Case(name, [(xi, y), (xj, y), (xk, y)], [10], expect=REACH if raisers else EQUAL, bodies=bodies,
                marks={"i": 0, "j": 1, "k": 2}, raisers=list(raisers))
    return case.mirrored() if mirrored else case


I_OUT, K_IN = ("i", 0, "out"), ("k", 1, "in")


def joint_reach(mirrored=False):
    """The reproduction: i at 0.4995 beside a joint whose tip is at 0.497, j at 0.592, k at 0.6845 beside a joint at 0.687.
    The span before the fix is 3.7 d, k sits in column 13 and is never sent; after the fix both are 0.95 d from j.  Without
    the report slab 0 computes i with a j that lacks a neighbor.  i is put at 10.89 d: its owner, slab 0, reports."""
    return _joint_world("joint_reach", 0.4995, 0.592, 0.6845, raisers=[I_OUT], mirrored=mirrored)


def joint_reach_one_side(mirrored=False):
    """A joint at i only; k is pushed by a single wall and starts at 13.24 d, column 13: 3.25 d from i, never sent, and
    0.95 d from j after the fix.  k's own fix is an ordinary one: the report comes from i, from slab 0."""
    return _joint_world("joint_reach_one_side", 0.4995, 0.592, 13.24 * D, k_side="post", raisers=[I_OUT], mirrored=mirrored)


def missed_one_reports(mirrored=False):
    """The other way round: i is pushed by a single wall, 9.99 d -> 10.44 d, short of half a column beyond its slab; k starts
    at 13.24 d beside a joint and is put at 12.34 d, 0.95 d from j at 11.39 d.  Slab 0 cannot know; k's owner, slab 1,
    sees k come in from beyond the band it sent and reports."""
    return _joint_world("missed_one_reports", 9.99 * D, 11.39 * D, 13.24 * D, i_side="post", raisers=[K_IN], mirrored=mirrored)


def joint_reach_not_neighbors():
    """The joints of joint_reach, but k 0.3 d farther out: after the fix it is 1.25 d from j and matters to nobody.  The
    check judges a particle by the fix it got, not by the neighbor lists that do not exist yet: reported all the same."""
    return _joint_world("joint_reach_not_neighbors", 0.4995, 0.592, 0.6845 + 0.3 * D, raisers=[I_OUT])


def out_just_over(mirrored=False):
    """The first threshold, (edge + 0.5) d less 0.01 d of margin, from either side: i is put at 10.51 d -- reported ..."""
    return _joint_world("out_just_over", 9.61 * D, 0.592, 0.6845, raisers=[I_OUT], mirrored=mirrored)


def out_just_under(mirrored=False):
    """... and at 10.47 d: not reported.  k is put at 12.79 d, 2.32 d away, so no j can join them and the chain equals."""
    return _joint_world("out_just_under", 9.57 * D, 0.592, 0.6845, mirrored=mirrored)


def in_just_under(mirrored=False):
    """The second threshold, (edge + 2.5) d plus 0.01 d of margin: k comes from 13.39 d to 12.49 d -- reported by slab 1 ..."""
    return _joint_world("in_just_under", 9.99 * D, 11.39 * D, 13.39 * D, i_side="post", raisers=[K_IN], mirrored=mirrored)


def in_just_over(mirrored=False):
    """... and from 13.43 d to 12.53 d: not reported.  i is put at 10.44 d, 2.09 d away: no j can join them."""
    return _joint_world("in_just_over", 9.99 * D, 11.39 * D, 13.43 * D, i_side="post", mirrored=mirrored)


def joint_lands_short():
    """Far from both thresholds: i goes from 9.39 d to 10.29 d, k from 13.69 d to 12.79 d.  Nothing is reported."""
    return _joint_world("joint_lands_short", 9.39 * D, 0.592, 0.6845)


def joint_inside_window():
    """joint_reach six columns to the left: all of it inside slab 0 although k starts in column 7, the first column of the
    band slab 0 sends.  Nobody crosses a slab's edge and nobody comes in from beyond a band: nothing is reported."""
    return _joint_world("joint_inside_window", 0.4995 - 6 * D, 0.592 - 6 * D, 0.6845 - 6 * D)


def joint_outside_window():
    """... and seven columns to the left: nobody touches columns 7 .. 12.  Nothing is reported."""
    return _joint_world("joint_outside_window", 0.4995 - 7 * D, 0.592 - 7 * D, 0.6845 - 7 * D)


def migrant_across_a_slab(mirrored=False):
    """Three slabs, the middle one [6, 14): a particle in column 5 that moves ten columns in one tick ends in column 15,
    in slab 2.  Slab 0 sends it to its neighbor, slab 1, where it is a ghost; slab 2 never hears of it.  Slab 1 sees a record
    from the left beyond its own right edge and reports it at the exchange after the move (the second tick): the particle
    count does not shrink silently."""
    pts = [(5.5 * D, 0.5, speed(10), 0.0), (15.9 * D, 0.51), (10.2 * D, 0.5), (10.9 * D, 0.52)]
    case = Case("migrant_across_a_slab", pts, [6, 14], expect=CROSSED, marks={"runner": 0}, overlap_ok=False, first_report_tick=1)
    return case.mirrored() if mirrored else case


def thin_slab():
    """Three slabs, the middle one of the minimum width of 8 columns [6, 14): a lattice 0.8 d apart over every column, so
    that both bands of every slab are in use and a particle of the middle slab is a ghost on one side at most."""
    rs = np.random.RandomState(3)
    xs = np.arange(0.07, 0.94, 0.8 * D)
    pts = [(x + 0.1 * D * (rs.rand() - 0.5), y + 0.1 * D * (rs.rand() - 0.5)) for y in (0.36, 0.40, 0.44, 0.48, 0.52) for x in xs]
    return Case("thin_slab", [(float(x), float(y)) for x, y in pts], [6, 14])


def migrants():
    """Particles that cross the cut in one tick: from column 9 by 1, 3, 4 and 5 columns to the right, from column 10 as far
    to the left, each on a row of its own with a slow companion where it lands.  The ones that go 4 and 5 columns land
    beyond the band the sender keeps as ghosts, the last one beyond the sender's local grid as well: the receiver owns them
    (its slab is open-ended: nothing lies beyond it), the sender drops its copy, and the particle count stays.  Where a
    slab does lie beyond the receiver: migrant_across_a_slab."""
    pts, marks = [], {}
    for k, n in enumerate((1, 3, 4, 5)):
        for name, x0, sign, y in (("right", 9.5 * D, 1, 0.12 + 0.2 * k), ("left", 10.5 * D, -1, 0.22 + 0.2 * k)):
            marks[f"{name}_{n}"] = len(pts)
            pts.append((x0, y, sign * speed(n), 0.0))
            pts.append((x0 + sign * (n + 0.6) * D, y + 0.01, 0.0, 0.0))
    return Case("migrants", pts, [10], marks=marks, overlap_ok=False)


def ghost_pushed_out():
    """A ghost of slab 0 at 12.9 d, in the last band column, beside a joint of THREE segments: the fix is 2.7 r = 1.35 d to
    the right, into column 14, past the one column of slack of slab 0's grid (columns .. 13).  The cell index is
    range-checked after the fix (wall_and_cell) and a ghost outside the grid is dropped.  Its owner, slab 1, has no cut on
    that side, so nothing is reported, and no owned particle of slab 0 changes: the chain equals the single domain."""
    y = 0.5
    xg = 12.9 * D
    pts = [(xg, y), (9.9 * D, y), (10.85 * D, y), (14.3 * D, y + 0.3 * D)]
    return Case("ghost_pushed_out", pts, [10], bodies=[vee(xg - 0.1 * R, y, -1, arms=3, length=0.04)],
                marks={"ghost": 0, "i": 1, "j": 2, "lands_beside": 3})


def rebalance_over_a_cluster():
    """Cuts re-derived every tick; a cluster of 48 particles in columns 10 .. 12, the band of slab 0, and a dozen particles
    elsewhere: the equal-count cut lies inside the cluster and the cut moves into it."""
    rs = np.random.RandomState(4)
    pts = [(10.1 * D + 0.8 * D * (k % 4) + 0.05 * D * rs.rand(), 0.3 + 0.8 * D * (k // 4) + 0.05 * D * rs.rand()) for k in range(48)]
    pts += [(0.15 + 0.06 * k, 0.7 + 0.01 * (k % 3)) for k in range(6)] + [(0.75 + 0.03 * k, 0.72) for k in range(6)]
    return Case("rebalance_over_a_cluster", [(float(x), float(y)) for x, y in pts], [10], rebalance_every=1, overlap_ok=False)


MIRRORED = [joint_reach, joint_reach_one_side, missed_one_reports, out_just_over, out_just_under, in_just_under, in_just_over,
            migrant_across_a_slab]
BUILDERS = [on_the_cut, band_edges, single_contact_reach, joint_reach, joint_reach_one_side, missed_one_reports,
            joint_reach_not_neighbors, out_just_over, out_just_under, in_just_under, in_just_over, joint_lands_short,
            joint_inside_window, joint_outside_window, thin_slab, migrants, migrant_across_a_slab, ghost_pushed_out,
            rebalance_over_a_cluster]
CASES = {b.__name__: b for b in BUILDERS}
CASES.update({b.__name__ + "_mirrored": (lambda b=b: b(mirrored=True)) for b in MIRRORED})
