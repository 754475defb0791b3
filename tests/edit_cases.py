"""Worlds that are edited between ticks (tests/test_gpu_edits.py, tests/test_edit_cases_cpu.py).

The reference's viewer edits a running crate: a slider per coefficient and for the gravity, and bodies and sources are
plain objects that anyone may change between two `physics_tick()` calls.  The rule on top of every kernel rule: a tick
depends on the inputs as they stand when it starts, and on nothing an earlier tick was given.  What can remember an
earlier tick without any kernel being wrong:
  the cell grid    `particle_radius` sets it (build_world); a smaller radius means more cells, and beyond the allocation
                   ensure_cells frees and reallocates the bucket arrays, whose stamps carry meaning across ticks -- on
                   the fused path in the middle of a tick, when the promised tick has the smaller radius;
  the padded walls `tick_geometry` caches them per body: by the body, by the identity of its `segments` array, by the
                   array's bytes, and by the radius;
  packed inputs    `Crate.run` and the promise of `engine.tick(now, next)` pack a tick's inputs ahead of it;
  the stream       a source the device cannot draw (dt > 0.5) moves a noise="host" crate to the host's generator in the
                   middle of a run: the refused emission must have drawn nothing.
A case is a world, a start state, a number of ticks and `edits`: tick -> the edits applied before that tick.  An edit is
written once, against `Hands`, which reaches into either side: a `Crate` (its attributes, `rigid_bodies`,
`particle_sources`) or a `growth_cases.Stage` (its `coef`, `bodies`, `sources`).  `run` ticks a case on the oracle and
says for every edit what the tick would have been without it -- the stale variant, which the GPU tests must be able to
tell from the right one.

  radius_steps      2,700 particles standing on the floor, the radius R, R, 0.75 R, 0.75 R, 0.93 R, 1.3 R, 1.3 R, R, R:
                    the grid grows beyond its allocation, changes inside it, shrinks, and comes back; every growth of
                    the radius puts more particles within reach of the floor.  (2,700, not fewer: at 0.75 R the mean
                    list would fall below 2.)
  every_coefficient the same cloud, one edit a tick: `max_particles` raised after it clipped a source, then every
                    coefficient of the tick, the gravity by assignment and in place.
  walls_edited      a band of particles on the floor under walls that change: an endpoint written in place, the array
                    replaced, a motored body appended (4 -> 5 segments), a free body of 11 appended (16 = SC_MAX_SEGMENTS),
                    the motor's function replaced, the free body's velocity set, the radius edited while the box stands
                    still, the free body removed.
  sources_edited    a cloud and three sources: position, radius, velocity, noise, flow up, down, to 0 and back,
                    active_ticks, and a source appended.
  dt_above_half     forces off, one source, dt 0.002 -> 0.6 at tick 3 and back at tick 5.
  promise_edits     not a world: the (case, tick) pairs at which the next tick's inputs differ from this tick's in one
                    kind of way -- what `engine.tick(now, next)` promises across an edit.

Slab contexts are out of scope: their cuts are counted in cells of the diameter and are chosen once.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import copy
import math
from dataclasses import dataclass

import numpy as np

import force_cases as fc
import growth_cases as G
import wall_cases as wc

R = wc.R
NOISES = ("none", "counter", "host-sync", "host")
SCAN_PER_BLOCK = 2048    # cells per workgroup of the bucket scan (sc_device.h: kScanPerBlock)
MAX_SEGMENTS = 16        # SC_MAX_SEGMENTS
MAX_NEIGHBORS = 20       # SC_MAX_NEIGHBORS
# binomial(DT_HALF_FLOW, 0.6) on np.random seeded with 0, as dt_above_half draws it at tick 3: how many doubles the
# stream advances (test_edit_cases_cpu.py proves it)
DT_HALF_FLOW, DT_HALF_DRAWS = 1500, 2


# ------------------------------------------------------------------ one edit, two sides
class Hands:
    """What an edit reaches for, on either side.  `bodies` and `sources` are the lists themselves; `gravity` is the
    array itself, so that an edit may write into it."""

    def __init__(self, target):
        self.target = target
        self.is_stage = isinstance(target, G.Stage)

    @property
    def bodies(self) -> list:
        return self.target.bodies if self.is_stage else self.target.rigid_bodies

    @property
    def sources(self) -> list:
        return self.target.sources if self.is_stage else self.target.particle_sources

    @property
    def gravity(self) -> np.ndarray:
        return self.target.coef["gravity"] if self.is_stage else self.target.gravity

    def set(self, name, value) -> None:
        if name == "gravity":
            value = np.array(value, dtype=np.float64)
        if self.is_stage:
            self.target.coef[name] = value
        else:
            setattr(self.target, name, value)

    def body(self, name):
        return next(b for b in self.bodies if b.name == name)

    def new_body(self, config):
        """A body from its YAML form, of the side's own class."""
        if self.is_stage:
            from oracle.world import build_bodies
            return build_bodies([config])[0]
        from sand_crate_amd.rigid_body import build_rigid_bodies
        return build_rigid_bodies([config])[0]

    def new_source(self, config):
        if self.is_stage:
            from oracle.world import build_sources
            return build_sources([dict(config)])[0]
        from sand_crate_amd.particle_source import build_particle_sources
        return build_particle_sources([dict(config)])[0]


@dataclass
class Edit:
    name: str
    apply: callable          # Hands -> None

    def __call__(self, target) -> None:
        self.apply(target if isinstance(target, Hands) else Hands(target))


def coef_edit(name, value) -> Edit:
    return Edit(name, lambda w: w.set(name, value))


@dataclass
class EditCase:
    name: str
    bodies: list                 # rigid body configs, as in a scene's YAML
    sources: list                # particle source configs
    coef: dict
    p: np.ndarray                # the start state
    v: np.ndarray
    ticks: int
    edits: dict                  # tick -> (Edit, ...): applied, in order, before that tick
    noises: tuple = NOISES
    forces_on: bool = True
    warns_at: tuple = ()         # the ticks at which a noise="host" crate falls back to the host's stream

    def __post_init__(self):
        for a in (self.p, self.v):
            a.setflags(write=False)

    def edits_at(self, tick: int, without: int | None = None) -> tuple:
        """The edits before tick `tick`; `without`: all but that one -- the stale variant of the tick."""
        return tuple(e for k, e in enumerate(self.edits.get(tick, ())) if k != without)

    def apply(self, target, tick: int, without: int | None = None) -> None:
        hands = Hands(target)
        for edit in self.edits_at(tick, without):
            edit(hands)

    def sources_active(self, tick: int) -> bool:
        """Whether a source may draw at `tick` or later, as far as the configs and the edits up to `tick` say."""
        stage = G.Stage(self.bodies, self.coef, self.sources)
        for t in range(tick + 1):
            self.apply(stage, t)
        return any(s.active_ticks > tick for s in stage.sources)


def cloud(seed=3, n=2700, lo=(0.03, 0.002), side=0.398, speed=0.1):
    """n uniform points in a square of this side whose lower left corner is `lo`, velocities up to `speed` either way.
    By default the square stands on the floor -- the particles within 1.2 r of it are the walls' work, more of them
    after every growth of the radius -- and clear of the left wall: particles the hard wall fix puts on a vertical wall
    share x up to an ulp, and the order of two of them in one row, with it their slots in each other's lists, would
    hang on the last bit (force_cases.floor_pile)."""
    rs = np.random.RandomState(seed)
    return np.array(lo) + side * rs.rand(n, 2), (rs.rand(n, 2) - 0.5) * 2 * speed


# ------------------------------------------------------------------ the cases
RADIUS_STEPS = (1.0, 1.0, 0.75, 0.75, 0.93, 1.3, 1.3, 1.0, 1.0)    # the radius of every tick, in units of R


def radius_steps() -> EditCase:
    p, v = cloud()
    edits = {t: (coef_edit("particle_radius", R * f),) for t, f in enumerate(RADIUS_STEPS) if t and f != RADIUS_STEPS[t - 1]}
    return EditCase("radius_steps", [wc.BOX], [], G.lively(), p, v, len(RADIUS_STEPS), edits)


def _gravity_in_place(w: Hands) -> None:
    w.gravity[1] = -4.0


def every_coefficient() -> EditCase:
    p, v = cloud()
    # the source wants 60 particles at tick 0 and finds room for 40; at tick 1 the room is raised; from tick 2 on it rests
    sources = [G.source(0.2, (0.7, 0.7), (0.0, 0.0), 30000, active_ticks=2)]
    steps = (coef_edit("max_particles", 4000), coef_edit("dt", wc.DT * 0.7), coef_edit("wall_collision_decay", 0.9),
             coef_edit("pressure_amplifier", 12.0), coef_edit("ignored_pressure", 0.5), coef_edit("collider_noise_level", 0.2),
             coef_edit("viscosity", 9.0), coef_edit("surface_smoothing", 30.0), coef_edit("target_pressure", 0.5),
             coef_edit("gravity", [1.5, -9.8]), Edit("gravity[1]", _gravity_in_place))
    return EditCase("every_coefficient", [wc.BOX], sources, G.lively(max_particles=len(p) + 40), p, v, len(steps) + 1,
                    {t + 1: (e,) for t, e in enumerate(steps)})


LID_Y = COMB_Y = 3.6 * R       # no particle is within 1.2 r of the floor and of what hangs above it
LID = {"motored": {"name": "lid", "segments": [[[-0.1, 0.0], [0.1, 0.0]]], "position": [0.25, LID_Y],
                   "angular_velocity_func": "lambda t: 0.0"}}
COMB = {"free": {"name": "comb", "segments": [[[0.03 * k, 0.0], [0.03 * k + 0.02, 0.0]] for k in range(11)],
                 "position": [0.5, COMB_Y]}}
SPARE = wc.fixed(((0.4, 0.5), (0.6, 0.5)), name="spare")      # the 17th segment


def _floor_end_in_place(w: Hands) -> None:
    w.body("box").segments[0, 1, 1] = 0.0035                    # the floor's right end, in the array the cache holds


def _floor_replaced(w: Hands) -> None:
    seg = w.body("box").segments.copy()
    seg[0, 0, 1] = 0.002
    w.body("box").segments = seg                                # another array of equal shape


def _spin_lid(w: Hands) -> None:
    w.body("lid").angular_velocity_func = lambda t: 0.8


def _lift_comb(w: Hands) -> None:
    w.body("comb").center_velocity = np.array([0.02, 0.25])


def walls_edited() -> EditCase:
    rs = np.random.RandomState(41)
    n = 340
    p = np.column_stack((0.08 + 0.84 * rs.rand(n), (0.75 + 2.45 * rs.rand(n)) * R))   # within 1.2 r of what changes
    v = (rs.rand(n, 2) - 0.5) * 0.1
    edits = {1: (Edit("endpoint in place", _floor_end_in_place),),
             2: (Edit("segments replaced", _floor_replaced),),
             3: (Edit("lid appended", lambda w: w.bodies.append(w.new_body(LID))),),
             4: (Edit("comb appended", lambda w: w.bodies.append(w.new_body(COMB))),),
             5: (Edit("motor replaced", _spin_lid),),
             6: (Edit("free velocity set", _lift_comb),),
             7: (coef_edit("particle_radius", 0.9 * R),),
             8: (Edit("comb removed", lambda w: w.bodies.remove(w.body("comb"))),)}
    return EditCase("walls_edited", [wc.BOX], [], G.lively(gravity=[0.0, -9.8], pressure_amplifier=10.0), p, v, 10, edits)


WALLS_FULL_AT = 5            # a tick of walls_edited that starts with 16 segments


def _source_edit(k, name, value) -> Edit:
    return Edit(f"source {k} {name}", lambda w: setattr(w.sources[k], name, value))


EXTRA_SOURCE = G.source(0.06, (0.8, 0.3), (-0.3, 0.0), 3000)


def sources_edited() -> EditCase:
    p, v = cloud(seed=7, n=700, lo=(0.1, 0.1), side=0.2)
    sources = [G.source(0.06, (0.4, 0.6), (0.5, 0.0), 3000), G.source(0.07, (0.7, 0.7), (0.0, 0.0), 4000),
               G.source(0.06, (0.6, 0.3), (0.0, 0.3), 2500, noise=0.1)]
    edits = {1: (_source_edit(0, "position", [0.42, 0.62]),), 2: (_source_edit(1, "radius", 0.1),),
             3: (_source_edit(0, "velocity", [0.3, 0.2]),), 4: (_source_edit(1, "noise", 0.2),),
             5: (_source_edit(0, "flow", 5000),), 6: (_source_edit(1, "flow", 2000),),
             7: (_source_edit(2, "flow", 0),), 9: (_source_edit(2, "flow", 2500),),
             10: (_source_edit(1, "active_ticks", 10),),
             11: (Edit("source appended", lambda w: w.sources.append(w.new_source(EXTRA_SOURCE))),)}
    return EditCase("sources_edited", [wc.BOX], sources, G.lively(max_particles=3000), p, v, 13, edits)


FLOW_ZERO_TICKS = (7, 8)     # the ticks of sources_edited in which a source has flow 0


def dt_above_half() -> EditCase:
    coef = dict(wc.LIVELY, **fc.OFF)
    coef.update(dt=0.002, collider_noise_level=G.NOISE_LEVEL, max_particles=4000)
    sources = [G.source(0.5, (0.5, 0.5), (0.02, 0.01), DT_HALF_FLOW, noise=0.01)]
    edits = {3: (coef_edit("dt", 0.6),), 5: (coef_edit("dt", 0.002),)}
    return EditCase("dt_above_half", [wc.BOX], sources, coef, np.zeros((0, 2)), np.zeros((0, 2)), 7, edits,
                    forces_on=False, warns_at=(3,))


CASES = {"radius_steps": radius_steps, "every_coefficient": every_coefficient, "walls_edited": walls_edited,
         "sources_edited": sources_edited, "dt_above_half": dt_above_half}

# (case, tick, kind): the inputs of tick + 1 differ from those of `tick` in this kind of way
PROMISE_EDITS = (("radius_steps", 1, "radius smaller, past the allocation"),
                 ("radius_steps", 6, "radius smaller, inside the allocation"),
                 ("radius_steps", 4, "radius larger"),
                 ("every_coefficient", 6, "another coefficient"),
                 ("walls_edited", 0, "a moved wall"),
                 ("walls_edited", 2, "another segment count"))
PROMISE_SMALLER = PROMISE_EDITS[:2]     # ... which also run with the stream on the device


# ------------------------------------------------------------------ the grid, as build_world and ensure_cells have it
def grid_cells(radius: float) -> int:
    """build_world: the grid covers [-r, 1 + r]^2, three cells of margin and a ring of empty cells."""
    d = 2 * radius
    cmin, cmax = math.floor(-radius / d) - 3, math.floor((1 + radius) / d) + 3
    return (cmax - cmin + 1 + 2) ** 2


def grid_plan(radii):
    """Per tick (cells, workgroups of the scan, whether ensure_cells reallocates), from an empty context."""
    room, out = 0, []
    for radius in radii:
        cells = grid_cells(radius)
        grows = cells + 1 > room
        if grows:
            room = cells + 1 + cells // 4
        out.append((cells, (cells + 1 + SCAN_PER_BLOCK - 1) // SCAN_PER_BLOCK, grows))
    return out


# ------------------------------------------------------------------ the oracle side of a run
def eta_of(noise, ids, tick):
    """tick_core's eta_u01: nothing, counter noise by id and tick, or the next block of np.random."""
    if noise == "none":
        return None
    if noise == "counter":
        return G.counter_eta(ids, tick)
    return lambda total: np.random.rand(total, 2)


def oracle_tick(stage, tick, state, noise, nudge=None):
    """One tick as `physics_tick` orders it -- the sources emit, the bodies move, the particles outside leave, the
    tick, the free bodies accelerate -- on a stage whose edits are made: state = (p, v, ids, next_id) ->
    (state the tick computed on, state after, tick_core's dict, [(drawn, count)] per active source)."""
    p, v, ids, next_id = state
    emitted = []
    for drawn, pos, vel in stage.emit(tick, len(p)):
        k = 0 if pos is None else len(pos)
        emitted.append((drawn, k))
        if k:
            p, v = np.vstack((p, pos)), np.vstack((v, vel))
            ids = np.concatenate((ids, next_id + np.arange(k)))
            next_id += k
    stage.advance()
    p, v, ids = stage.remove(p, v, ids)
    if nudge is not None:
        p, v = nudge(p, v, ids)
    with np.errstate(all="ignore"):
        out = stage.core(p, v, eta_of(noise, ids, tick))
    stage.accelerate()
    return (p, v, ids), (out["particles"], out["velocities"], ids, next_id), out, emitted


def start_of(case):
    return np.array(case.p), np.array(case.v), np.arange(len(case.p), dtype=np.int64), len(case.p)


def distance(right, wrong) -> float:
    """`growth_cases.worst` between two ticks' results; infinite when they do not even hold the same particles."""
    (ids_a, out_a), (ids_b, out_b) = right, wrong
    if not np.array_equal(ids_a, ids_b):
        return float("inf")
    return G.worst(out_a, out_b)


def run(case: EditCase, noise="counter", stale=True, ulp=False):
    """The case on the oracle, np.random seeded as `Crate.__init__` seeds it.  Yields per tick a dict: tick, ids (of the
    particles the tick computes), out (tick_core's dict), emitted, coef and n_segments (as the tick had them), and -- `stale` -- stale:
    [(edit name, distance of the tick without that edit from the right one)], and -- `ulp` -- sensitivity:
    `force_cases.tick_sensitivity` of the tick against itself with every input one ulp away."""
    np.random.seed(0)
    stage = G.Stage(case.bodies, case.coef, case.sources)
    state = start_of(case)
    for t in range(case.ticks):
        found = np.random.get_state()
        before = copy.deepcopy(stage)
        case.apply(stage, t)
        edited = copy.deepcopy(stage)
        (p, v, ids), after, out, emitted = oracle_tick(stage, t, state, noise)
        left = np.random.get_state()
        rec = dict(tick=t, ids=ids, out=out, emitted=emitted, coef=dict(stage.coef, gravity=stage.coef["gravity"].copy()),
                   n_segments=len(stage.segments), stale=[], sensitivity=None)
        for k, edit in enumerate(case.edits_at(t) if stale else ()):
            other = copy.deepcopy(before)
            case.apply(other, t, without=k)
            np.random.set_state(found)
            (_, _, ids_k), _, out_k, _ = oracle_tick(other, t, state, noise)
            rec["stale"].append((edit.name, distance((ids, out), (ids_k, out_k))))
        if ulp:
            np.random.set_state(found)
            _, _, out_b, _ = oracle_tick(edited, t, state, noise, nudge=fc.one_ulp(1000 + t))
            rec["sensitivity"] = fc.tick_sensitivity(out, out_b, 2 * stage.coef["particle_radius"])
        np.random.set_state(left)
        yield rec
        state = after


def list_lengths(out, d):
    """The number of particles within d of each, uncut, on the positions the lists are made of."""
    p = out["fixed_positions"]
    if not len(p):
        return np.zeros(0, dtype=np.int64)
    diff = p[:, None, :] - p[None, :, :]
    return ((diff ** 2).sum(2) < d * d).sum(1) - 1
