"""Worlds in which a growth of the crate's GPU context decides the result (tests/test_gpu_growth.py,
tests/test_growth_cases_cpu.py).

The reference has no capacity; `Crate` has one, and `Crate._grow` replaces the context when the state outgrows it.  The
rule on top of every kernel rule: a run does not depend on the capacity the context happened to get.  What a hand-over
can lose without any kernel being wrong:
  ids        the state goes over renumbered 0..n-1; after a removal the real ids have gaps, and counter noise is keyed by id;
  the tick   the new context counts from 0: counter noise is keyed by the tick as well, and the logs stamp it;
  next_id    the ids handed out after the growth start again at n.
Each case is a world plus the capacities to run it at; `run` ticks it on the oracle with the crate's growth policy
(crate.py: `_create_new_particles`, `_grow`) and says, for every tick, what a context that lost the ids or the tick at
its last growth would have been given instead.

  sources_two_growths  two sources in the middle of the box and one near y = 1 that shoots outwards (gravity +y): its
                       particles leave within a few ticks, and as it is the first source its ids lie in front of the
                       tick's other ids -- every removal leaves a gap in the middle.  From capacity 16 the count passes
                       16 within 4 ticks and int(needed * 1.5) + 1024 within 16.  No static flow does both -- at most 16
                       particles in the first ticks, so at most 16 a tick, is at most 256 in 16 ticks -- so the wide
                       source is switched on after the first growth: `flow_steps`, an edit of `particle_sources[k].flow`
                       between ticks, as the viewer may make it.  The only wall is a short segment far outside (an
                       empty body list breaks `segments`): no particle reaches it, no order is ill-conditioned.
  exact_fit            max_particles equals the capacity equals a count the sources reach exactly: the last emission is
                       clipped by the room, later ones draw their binomial and emit nothing.  255, 256 and 257.
  set_state_growth     50 particles ticked 3 times, then `crate.particles =` 2,200 points, then more ticks.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field

import numpy as np

import force_cases as fc
import track_cases as tk
import wall_cases as wc
from oracle.tick import BodyState, counter_noise_key, counter_noise_u01, remove_outside, tick_core
from oracle.world import build_bodies, build_sources

SEED = 23            # counter noise: the context's seed
NOISE_LEVEL = 0.5    # collider_noise_level of every case: a wrong key or id moves a particle far beyond the tolerances
SHARP = 1000.0       # ... by at least this many times (test_growth_cases_cpu.py asserts it)
FIRST_CAPACITY = 16
EXACT_COUNTS = (255, 256, 257)
# (tick, capacity after) of the growths from capacity 16 with the sources' draws alone on np.random -- noise "none" and
# "counter"; test_growth_cases_cpu.py proves them on the oracle
TWO_GROWTHS = ((2, 1049), (10, 2770))    # sources_two_growths
EXACT_FIRST_GROWTH = (0, 1096)           # exact_fit: the very first emission, out of an empty context


def grown(needed: int) -> int:
    """The capacity of the context `Crate._grow(needed)` makes."""
    return int(needed * 1.5) + 1024


@dataclass
class GrowthCase:
    name: str
    bodies: list                 # rigid body configs, as in a scene's YAML
    sources: list                # particle source configs, as in a scene's YAML
    coef: dict
    ticks: int
    capacities: tuple            # the capacities to run at; the last one is ample (no growth)
    growths: dict                # capacity -> ((tick, capacity after), ...): the growths of a run that starts there
    flow_steps: dict = field(default_factory=dict)   # tick -> the sources' flows from that tick's emission on

    @property
    def ample(self) -> int:
        return self.capacities[-1]

    def flows_at(self, tick: int):
        """The flows to set before tick `tick` (the crate's `tick` attribute before `physics_tick`), or None."""
        return self.flow_steps.get(tick)


@dataclass
class SetStateCase:
    name: str
    bodies: list
    coef: dict
    first: tuple                 # (particles, velocities) the run starts with
    ticks_before: int
    second: np.ndarray           # the particles `crate.particles =` is given (velocities become zero: crate.py setter)
    ticks_after: int
    capacities: tuple            # (too small for `second`, ample)


def lively(**changes):
    coef = dict(wc.LIVELY, collider_noise_level=NOISE_LEVEL, gravity=[0.0, 9.8])
    coef.update(changes)
    return coef


def far_wall():
    return tk.wall_bodies(1)


def source(radius, position, velocity, flow, noise=0.05, active_ticks=10 ** 9):
    return dict(radius=radius, position=list(position), velocity=list(velocity), flow=flow, noise=noise,
                active_ticks=active_ticks)


def sources_two_growths() -> GrowthCase:
    r = wc.R
    sources = [
        # y in [0.985, 0.995], 0.016 a tick outwards: beyond 1 + r after one tick, the slowest after two
        source(0.01, (0.5, 0.99), (0.0, 8.0), 1500, noise=0.2),
        source(0.03, (0.5, 0.5), (0.0, 0.0), 2000),             # a tight clump: the first particles have neighbors
        source(0.3, (0.5, 0.45), (0.0, 0.0), 0),                # the crowd, switched on at tick 4
    ]
    assert 0.985 + 2 * wc.DT * 7.9 > 1 + r > 0.985 + wc.DT * 8.1
    return GrowthCase("sources_two_growths", far_wall(), sources, lively(max_particles=3000), ticks=16,
                      capacities=(FIRST_CAPACITY, 4096), growths={FIRST_CAPACITY: TWO_GROWTHS, 4096: ()},
                      flow_steps={4: (1500, 2000, 75000)})


def exact_fit(count: int) -> GrowthCase:
    sources = [source(0.1, (0.5, 0.5), (0.0, 0.0), 20000), source(0.05, (0.3, 0.5), (0.5, 0.0), 5000)]
    return GrowthCase(f"exact_fit_{count}", far_wall(), sources, lively(max_particles=count), ticks=9,
                      capacities=(FIRST_CAPACITY, count, count + 1024),
                      growths={FIRST_CAPACITY: (EXACT_FIRST_GROWTH,), count: (), count + 1024: ()})


def set_state_growth() -> SetStateCase:
    n, many = 50, 2200
    d = float(np.sqrt(6.0 / (np.pi * many)))                     # (discs sized for the crowd: six neighbors each)
    coef = lively(particle_radius=d / 2, dt=0.002 * (d / 0.01), max_particles=many, gravity=[1.5, -9.8])
    return SetStateCase("set_state_growth", far_wall(), coef, tk.cloud(2, n), 3, tk.cloud(3, many)[0], 4, (n, many + 64))


def cases() -> dict:
    out = {"sources_two_growths": sources_two_growths()}
    out.update({f"exact_fit_{n}": exact_fit(n) for n in EXACT_COUNTS})
    return out


# ------------------------------------------------------------------ the oracle side of a run
class Stage:
    """The host side of a world as the oracle has it: bodies, coefficients, and the emission rule.  `coef`, `bodies`
    and `sources` are read afresh by every call, so they may be edited between ticks (tests/edit_cases.py): a
    coefficient replaced, the gravity written in place, a body or a source changed, appended or removed."""

    def __init__(self, bodies, coef, sources=()):
        self.bodies = build_bodies(bodies)                       # (a list: it may grow and shrink)
        self.sources = build_sources(copy.deepcopy(list(sources)))
        self.coef = dict(coef)
        self.coef["gravity"] = np.array(self.coef["gravity"], dtype=np.float64)

    @property
    def segments(self):
        return np.vstack([b.segments for b in self.bodies])

    def body_states(self):
        return [BodyState(np.asarray(b.position, dtype=np.float64), np.asarray(b.center_velocity, dtype=np.float64),
                          float(b.angular_clockwise_velocity), len(b)) for b in self.bodies]

    def emit(self, tick: int, stored: int):
        """particle_source.py:17-24 for every active source in order, from the global generator, each seeing the room
        the previous ones left (crate.py:138-147): -> [(binomial drawn, positions, velocities) per active source];
        positions and velocities are None where nothing was emitted."""
        out = []
        for s in self.sources:
            if s.active_ticks <= tick:
                continue
            drawn = int(np.round(np.random.binomial(s.flow, self.coef["dt"])))
            count = min(drawn, self.coef["max_particles"] - stored)
            if count == 0:
                out.append((drawn, None, None))
                continue
            pos = (np.random.rand(count, 2) - 0.5) * s.radius + np.array(s.position)
            vel = np.ones_like(pos) * np.array(s.velocity)[None]
            vel += (np.random.rand(count, 2) - 0.5) * s.noise
            out.append((drawn, pos, vel))
            stored += count
        return out

    def advance(self) -> None:
        for b in self.bodies:
            b.advance(self.coef["dt"])

    def accelerate(self) -> None:
        """crate.py:311-314, behind the tick: gravity accelerates the bodies that are neither fixed nor motored."""
        for b in self.bodies:
            if b.kind == "free":
                b.center_velocity = b.center_velocity + self.coef["dt"] * np.asarray(self.coef["gravity"], dtype=np.float64)

    def remove(self, p, v, ids):
        return remove_outside(p, v, self.coef["particle_radius"], ids)

    def core(self, p, v, eta):
        """`tick_core` of a state after removal, with the bodies where they stand."""
        return tick_core(p, v, self.segments, self.body_states(), self.coef, eta_u01=eta)


def counter_eta(ids, tick: int):
    return counter_noise_u01(ids, counter_noise_key(SEED, tick))


def worst(right: dict, wrong: dict) -> float:
    """How far `wrong` is from `right`, in units of the suite's tolerances (force_cases.RTOL, ATOL), over particles and
    velocities: the largest |x - y| / (atol + rtol |x|)."""
    out = 0.0
    for key in ("particles", "velocities"):
        x, y = right[key], wrong[key]
        out = max(out, float((np.abs(x - y) / (fc.ATOL[key] + fc.RTOL * np.abs(x))).max(initial=0.0)))
    return out


def run(case: GrowthCase, capacity: int):
    """The case on the oracle with counter noise, growing as the crate grows from `capacity`.  Yields per tick a dict:
    tick, grew ((capacity after, ids stored at that moment, count that did not fit) per growth of this tick), emitted
    ([(drawn, count)] per source), removed (how many left), ids (of the particles the tick computes), out (tick_core's
    dict), capacity, and -- None before the first growth -- out_old_key: the same tick with the key of a context that
    started counting at the last growth, out_renumbered: with the ids of a context that renumbered the particles 0..n-1
    at the last growth and handed out n, n + 1, .. since."""
    np.random.seed(0)                                            # Crate.__init__ (crate.py:22)
    stage = Stage(case.bodies, case.coef, case.sources)
    p, v = np.zeros((0, 2)), np.zeros((0, 2))
    ids = np.zeros(0, dtype=np.int64)
    next_id = 0
    lost_ids, lost_next, lost_tick0 = ids, 0, None               # what the forgetful context holds
    for t in range(case.ticks):
        flows = case.flows_at(t)
        if flows is not None:
            for s, f in zip(stage.sources, flows):
                s.flow = f
        grew, emitted = [], []
        for drawn, pos, vel in stage.emit(t, len(p)):
            k = 0 if pos is None else len(pos)
            emitted.append((drawn, k))
            if not k:
                continue
            if len(p) + k > capacity:                            # crate.py: _create_new_particles, the host's emission
                capacity = grown(len(p) + k)
                grew.append((capacity, ids.copy(), len(p) + k))
                lost_ids, lost_next, lost_tick0 = np.arange(len(p), dtype=np.int64), len(p), t
            p, v = np.vstack((p, pos)), np.vstack((v, vel))
            ids = np.concatenate((ids, next_id + np.arange(k)))
            lost_ids = np.concatenate((lost_ids, lost_next + np.arange(k)))
            next_id, lost_next = next_id + k, lost_next + k
        stage.advance()
        lost_ids = stage.remove(p, v, lost_ids)[2]
        stored = len(p)
        p, v, ids = stage.remove(p, v, ids)
        out = stage.core(p, v, counter_eta(ids, t))
        old_key = renumbered = None
        if lost_tick0 is not None:
            old_key = stage.core(p, v, counter_eta(ids, t - lost_tick0))
            renumbered = stage.core(p, v, counter_eta(lost_ids, t))
        yield dict(tick=t, grew=grew, emitted=emitted, removed=stored - len(p), ids=ids, out=out, capacity=capacity,
                   out_old_key=old_key, out_renumbered=renumbered)
        p, v = out["particles"], out["velocities"]


def run_set_state(case: SetStateCase):
    """The case on the oracle with counter noise: yields per tick (tick, out, out_old_key); out_old_key is None before
    the state is replaced, and afterwards the tick with the key of a context that started counting there."""
    stage = Stage(case.bodies, case.coef)
    p, v = case.first
    t = 0
    for phase, ticks in enumerate((case.ticks_before, case.ticks_after)):
        if phase:
            p, v = case.second, np.zeros_like(case.second)
        ids = np.arange(len(p), dtype=np.int64)                  # an upload numbers from 0
        for _ in range(ticks):
            stage.advance()
            p, v, ids = stage.remove(p, v, ids)
            out = stage.core(p, v, counter_eta(ids, t))
            old_key = stage.core(p, v, counter_eta(ids, t - case.ticks_before)) if phase else None
            yield t, out, old_key
            p, v = out["particles"], out["velocities"]
            t += 1
