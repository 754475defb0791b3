"""GPU tests of the edit rule: a tick depends on the inputs as they stand when it starts, and on nothing an earlier
tick was given (the worlds are tests/edit_cases.py, their premises tests/test_edit_cases_cpu.py).

A crate whose radius, coefficients, gravity, walls and sources are edited between ticks -- the grid reallocated, changed
inside its allocation and shrunk; an endpoint written in place, a `segments` array replaced, bodies appended and
removed; a flow set to 0 and a dt above one half -- is compared tick by tick with the oracle restarted from the device's
previous state and given the same edits; with the stream on the device, byte for byte with a twin whose host draws it;
driven by `engine.tick(now, next)` across an edit and by `run` between edits, byte for byte with a twin driven by
`physics_tick`; and, back at the first radius, byte for byte with a crate that never saw another.

Slab contexts are out of scope: their cuts are counted in cells of the diameter and are chosen once."""
import copy
import warnings

import numpy as np
import pytest

import edit_cases as E
import force_cases as fc
import gpu_support as U
import growth_cases as G
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = {name: build() for name, build in E.CASES.items()}


def make_crate(sc, case, noise):
    wc = sc.WorldConfig(rigid_bodies=copy.deepcopy(case.bodies), particle_sources=copy.deepcopy(case.sources),
                        coefficients=copy.deepcopy(case.coef))
    crate = sc.Crate(wc, noise=noise, noise_seed=G.SEED)          # (seeds np.random, crate.py:22)
    if len(case.p):
        crate.particles = np.array(case.p)
        crate.particle_velocities = np.array(case.v)
    return crate


def same_stream(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1])


def ticked(crate, case, before=None):
    """One `physics_tick` of the case: the tick's edits first.  -> whether the crate warned."""
    if before is not None:
        before(crate, crate.tick)
    case.apply(crate, crate.tick)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        crate.physics_tick()
    ours = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert all("sand_crate_amd" in str(w.message) and "host-sync" in str(w.message) for w in ours), ours
    return len(ours)


# ------------------------------------------------------------------ every tick against the oracle
def run_against_oracle(sc, case, noise, before=None):
    """The case on a crate, every tick against one oracle tick restarted from the device's previous state: ids, counts
    and removals exact, floats within the suite's tolerances; the oracle draws the sources (and the host-drawn noise)
    from the generator as the crate found it -- on the device, where the crate holds it there -- and must leave it
    where the crate left it.  `before(crate, tick)` runs before the tick's edits."""
    crate = make_crate(sc, case, noise)
    stage = G.Stage(case.bodies, case.coef, case.sources)
    state = E.start_of(case)
    warned = []
    for t in range(case.ticks):
        crate.sync_host_rng()                                     # (noise="host": np.random goes where the device stands)
        found = np.random.get_state()
        warned += [t] * ticked(crate, case, before)
        crate.sync_host_rng()
        left = np.random.get_state()
        np.random.set_state(found)
        case.apply(stage, t)
        drawn = "host-sync" if noise == "host" else noise
        (p, v, ids), state, out, _ = E.oracle_tick(stage, t, state, drawn)
        where = f"{case.name}, noise {noise}, tick {t}"
        assert same_stream(np.random.get_state(), left), f"{where}: the crate drew another stretch of np.random"
        gp, gv, gpr, gids = crate.engine.download()
        assert np.array_equal(gids, ids), where                   # ids, counts and removals: exact
        assert crate.particle_count == len(ids) and crate.tick == t + 1, where
        assert crate.measure()["tick"] == t + 1, where            # the context's own tick number
        np.testing.assert_allclose(gp, out["particles"], rtol=fc.RTOL, atol=fc.ATOL["particles"], err_msg=where)
        np.testing.assert_allclose(gv, out["velocities"], rtol=fc.RTOL, atol=fc.ATOL["velocities"], err_msg=where)
        np.testing.assert_allclose(gpr, out["pressure"], rtol=fc.RTOL, atol=fc.ATOL["pressure"], err_msg=where)
        state = (gp, gv, ids, state[3])
    assert tuple(warned) == (case.warns_at if noise == "host" else ()), where
    assert crate._noise == ("host-sync" if noise == "host" and case.warns_at else noise)
    crate.close()


@pytest.mark.parametrize("noise", E.NOISES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_tick_matches_the_oracle(sc, name, noise):
    run_against_oracle(sc, CASES[name], noise)


def test_a_17th_segment_is_refused_and_the_run_goes_on(sc):
    """One segment more than the library takes: `physics_tick` raises its capacity error before anything has changed --
    no source has emitted, no body has moved, the state, its ids and both tick numbers are what they were -- and with
    the body taken away again the run goes on and matches the oracle to its end."""
    from sand_crate_amd import _native as N
    case = CASES["walls_edited"]
    seen = []

    def before(crate, tick):
        if tick != E.WALLS_FULL_AT:
            return
        assert len(crate.segments) == E.MAX_SEGMENTS
        state = crate.engine.download()
        walls, times = crate.segments.copy(), [getattr(b, "time_from_start", None) for b in crate.rigid_bodies]
        crate.rigid_bodies.append(E.Hands(crate).new_body(E.SPARE))
        assert U.code_of(crate.physics_tick) == N.ERR_CAPACITY
        spare = crate.rigid_bodies.pop()
        assert spare.name == "spare"
        assert crate.tick == tick and crate.measure()["tick"] == tick
        for a, b in zip(state, crate.engine.download()):
            U.same_bytes(a, b)
        U.same_bytes(walls, crate.segments)
        assert times == [getattr(b, "time_from_start", None) for b in crate.rigid_bodies]
        seen.append(tick)

    run_against_oracle(sc, case, "counter", before)
    assert seen == [E.WALLS_FULL_AT]


# ------------------------------------------------------------------ the stream on the device against the host's
class Streams:
    """Two crates that both draw from np.random take turns at it: each finds it where it left it."""

    def __init__(self):
        self.at = {}

    def turn(self, key, call):
        if key in self.at:
            np.random.set_state(self.at[key])
        out = call()
        self.at[key] = np.random.get_state()
        return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_stream_equals_the_host_drawn_twin(sc, name):
    """noise="host" against noise="host-sync" with the same edits: byte for byte after every tick, and the device's
    stream ends where the twin's np.random stands.  In dt_above_half the device refuses binomial(n, 0.6): the crate
    warns once, at tick 3, and goes on in "host-sync" -- equal to the twin, so the refused emission drew nothing.  A
    flow of 0 is drawn on the device: no warning, the mode stays."""
    case = CASES[name]
    streams = Streams()
    device = make_crate(sc, case, "host")
    twin = streams.turn("twin", lambda: make_crate(sc, case, "host-sync"))
    warned = []
    for t in range(case.ticks):
        if device._noise == "host":
            warned += [t] * ticked(device, case)
            if device._noise != "host":                           # (it fell back: from here on it draws from np.random)
                streams.at["device"] = np.random.get_state()
        else:
            warned += [t] * streams.turn("device", lambda: ticked(device, case))
        assert streams.turn("twin", lambda: ticked(twin, case)) == 0
        for a, b in zip(device.engine.download(), twin.engine.download()):
            U.same_bytes(a, b, f"{name}, tick {t}")
        assert device._noise == ("host-sync" if case.warns_at and t >= case.warns_at[0] else "host"), t
    assert tuple(warned) == case.warns_at
    assert device.particle_count == twin.particle_count > 200
    if device._noise == "host":
        device.sync_host_rng()
        streams.at["device"] = np.random.get_state()
    assert same_stream(streams.at["device"], streams.at["twin"])
    draws = [streams.turn(key, lambda: np.random.rand(5)) for key in ("device", "twin")]
    U.same_bytes(*draws)
    device.close()
    twin.close()


# ------------------------------------------------------------------ the promise across an edit
def promised_pair(crate, case):
    """Ticks `crate.tick` and the one after it as `Crate.run` drives two ticks -- `engine.tick(now, next)`, then
    `engine.tick(next)` -- with the second tick's edits made between the packing of `now` and of `next`."""
    t = crate.tick
    case.apply(crate, t)
    crate._create_new_particles()                                 # (the sources of these ticks rest, or find no room)
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    now = crate._pack_tick_inputs()
    crate._accelerate_free_bodies()
    case.apply(crate, t + 1)
    crate._create_new_particles()
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    nxt = crate._pack_tick_inputs()
    crate.engine.tick(now, nxt)
    crate._accelerate_free_bodies()
    crate.engine.tick(nxt)
    crate.tick += 2
    crate._state_changed()


def promise_run(sc, case, at, noise, promised):
    crate = make_crate(sc, case, noise)
    assert not crate._hud_forces and crate._trajectory is None    # (the monitor and the logs, which disable fusion, stay off)
    states = []
    while crate.tick < case.ticks:
        if promised and crate.tick == at:
            promised_pair(crate, case)
        else:
            assert ticked(crate, case) == 0
        states.append((crate.tick, crate.engine.download()))
    assert crate._noise == noise and crate.measure()["tick"] == case.ticks
    crate.close()
    return states


PROMISES = [(name, t, kind, noise) for name, t, kind in E.PROMISE_EDITS for noise in ("counter", "none")] + \
           [(name, t, kind, "host") for name, t, kind in E.PROMISE_SMALLER]


@pytest.mark.parametrize("name,at,kind,noise", PROMISES, ids=[f"{n}-{t}-{z}" for n, t, _, z in PROMISES])
def test_a_promise_across_an_edit_equals_two_plain_ticks(sc, name, at, kind, noise):
    """`engine.tick(now, next)` with `next` packed behind the edit: the crate is byte for byte the twin that made one
    `physics_tick` per tick, at the promised tick and to the end of the case.  With noise="host" the stream is on the
    device, and pass A's density launch follows the reallocation in the middle of the tick."""
    case = CASES[name]
    got = promise_run(sc, case, at, noise, True)
    want = promise_run(sc, case, at, noise, False)
    assert [t for t, _ in got] == [t for t, _ in want if t != at + 1] and (at + 2) in [t for t, _ in got]
    twin = dict(want)
    for t, state in got:
        for a, b in zip(state, twin[t]):
            U.same_bytes(a, b, f"{name}, {kind}, noise {noise}, after tick {t - 1}")
    if noise == "host":     # (the twin is the crate of test_every_tick_matches_the_oracle)
        return
    # ... and the promised tick is the oracle's, restarted from the state the tick before it left
    np.random.seed(0)
    stage = G.Stage(case.bodies, case.coef, case.sources)
    state = E.start_of(case)
    for t in range(at + 1):                                       # (the oracle's bodies, sources and next id, up to here)
        case.apply(stage, t)
        _, state, _, _ = E.oracle_tick(stage, t, state, noise)
    gp, gv, _, gids = twin[at + 1]
    case.apply(stage, at + 1)
    (_, _, ids), _, out, _ = E.oracle_tick(stage, at + 1, (gp, gv, gids, state[3]), noise)
    gp, gv, gpr, gids = dict(got)[at + 2]
    assert np.array_equal(gids, ids) and len(ids) > 200
    np.testing.assert_allclose(gp, out["particles"], rtol=fc.RTOL, atol=fc.ATOL["particles"])
    np.testing.assert_allclose(gv, out["velocities"], rtol=fc.RTOL, atol=fc.ATOL["velocities"])
    np.testing.assert_allclose(gpr, out["pressure"], rtol=fc.RTOL, atol=fc.ATOL["pressure"])


# ------------------------------------------------------------------ `run` between edits
def run_between_edits(sc, case, use_run):
    crate = make_crate(sc, case, "counter")
    states = []
    while crate.tick < case.ticks:
        t = crate.tick
        if not use_run or case.sources_active(t):
            assert ticked(crate, case) == 0
        else:
            k = 1
            while t + k < case.ticks and not case.edits_at(t + k):
                k += 1
            case.apply(crate, t)
            crate.run(k)
        states.append((crate.tick, crate.engine.download()))
    crate.close()
    return states


@pytest.mark.parametrize("name", ["radius_steps", "every_coefficient", "walls_edited"])
def test_run_between_edits_equals_physics_tick(sc, name):
    case = CASES[name]
    got, want = run_between_edits(sc, case, True), dict(run_between_edits(sc, case, False))
    assert len(want) == case.ticks and got[-1][0] == case.ticks
    assert len(got) < len(want) or name == "every_coefficient"   # (elsewhere some stretches are longer than a tick)
    for t, state in got:
        for a, b in zip(state, want[t]):
            U.same_bytes(a, b, f"{name}, after tick {t - 1}")


# ------------------------------------------------------------------ back where it was
def test_back_at_the_first_radius_nothing_of_the_other_grids_is_left(sc):
    """After radius_steps the radius is R again: three more ticks equal, byte for byte, three ticks of a fresh crate
    that was given the state with its ids, the tick number and the next id, and never saw another radius -- nothing of
    the other grids is left in stamps, counts or hints."""
    case = CASES["radius_steps"]
    crate = make_crate(sc, case, "counter")
    while crate.tick < case.ticks:
        assert ticked(crate, case) == 0
    assert crate.particle_radius == E.R == case.coef["particle_radius"]
    p, v, _, ids = crate.engine.download()
    fresh = make_crate(sc, case, "counter")
    fresh.engine.upload_with_ids(p, v, ids)
    fresh.engine.restore_counters(case.ticks, len(case.p))
    fresh._state_changed(len(ids))
    assert len(ids) > 2000 and fresh.measure()["tick"] == case.ticks
    for k in range(3):
        crate.physics_tick()
        fresh.physics_tick()
        for a, b in zip(crate.engine.download(), fresh.engine.download()):
            U.same_bytes(a, b, f"tick {case.ticks + k}")
    crate.close()
    fresh.close()
