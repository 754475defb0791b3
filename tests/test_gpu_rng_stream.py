"""NumPy's legacy stream on the device (noise="host", csrc/sc_rng.h) pinned to `np.random` where the scene tests do
not reach: the emission kernel against NumPy draw for draw over inversion and every BTPE branch (tests/rng_cases.py)
and over more sources than one launch takes; the collider noise of worlds past the small-world kernel
(k_rng_noise after the id count and scan) against the oracle; a run whose id bound crosses that kernel's limit, and a
world of twelve sources, against the host-drawn stream."""
import copy
import time

import numpy as np
import pytest

from gpu_support import sc  # noqa: F401
from rng_cases import CALLS, SWEEP, mixed_sources, numpy_emit, seed_of, source
from test_gpu_parity import bench_like_crate, synthetic, wave_world
from test_gpu_round2 import pile_up_state

pytestmark = pytest.mark.gpu

SMALL_IDS = 1 << 16  # sc_rng.h kSmallIds: the host's id bound up to which one launch takes the noise offsets and draws


def assert_same_state(eng, rs):
    key, pos = eng.rng_get_state()
    _, want_key, want_pos, _, _ = rs.get_state()
    assert pos == want_pos and np.array_equal(key, want_key)


def fresh_engine(sc, rs, capacity):
    eng = sc.Engine(capacity)
    _, key, pos, _, _ = rs.get_state()
    eng.rng_set_state(key, pos)
    return eng


def check_emission(eng, rs, sources, dt, max_particles, stored, next_id):
    """One emit call on the device against `numpy_emit`: the new particles' positions, velocities and ids, bit for
    bit.  -> (stored, next_id, spec) after the call."""
    spec = numpy_emit(rs, sources, dt, stored, max_particles)
    eng.emit_particles(sources, dt, max_particles)
    new = [(p, v) for _, p, v in spec if p is not None]
    count = sum(len(p) for p, _ in new)
    xy, vxy, _, ids = eng.download(room=stored + count)
    assert len(ids) == stored + count
    if count:
        want_p = np.vstack([p for p, _ in new])
        want_v = np.vstack([v for _, v in new])
        assert np.array_equal(ids[stored:], next_id + np.arange(count))
        assert np.array_equal(xy[stored:], want_p)
        assert np.array_equal(vxy[stored:], want_v)
    return stored + count, next_id + count, spec


# ------------------------------------------------------------------ A: k_rng_emit against np.random
@pytest.mark.parametrize("flow,dt", SWEEP)
def test_emission_equals_numpy_over_the_sweep(sc, flow, dt):
    """CALLS calls of one source: every count, position, velocity and id as NumPy draws them, then the stream state.
    The store is emptied (ids start again at 0) whenever the next call might not fit."""
    rs = np.random.RandomState(seed_of(flow, dt))
    cap = 1 << 17
    eng = fresh_engine(sc, rs, cap)
    src = [source(flow, radius=0.07, position=(0.3, 0.6), velocity=(1.5, -0.25), noise=0.2)]
    bound = min(flow, flow * dt + 10 * np.sqrt(flow * dt * (1 - dt) + 1))
    stored = next_id = 0
    for _ in range(CALLS):
        if stored + bound > cap:
            eng.upload(np.zeros((0, 2)), np.zeros((0, 2)))
            stored = next_id = 0
        stored, next_id, _ = check_emission(eng, rs, src, dt, 10 ** 9, stored, next_id)
    assert_same_state(eng, rs)
    eng.close()


@pytest.mark.parametrize("n_sources", [2, 8, 9, 17])
def test_many_sources_in_one_call(sc, n_sources):
    """Sources in order, each seeing the room the previous ones left: max_particles binds at a different place of the
    list from call to call, the sources after it draw their binomial only; one call finds the store over max_particles
    (negative room).  Nine and seventeen sources take two and three launches (sc_emit_particles groups them by
    eight)."""
    rs = np.random.RandomState(500 + n_sources)
    eng = fresh_engine(sc, rs, 1 << 17)
    srcs = mixed_sources(n_sources)
    dt = 0.002
    expected = sum(s.flow * dt for s in srcs)
    stored = next_id = 0
    capped = starved = beyond_first_launch = 0
    for call in range(40):
        room = (0.15, 0.4, 0.65, 0.9, 1.2)[call % 5] * expected
        max_particles = stored - 5 if call == 20 else stored + int(room) + 1
        stored, next_id, spec = check_emission(eng, rs, srcs, dt, max_particles, stored, next_id)
        emitted = [0 if p is None else len(p) for _, p, _ in spec]
        capped += any(0 < e < x for (x, _, _), e in zip(spec, emitted))
        starved += any(x > 0 and e == 0 for (x, _, _), e in zip(spec[1:], emitted[1:]))
        beyond_first_launch += any(emitted[8:])
    assert capped > 10 and starved >= 5
    assert n_sources <= 8 or beyond_first_launch > 10
    assert_same_state(eng, rs)
    eng.close()


def test_emission_argument_errors(sc):
    """flow < 0, dt <= 0 and dt > 0.5 are outside the device's binomial (SC_ERR_DOMAIN, nothing drawn); dt = 0.5 is
    inside, and so is a flow of 0 -- a flow slider at its stop: one double, no particle, as NumPy draws binomial(0, p)."""
    from sand_crate_amd import _native as N
    rs = np.random.RandomState(3)
    eng = fresh_engine(sc, rs, 4096)
    for flows, dt in (([-1], 0.002), ([-3], 0.002), ([7000, -1], 0.002), ([10], 0.0), ([10], -0.1), ([10], 0.5000001),
                      ([0], 0.75), ([10] * 9, 0.75)):
        with pytest.raises(N.NativeError) as err:
            eng.emit_particles([source(f) for f in flows], dt, 10 ** 6)
        assert err.value.code == N.ERR_DOMAIN
    assert eng.count() == 0
    assert_same_state(eng, rs)
    one_double = np.random.RandomState()
    one_double.set_state(rs.get_state())
    one_double.random_sample()
    stored, next_id, spec = check_emission(eng, rs, [source(0)], 0.002, 10 ** 6, 0, 0)
    assert (stored, next_id) == (0, 0) and spec[0][0] == 0
    assert rs.get_state()[2] == one_double.get_state()[2] and np.array_equal(rs.get_state()[1], one_double.get_state()[1])
    assert_same_state(eng, rs)
    stored, next_id, spec = check_emission(eng, rs, [source(7000), source(0), source(90)], 0.002, 10 ** 6, 0, 0)
    assert stored > 0 and spec[1][1] is None
    assert_same_state(eng, rs)
    stored, next_id, _ = check_emission(eng, rs, [source(13), source(0), source(2000)], 0.5, 10 ** 6, stored, next_id)
    check_emission(eng, rs, mixed_sources(12), 0.002, 10 ** 6, stored, next_id)
    assert_same_state(eng, rs)
    eng.close()


# ------------------------------------------------------------------ C: the large-world noise chain against the oracle
def host_noise_ticks(sc, crate, wc, p, v, ids, ticks):
    """`ticks` ticks of a crate in noise="host", each against the oracle restarted from the GPU's state, its collider
    noise drawn from np.random (which the oracle seeded like the crate); then the stream position.  -> the wall time
    of each tick in ms."""
    from oracle.scene import OracleCrate
    from oracle.tick import remove_outside, tick_core
    from oracle.world import World
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))  # np.random.seed(0), as the crate did
    ms = []
    for _ in range(ticks):
        t0 = time.perf_counter()
        crate.physics_tick()
        crate.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        p, v, ids = remove_outside(p, v, orc.coef["particle_radius"], ids)
        out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef,
                        eta_u01=lambda total: np.random.rand(total, 2))  # crate.py:169, in id order
        gp, gv, gpr, gids = crate.engine.download()
        assert np.array_equal(gids, ids)
        np.testing.assert_allclose(gp, out["particles"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gv, out["velocities"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(gpr, out["pressure"], rtol=1e-9, atol=1e-12)
        p, v = gp, gv
    want = np.random.rand(4)
    crate.sync_host_rng()
    assert np.array_equal(np.random.rand(4), want)
    return ms


@pytest.mark.parametrize("n", [SMALL_IDS, SMALL_IDS + 1])
def test_host_noise_on_both_sides_of_the_small_world_kernel(sc, n):
    """65,536 ids take k_rng_noise_small, one more takes the id count, the scan and k_rng_noise: the same particles
    (the first n of one seeded draw, one diameter) and the oracle's stream."""
    p, v, d = synthetic(SMALL_IDS + 1, seed=65)
    p, v = p[:n], v[:n]
    d = float(np.sqrt(12 / (np.pi * SMALL_IDS)))
    wc = wave_world(sc, d, 0.1)
    wc.coefficients["max_particles"] = n
    crate = sc.Crate(wc, noise="host", capacity=n + 64)
    crate.particles = p
    crate.particle_velocities = v
    host_noise_ticks(sc, crate, wc, p, v, np.arange(n), 3)


@pytest.mark.parametrize("tile", ["wide", "narrow"])
def test_host_noise_at_262144_particles(sc, tile, monkeypatch):
    """bench.py's M2 world at 262,144 particles in the default noise mode, with the wide pass A tile the grid size
    picks and with the narrow one (host-mode density pass k_pass_a<SC_NOISE_HOST, false, true, kTileCapA>)."""
    monkeypatch.setenv("SANDCRATE_TILE", tile)  # read by sc_create
    n = 262144
    crate, wc, p, v, d = bench_like_crate(sc, n, noise="host")
    ms = host_noise_ticks(sc, crate, wc, p, v, np.arange(n), 2)
    print(f"\n262,144 particles, noise='host', {tile} tile: ticks took {', '.join(f'{t:.2f}' for t in ms)} ms (wall)")


def test_host_noise_with_sparse_ids(sc):
    """About 20,000 particles uploaded with their ids spread up to 10^6 in random storage order: a large id table of
    mostly zero counts, the offsets scanned over all of it, the noise drawn in id order."""
    n = 20000
    p, v, d = synthetic(n, seed=7)
    rs = np.random.RandomState(8)
    ids = np.sort(rs.choice(10 ** 6 - 1, n - 1, replace=False))
    ids = np.append(ids, 10 ** 6 - 1)
    wc = wave_world(sc, d, 0.1)
    wc.coefficients["max_particles"] = n
    crate = sc.Crate(wc, noise="host", capacity=n + 64)
    perm = rs.permutation(n)
    crate.engine.upload_with_ids(p[perm], v[perm], ids[perm])
    host_noise_ticks(sc, crate, wc, p, v, ids, 3)


def test_host_noise_pile_up_past_the_small_world_kernel(sc):
    """The pile-up state with uniform filler to 70,000-odd particles, with the noise of the large chain: big buckets
    (sorted, and grouped by the scatter, on the second tick) and tiles past the LDS budget.  (Host noise runs pass B
    unfused, which has no grouped variant.)"""
    d = 0.012
    p, v = pile_up_state(d)
    rs = np.random.RandomState(31)
    fill = 56000
    p = np.vstack((p, rs.rand(fill, 2) * 0.96 + 0.02))
    v = np.vstack((v, (rs.rand(fill, 2) - 0.5) * 0.1))
    perm = rs.permutation(len(p))
    p, v = p[perm], v[perm]
    n = len(p)
    assert n > SMALL_IDS
    wc = wave_world(sc, d, 0.1)
    wc.coefficients["max_particles"] = n
    crate = sc.Crate(wc, noise="host", capacity=n + 64)
    crate.particles = p
    crate.particle_velocities = v
    host_noise_ticks(sc, crate, wc, p, v, np.arange(n), 2)


# ------------------------------------------------------------------ D: device stream against the host-drawn one
def device_against_host_drawn(sc, wc, ticks, setup=None):
    runs = []
    for noise in ("host", "host-sync"):
        crate = sc.Crate(copy.deepcopy(wc), noise=noise)  # seeds np.random (crate.py:22)
        if setup is not None:
            setup(crate)
        for _ in range(ticks):
            crate.physics_tick()
        out = crate.engine.download()
        crate.sync_host_rng()
        runs.append((out, np.random.rand(4), crate))
    (a, after_a, dev), (b, after_b, ref) = runs
    assert dev._noise == "host"
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(after_a, after_b)
    return a


def test_id_bound_crosses_the_small_world_limit_mid_run(sc):
    """64,000 particles and two sources emitting ~56 a tick: the host's id bound (the real ids plus up to a few ticks'
    restart bounds, ~160 each) starts under 65,536 and passes it within the run, and the noise moves from
    k_rng_noise_small to the scanned chain in the middle of it."""
    n = 64000
    p, v, d = synthetic(n, seed=41)
    wc = wave_world(sc, d, 0.1)
    wc.coefficients["max_particles"] = n + 5000
    wc.particle_sources = [dict(radius=0.05, position=[0.3, 0.8], velocity=[1.0, 0.0], flow=30000, noise=0.02,
                                active_ticks=10 ** 9),
                           dict(radius=0.03, position=[0.7, 0.8], velocity=[-1.0, 0.0], flow=7000, noise=0.05,
                                active_ticks=10 ** 9)]

    def setup(crate):
        crate.particles = p
        crate.particle_velocities = v

    out = device_against_host_drawn(sc, wc, 40, setup)
    assert out[3].max() >= SMALL_IDS + 100  # (the real ids crossed too)


def test_twelve_sources_against_the_host_drawn_stream(sc):
    """Twelve sources (two launches of the emission kernel), inversion and BTPE, six of them expiring mid-run, and
    max_particles binding: 100 ticks as the host draws them."""
    wc = sc.load_config("config/wave_machine.yaml").world_config
    wc.coefficients["max_particles"] = 1500
    flows = (7000, 20000, 100, 22500, 15000, 100000, 1, 14999, 30000, 2000, 40000, 5000)
    wc.particle_sources = [dict(radius=0.02 + 0.01 * k, position=[0.1 + 0.07 * k, 0.9 - 0.02 * k],
                                velocity=[2.0 - 0.4 * k, 0.1 * k], flow=f, noise=0.01 * (k + 1),
                                active_ticks=(10 ** 9, 30, 60, 10 ** 9)[k % 4])
                           for k, f in enumerate(flows)]
    out = device_against_host_drawn(sc, wc, 100)
    assert 1000 < len(out[3]) <= 1500
