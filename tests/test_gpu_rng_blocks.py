"""The device's NumPy stream (csrc/sc_rng.h) at the borders of its 624-word blocks: the cases of tests/rng_block_cases.py
-- what each of them meets is proved in tests/test_rng_block_cases_cpu.py -- on the kernels.

  noise     every named case through `k_rng_noise_small` (ids up to 65,536) and through the scanned chain (the id count,
            the two-level scan, `k_rng_noise`: the same world with its top id at 65,536), which of the two asserted from
            the timing counters: the stream state after the tick is NumPy's after rand(P, 2), and the tick's result is,
            bit for bit, that of a twin context that is handed NumPy's block; the border cases also against the oracle;
  id scan   `k_rng_noise_small` at the id bounds where its threads' run length changes, against NumPy, the twin and
            the scanned chain;
  emission  `k_rng_emit` from positions on both sides of the border against NumPy call by call, one launch and two;
  runs      a crate from an odd position against the host-drawn stream, and through a checkpoint."""
import json

import numpy as np
import pytest

import gpu_support as U
import rng_block_cases as K
from gpu_support import sc  # noqa: F401
from test_gpu_parity import wave_world
from test_gpu_rng_stream import check_emission

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, dict(particles=1e-12, velocities=1e-11, pressure=1e-12)  # test_gpu_rng_stream.host_noise_ticks


def engine_ticks(sc, world: K.World, start: int, ticks: int, device_stream: bool):
    """`ticks` ticks of `world` at engine level (the pattern of test_gpu_round2's straddle test): with `device_stream`
    the context holds the stream (K.KEY, start) and draws the tick's block itself; without, it is handed the block
    NumPy draws from that state.  -> per tick dict(out, rows, block, state, want, launches): the downloaded state, P
    as sc_step_stats counts it, NumPy's rand(P, 2), the device's stream state after the tick (None for the twin),
    NumPy's, and how many noise_offsets brackets the tick took."""
    wc = wave_world(sc, K.D, K.NOISE_LEVEL)
    crate = sc.Crate(wc, noise="host-sync", capacity=len(world.p) + 64)
    eng = crate.engine
    rs = K.numpy_state(start)
    if device_stream:
        eng.rng_set_state(K.KEY, start)
    eng.upload_with_ids(*world.stored())
    eng.enable_timing(True)
    out = []
    for _ in range(ticks):
        for b in crate.rigid_bodies:
            b.apply_velocity(crate.dt)
        crate._send_tick_inputs()
        eng.reset_timing()
        eng.step_begin()
        rows = eng.step_stats().neighbor_slots
        block = rs.rand(rows, 2)
        if not device_stream:
            eng.set_noise_host(block)
        eng.step_finish()
        state = eng.download()
        _, key, pos, _, _ = rs.get_state()
        out.append(dict(out=state, rows=rows, block=block, state=eng.rng_get_state() if device_stream else None,
                        want=(key.copy(), int(pos)), launches=eng.timing()["noise_offsets"][1]))
    crate.close()
    return out


def assert_stream(tick: dict) -> None:
    (key, pos), (want_key, want_pos) = tick["state"], tick["want"]
    assert pos == want_pos
    assert np.array_equal(key, want_key)


def assert_same_bytes(a, b) -> None:
    for x, y in zip(a, b):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


def on_chain(world: K.World, chain: str) -> K.World:
    return world if chain == "small" else world.with_top_id(K.SMALL_IDS)


def assert_chain(tick: dict, chain: str) -> None:
    """One bracket is `k_rng_noise_small` alone; the scanned chain takes one in sc_step_begin (count, scan) and one for
    `k_rng_noise`."""
    assert tick["launches"] == (1 if chain == "small" else 2)


def against_twin(sc, world: K.World, start: int, ticks: int, chain: str, first_rows: int):
    dev = engine_ticks(sc, world, start, ticks, True)
    twin = engine_ticks(sc, world, start, ticks, False)
    for t, (a, b) in enumerate(zip(dev, twin)):
        assert a["rows"] == b["rows"] and (a["rows"] == first_rows if t == 0 else a["rows"] > 0)
        assert_chain(a, chain)
        assert_stream(a)
        assert np.array_equal(a["out"][3], world.ids)
        assert_same_bytes(a["out"], b["out"])
    return dev


def against_oracle(world: K.World, wc_coef: dict, ticks: list) -> None:
    """The ticks `engine_ticks` returned, each against `tick_core` restarted from the state before it, its `eta_u01`
    NumPy's block of that tick."""
    stage = K.oracle_stage()
    for name in ("dt", "particle_radius", "collider_noise_level", "viscosity", "pressure_amplifier", "target_pressure"):
        assert stage.coef[name] == wc_coef[name], name
    p, v = world.p, world.v
    for tick in ticks:
        out = K.oracle_tick(stage, p, v, tick["block"])
        gp, gv, gpr, _ = tick["out"]
        np.testing.assert_allclose(gp, out["particles"], rtol=RTOL, atol=ATOL["particles"])
        np.testing.assert_allclose(gv, out["velocities"], rtol=RTOL, atol=ATOL["velocities"])
        np.testing.assert_allclose(gpr, out["pressure"], rtol=RTOL, atol=ATOL["pressure"])
        p, v = gp, gv


# ------------------------------------------------------------------ the named noise cases, on both kernels
@pytest.mark.parametrize("chain", ["small", "scanned"])
@pytest.mark.parametrize("case", K.NOISE_CASES, ids=lambda c: c.name)
def test_noise_case_equals_numpy_and_the_host_block(sc, case, chain):
    """The stream state after every tick is NumPy's after rand(P, 2) from (key, start) -- key and position, exactly;
    P from sc_step_stats is the case's --, and positions, velocities and pressures equal the twin's that was handed
    `rs.rand(P, 2)`, bit for bit.  A quiet case leaves key and position as they were.  The cases that end or begin on
    the border and the one of two ticks also go against the oracle, `eta_u01` NumPy's block, at the margin the suite
    keeps between the kernels and the oracle."""
    world = on_chain(K.world_of(case), chain)
    dev = against_twin(sc, world, case.start, case.ticks, chain, case.rows)
    if case.family == "quiet":
        key, pos = dev[0]["state"]
        assert pos == case.start and np.array_equal(key, K.KEY)
    if case.family == "second_tick":  # the second tick began where the first ended, at an odd position
        assert dev[0]["want"][1] == 17 and dev[1]["want"][1] % 2 == 1
    if case in K.ORACLE_CASES or case.family == "second_tick":
        against_oracle(world, wave_world(sc, K.D, K.NOISE_LEVEL).coefficients, dev)


# ------------------------------------------------------------------ the small kernel's id scan
@pytest.mark.parametrize("bound", K.ID_BOUNDS)
def test_small_kernel_at_the_id_bounds(sc, bound):
    """Sparse ids in shuffled storage order whose host bound is `bound`: the offsets `k_rng_noise_small` scans put
    every particle's noise where the id order puts it -- the twin's offsets come from the two-level scan --, and the
    same world with only its top id moved past the small kernel's limit gives the same bytes and the same stream."""
    world = K.id_bound_world(bound)
    small = against_twin(sc, world, K.ID_BOUND_START, 1, "small", world.rows)
    up = world.with_top_id(K.SMALL_IDS)
    scanned = against_twin(sc, up, K.ID_BOUND_START, 1, "scanned", world.rows)
    assert_same_bytes(small[0]["out"][:3], scanned[0]["out"][:3])
    assert np.array_equal(small[0]["state"][0], scanned[0]["state"][0]) and small[0]["state"][1] == scanned[0]["state"][1]
    if bound == K.ID_BOUND_ORACLE:
        against_oracle(world, wave_world(sc, K.D, K.NOISE_LEVEL).coefficients, small)


# ------------------------------------------------------------------ emission
@pytest.mark.parametrize("name,start", K.EMIT_CASES)
def test_emission_from_the_border(sc, name, start):
    """EMIT_CALLS calls from (key, start): new positions, velocities and ids as NumPy draws them, bit for bit, and the
    stream state after every call -- after a launch that refilled and after one that did not."""
    sources = K.EMIT_LISTS[name]
    rs = K.numpy_state(start)
    eng = sc.Engine(2 * K.EMIT_ROOM)
    eng.rng_set_state(K.KEY, start)
    stored = next_id = 0
    trace = iter(t for t in K.emission_trace(name, start) if t["launch"] == 0)
    for _ in range(K.EMIT_CALLS):
        if stored + K.call_bound(sources) > K.EMIT_ROOM:
            eng.upload(np.zeros((0, 2)), np.zeros((0, 2)))
            stored = next_id = 0
        assert rs.get_state()[2] == next(trace)["start"]
        stored, next_id, _ = check_emission(eng, rs, sources, K.EMIT_DT, K.EMIT_MAX_PARTICLES, stored, next_id)
        key, pos = eng.rng_get_state()
        assert pos == rs.get_state()[2]
        assert np.array_equal(key, rs.get_state()[1])
    eng.close()


# ------------------------------------------------------------------ whole runs from an odd position
ODD = 623


def seed_key():
    """The key `Crate.__init__` leaves in np.random (it seeds it like the reference: crate.py:22)."""
    return np.random.RandomState(0).get_state()[1]


def test_a_run_from_an_odd_position_equals_the_host_drawn_stream(sc):
    """config/wave_machine.yaml for 30 ticks, emission and collider noise: the device stream from (key, 623) against
    noise="host-sync" with np.random set to the same state.  Every double of the run straddles a pair of words NumPy's
    even-position runs never pair up."""
    ticks = 30
    dev = sc.Crate(U.scene(sc), noise="host")
    dev.engine.rng_set_state(seed_key(), ODD)
    for _ in range(ticks):
        dev.physics_tick()
    got = dev.engine.download()
    _, pos = dev.engine.rng_get_state()
    dev.sync_host_rng()
    after_dev = np.random.rand(4)
    ref = sc.Crate(U.scene(sc), noise="host-sync")  # seeds np.random again
    np.random.set_state(("MT19937", seed_key(), ODD))
    for _ in range(ticks):
        ref.physics_tick()
    want = ref.engine.download()
    after_ref = np.random.rand(4)
    assert dev._noise == "host" and pos % 2 == 1
    assert len(got[3]) > 100 and got[3].max() > 300  # ~14 particles a tick were emitted, and part of them has left
    assert_same_bytes(got, want)
    assert np.array_equal(after_dev, after_ref)
    dev.close()
    ref.close()


def test_a_checkpoint_at_an_odd_position_resumes_the_same_run(sc, tmp_path):
    def started():
        crate = sc.Crate(U.scene(sc), noise="host")
        crate.engine.rng_set_state(seed_key(), ODD)
        return crate

    a = started()
    for _ in range(24):
        a.physics_tick()
    want, want_state = a.engine.download(), a.engine.rng_get_state()
    b = started()
    for _ in range(12):
        b.physics_tick()
    b.save_checkpoint(tmp_path / "odd.npz")
    with np.load(tmp_path / "odd.npz", allow_pickle=False) as z:
        meta = json.loads(str(z["meta"]))
    assert meta["rng_pos"] % 2 == 1
    np.random.seed(99)
    c = sc.Crate.from_checkpoint(tmp_path / "odd.npz")
    for _ in range(12):
        c.physics_tick()
    assert_same_bytes(c.engine.download(), want)
    key, pos = c.engine.rng_get_state()
    assert pos == want_state[1] and pos % 2 == 1 and np.array_equal(key, want_state[0])
    for crate in (a, b, c):
        crate.close()
