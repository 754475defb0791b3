"""GPU tests of the probe (sc_probe_now / sc_probe_enable / sc_probe_read, `Engine.probe_*`, `Crate.measure`,
`Crate.observe` / `Crate.observations`, `main --observe`): a measurement equals tests/probe_spec.py applied to the
downloaded state -- the six sums within the spec's tolerance, every other field and both profile arrays equal --, the log
holds byte for byte what measuring after every tick returns, a full log drops and counts, the log survives a grown
engine, logging changes no result, and measuring changes nothing in the simulation."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import gpu_support as U
import probe_cases as K
import probe_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def launch_sizes():
    from sand_crate_amd import _native as N
    from sand_crate_amd.engine import Engine
    assert Engine.PROBE_LAUNCH_THREADS == N.PROBE_BLOCK * N.PROBE_BLOCKS
    return N.PROBE_BLOCK, Engine.PROBE_LAUNCH_THREADS


CASES = K.cases(*launch_sizes())


def world_of(sc, case, **kw):
    n = len(case.xy)
    crate = sc.Crate(U.spread_world(sc, n), noise=kw.pop("noise", "counter"), noise_seed=1, capacity=n + 64, **kw)
    crate.particles = case.xy
    crate.particle_velocities = case.vxy
    return crate


def row_of(measured):
    return np.array([measured[name] for name in S.FIELDS], dtype=np.float64)


# ---- a measurement is the spec's

@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(sc, name):
    c = CASES[name]
    crate = world_of(sc, c)
    if c.tick:
        crate.physics_tick()
    xy, vxy, pressure, _ = crate.engine.download()
    got = crate.measure(c.bins, c.x_range)
    assert list(got)[:16] == list(S.FIELDS) and (("count" in got) == ("top" in got) == (c.bins > 0))
    S.compare_row(row_of(got), xy, vxy, pressure, 1 if c.tick else 0, c.bins, *c.x_range)
    if c.bins:
        count, top = S.profile(xy, c.bins, *c.x_range)
        assert got["count"].dtype == np.int32 and got["top"].dtype == np.float64
        assert np.array_equal(got["count"], count) and np.array_equal(got["top"], top)
    if c.tick:
        assert got["n_pressed"] > 0 and got["max_p"] > 0 and got["sum_p"] > 0 and got["n"] == len(c.xy)
    else:
        assert got["n_pressed"] == 0 and got["sum_p"] == 0 and got["max_p"] == 0   # right after an upload: zeros
    again = crate.measure(c.bins, c.x_range)                                     # measuring twice: identical bytes
    U.same_bytes(row_of(again), row_of(got))
    if c.bins:
        U.same_bytes(again["count"], got["count"])
        U.same_bytes(again["top"], got["top"])
    if "bin" in c.claims:
        assert got["count"][c.claims["bin"]] == len(c.xy) and got["top"][c.claims["bin"]] == c.claims["top"]
    if "bins" in c.claims:
        want = c.claims["bins"]
        assert np.array_equal(got["count"], np.bincount(want[want >= 0], minlength=c.bins))


def test_engine_calls_return_arrays(sc):
    crate = world_of(sc, CASES["n65"])
    row, counts, tops = crate.engine.probe_now(4, 0.0, 1.0)
    assert row.shape == (16,) and counts.shape == tops.shape == (4,) and counts.sum() == row[15] == 65
    row0, counts0, tops0 = crate.engine.probe_now()
    assert counts0.shape == tops0.shape == (0,) and row0[15] == 0 and np.array_equal(row0[:15], row[:15])


# ---- the log

@pytest.fixture()
def world400(sc):
    def make(noise="counter"):
        return world_of(sc, CASES["after_tick"], noise=noise)
    return make


def test_log_equals_measuring_after_every_tick(world400):
    crate = world400()
    assert crate.observations()["n"].shape == (0,) and crate.observations()["dropped"] == 0   # nothing is logged
    crate.observe(capacity=16, bins=32)
    empty = crate.observations()
    assert empty["tick"].shape == (0,) and empty["count"].shape == empty["top"].shape == (0, 32) and empty["dropped"] == 0
    measured = []
    for _ in range(8):
        crate.physics_tick()
        measured.append(crate.measure(32))
    obs = crate.observations()
    assert obs["tick"].tolist() == list(range(1, 9)) and obs["dropped"] == 0
    assert obs["count"].shape == obs["top"].shape == (8, 32) and obs["count"].dtype == np.int32
    for t, m in enumerate(measured):
        U.same_bytes(np.array([obs[name][t] for name in S.FIELDS]), row_of(m))
        U.same_bytes(obs["count"][t], m["count"])
        U.same_bytes(obs["top"][t], m["top"])
    assert len(set(obs["sum_ke"].tolist())) == 8                       # (the state moves)
    assert crate.observations()["tick"].shape == (0,)                  # read and cleared
    crate.physics_tick()
    assert crate.observations()["tick"].tolist() == [9.0]
    crate.observe(False)
    crate.physics_tick()
    assert crate.observations()["tick"].shape == (0,)


def test_log_through_run_changes_nothing(world400):
    logged, single, plain = world400(), world400(), world400()
    logged.observe(capacity=8, bins=32)
    single.observe(capacity=8, bins=32)
    logged.run(8)
    for _ in range(8):
        single.physics_tick()
    plain.run(8)
    a, b = logged.observations(), single.observations()
    assert a["tick"].tolist() == list(range(1, 9)) and a["dropped"] == b["dropped"] == 0
    for name in (*S.FIELDS, "count", "top"):
        U.same_bytes(a[name], b[name])
    for x, y in zip(logged.engine.download(), plain.engine.download()):   # the log changes no result
        U.same_bytes(x, y)
    for x, y in zip(logged.engine.download(), single.engine.download()):
        U.same_bytes(x, y)
    xy, vxy, pressure, _ = logged.engine.download()
    S.compare_row(np.array([a[name][-1] for name in S.FIELDS]), xy, vxy, pressure, 8, 32)
    count, top = S.profile(xy, 32, 0.0, 1.0)
    assert np.array_equal(a["count"][-1], count) and np.array_equal(a["top"][-1], top)


def test_a_full_log_drops_and_counts(world400):
    crate = world400()
    crate.observe(capacity=3, bins=4)
    for _ in range(5):
        crate.physics_tick()
    obs = crate.observations()
    assert obs["tick"].tolist() == [1.0, 2.0, 3.0] and obs["dropped"] == 2 and obs["count"].shape == (3, 4)
    assert (obs["count"].sum(axis=1) == obs["n_binned"]).all()
    crate.physics_tick()
    crate.physics_tick()
    obs = crate.observations()                                         # after the read the log records again
    assert obs["tick"].tolist() == [6.0, 7.0] and obs["dropped"] == 0
    assert (obs["count"].sum(axis=1) == obs["n_binned"]).all() and (obs["n_binned"] > 0).all()   # (its bins were cleared)
    # with less room than rows, the rest stays for the next read
    for _ in range(3):
        crate.physics_tick()
    rows, counts, tops, dropped = crate.engine.probe_read(2)
    assert rows[:, 0].tolist() == [8.0, 9.0] and counts.shape == (2, 4) and dropped == 0
    rows, _, _, _ = crate.engine.probe_read()
    assert rows[:, 0].tolist() == [10.0]


def test_grow_keeps_the_log(sc):
    n = 50
    crate = sc.Crate(U.spread_world(sc, 4 * n + 2000), noise="counter", noise_seed=1, capacity=n)   # (discs sized for the crowd)
    xy, vxy = K.cloud(2, n, 0.05, 0.95)
    crate.particles = xy
    crate.particle_velocities = vxy
    crate.observe(capacity=16, bins=8)
    for _ in range(3):
        crate.physics_tick()
    old = crate.engine
    more, _ = K.cloud(3, 4 * n + 2000, 0.05, 0.95)
    crate.particles = more                                            # more than the capacity: `_grow` makes a new context
    assert crate.engine is not old
    for _ in range(2):
        crate.physics_tick()
    obs = crate.observations()
    assert obs["n"][:3].tolist() == [n] * 3 and obs["n"][3] == len(more) >= obs["n"][4] > n   # before and after, in order
    assert obs["tick"].tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]          # (the new context counts on: the tick goes over)
    assert obs["count"].shape == (5, 8) and obs["dropped"] == 0
    U.same_bytes(np.array([obs[name][-1] for name in S.FIELDS]), row_of(crate.measure(8)))


# ---- errors

def test_argument_errors(sc):
    from sand_crate_amd import _native as N
    crate = world_of(sc, CASES["n65"])
    eng = crate.engine
    lib, ctx = eng._lib, eng._ctx
    nan, inf = float("nan"), float("inf")
    good = eng.probe_now(4)[0]
    for bad in ((-1, 0.0, 1.0), (1025, 0.0, 1.0), (4, nan, 1.0), (4, 0.0, inf), (4, -inf, 1.0), (4, 0.5, 0.5), (4, 0.75, 0.25)):
        assert U.code_of(eng.probe_now, *bad) == N.ERR_ARG, bad
        assert U.code_of(eng.probe_enable, 8, *bad) == N.ERR_ARG, bad
        U.same_bytes(eng.probe_now(4)[0], good)                          # a valid call still works
    for capacity in (0, -3, (1 << 20) + 1):
        assert U.code_of(eng.probe_enable, capacity) == N.ERR_ARG
    assert U.code_of(eng.probe_read, 4) == N.ERR_STATE                    # (none of them switched the log on)
    eng.probe_now(0, nan, nan)                                          # without bins the range is not looked at
    row = np.zeros(16)
    counts, tops = np.zeros(4, dtype=np.int32), np.zeros(4)
    n, dropped = C.c_int64(0), C.c_int64(0)
    assert lib.sc_probe_now(ctx, 0, 0.0, 1.0, None, None, None) == N.ERR_ARG
    assert lib.sc_probe_now(ctx, 4, 0.0, 1.0, N.dptr(row), None, N.dptr(tops)) == N.ERR_ARG
    assert lib.sc_probe_now(ctx, 4, 0.0, 1.0, N.dptr(row), N.i32ptr(counts), None) == N.ERR_ARG
    assert lib.sc_probe_now(None, 0, 0.0, 1.0, N.dptr(row), None, None) == N.ERR_ARG
    assert lib.sc_probe_enable(None, 8, 0, 0.0, 1.0) == N.ERR_ARG and lib.sc_probe_disable(None) == N.ERR_ARG
    eng.probe_enable(8, 4)
    crate.physics_tick()
    rows = np.zeros((8, 16))
    many_counts, many_tops = np.zeros((8, 4), dtype=np.int32), np.zeros((8, 4))
    assert lib.sc_probe_read(ctx, None, N.i32ptr(many_counts), N.dptr(many_tops), 8, C.byref(n), C.byref(dropped)) == N.ERR_ARG
    assert lib.sc_probe_read(ctx, N.dptr(rows), None, N.dptr(many_tops), 8, C.byref(n), C.byref(dropped)) == N.ERR_ARG
    assert lib.sc_probe_read(ctx, N.dptr(rows), N.i32ptr(many_counts), None, 8, C.byref(n), C.byref(dropped)) == N.ERR_ARG
    assert lib.sc_probe_read(ctx, N.dptr(rows), N.i32ptr(many_counts), N.dptr(many_tops), 8, None, C.byref(dropped)) == N.ERR_ARG
    assert lib.sc_probe_read(ctx, N.dptr(rows), N.i32ptr(many_counts), N.dptr(many_tops), 8, C.byref(n), None) == N.ERR_ARG
    assert lib.sc_probe_read(None, N.dptr(rows), N.i32ptr(many_counts), N.dptr(many_tops), 8, C.byref(n), C.byref(dropped)) == N.ERR_ARG
    assert U.code_of(eng.probe_read, -1) == N.ERR_ARG
    assert lib.sc_last_error()
    got, _, _, dropped_now = eng.probe_read()                           # none of the refused reads took the row
    assert got[:, 0].tolist() == [1.0] and dropped_now == 0
    eng.probe_disable()
    assert U.code_of(eng.probe_read) == N.ERR_STATE
    eng.probe_disable()                                                 # (off twice is fine)


def test_state_errors_inside_a_tick_and_after_a_promise(sc):
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc, "wave_machine"), noise="host-sync")
    crate.physics_tick()
    eng = crate.engine
    eng.probe_enable(8)
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(eng.probe_now) == N.ERR_STATE
        assert U.code_of(eng.probe_read) == N.ERR_STATE
        assert U.code_of(eng.probe_enable, 8) == N.ERR_STATE
        assert U.code_of(eng.probe_disable) == N.ERR_STATE
        stats = eng.step_stats()
        eng.set_noise_host(np.random.rand(stats.neighbor_slots, 2))
    finally:
        eng.step_finish()
    rows, _, _, _ = eng.probe_read()                                    # the refused calls left the log on
    assert rows[:, 0].tolist() == [2.0] and eng.probe_now()[0][0] == 2.0
    eng.probe_disable()

    # a pending promise (the tick before was fused with this one's wall pass): the log cannot be switched
    crate = world_of(sc, CASES["after_tick"])
    eng = crate.engine
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    now = crate._pack_tick_inputs()
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    nxt = crate._pack_tick_inputs()
    eng.tick(now, nxt)
    assert U.code_of(eng.probe_enable, 8) == N.ERR_STATE
    assert U.code_of(eng.probe_disable) == N.ERR_STATE
    assert U.code_of(eng.probe_read) == N.ERR_STATE                       # (it is not on)
    eng.tick(nxt)
    eng.probe_enable(8)                                                 # the promise is kept: now it can
    eng.tick(nxt)
    assert eng.probe_read()[0][:, 0].tolist() == [3.0]


def test_slab_contexts_refuse(sc):
    from sand_crate_amd import _native as N
    eng = sc.Engine(capacity=64)
    xy, vxy = K.cloud(1, 20)
    eng.upload(xy, vxy)
    assert eng.probe_now()[0][1] == 20
    eng.set_slab(0, 10, 3, False, False)
    for call, args in ((eng.probe_now, ()), (eng.probe_enable, (8,)), (eng.probe_disable, ()), (eng.probe_read, ())):
        assert U.code_of(call, *args) == N.ERR_STATE
        assert eng.count() == 20                                        # the context is fine
    eng.close()


# ---- the simulation is left alone

def test_measuring_is_read_only(sc):
    def trajectory(measure):
        crate = sc.Crate(U.scene(sc, "wave_machine"))                      # noise="host": the device holds the stream
        for _ in range(10):
            crate.physics_tick()
            if measure:
                before = crate.engine.download(), crate.engine.rng_get_state()
                assert crate.measure(64)["tick"] == crate.tick and crate.measure()["n"] == len(before[0][0])
                after = crate.engine.download(), crate.engine.rng_get_state()
                for x, y in zip(before[0], after[0]):
                    U.same_bytes(x, y)
                assert np.array_equal(before[1][0], after[1][0]) and before[1][1] == after[1][1]
        assert crate.tick == 10
        return (*crate.engine.download(), crate.engine.rng_get_state())

    a, b = trajectory(False), trajectory(True)
    for x, y in zip(a[:4], b[:4]):
        U.same_bytes(x, y)
    assert np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


# ---- the driver

def test_headless_driver_with_observe(tmp_path):
    from sand_crate_amd.main import main
    summary = main(ROOT / "config" / "wave_machine.yaml", tmp_path, variants=1, ticks=20, observe=16)
    with np.load(tmp_path / "variant_00" / "observables.npz") as z:
        obs = {k: z[k] for k in z.files}
    assert obs["fields"].tolist() == list(S.FIELDS) and obs["x_range"].tolist() == [0.0, 1.0] and float(obs["dt"]) == 0.002
    assert obs["tick"].tolist() == list(range(1, 21)) and obs["count"].shape == obs["top"].shape == (20, 16)
    assert all(obs[name].shape == (20,) for name in S.FIELDS) and int(obs["dropped"]) == 0
    assert obs["n"][-1] == summary[0]["particles"] == summary[0]["n"] > 0
    assert summary[0]["sum_ke"] == obs["sum_ke"][-1] and summary[0]["max_speed2"] == obs["max_speed2"][-1]
    assert (tmp_path / "variant_00" / "config.yaml").exists()
    plain = main(ROOT / "config" / "wave_machine.yaml", tmp_path / "plain", variants=1, ticks=20)
    assert not (tmp_path / "plain" / "variant_00" / "observables.npz").exists()
    assert sorted(plain[0]) == ["coefficients", "particles", "seconds", "ticks", "variant"]
    assert plain[0]["particles"] == summary[0]["particles"]
