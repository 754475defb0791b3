"""What a context is worth after the library has reported an error and the caller carries on (include/sandcrate_hip.h,
sc_set_scan_patience: "What an abandoned tick leaves"): ticks abandoned behind their bucket scan, read first by every
call that reads the flags, on both tick paths; and a particle dropped as NaN.  The worlds and their premises:
tests/recovery_cases.py, proved in tests/test_recovery_cases_cpu.py, which also holds the model of the counters that says
what each assertion here saw before `recover_flags` existed.

Every context has room for (A + 2) n particles (recovery_cases.capacity).  Tolerances are test_ticks_match_oracle's; what is
called exact is compared byte for byte."""
import copy

import numpy as np
import pytest

import gpu_support as U
import probe_spec
import recovery_cases as rc
import track_spec
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 77
PATIENCE = 1 << 22  # the default (sc_kernels.h: kScanMaxPolls)
# the oracle's worlds, built once and before any crate: an OracleCrate seeds np.random as the reference does (crate.py:22),
# and the crate of the "host-sync" test draws from that very generator between its ticks
ORACLES = {id(coef): rc.oracle(coef) for coef in (rc.COEF, rc.PILE_COEF)}


def make_crate(sc, state, noise, capacity, coef=rc.COEF):
    from sand_crate_amd.load_config import WorldConfig
    wc = WorldConfig([copy.deepcopy(rc.BOX)], [], copy.deepcopy(coef))
    crate = sc.Crate(wc, noise=noise, noise_seed=SEED, capacity=capacity)
    crate.particles = state[0]
    crate.particle_velocities = state[1]
    return crate


def run_ticks(crate, path, k):
    if path == "run":
        crate.run(k)
    else:
        for _ in range(k):
            crate.physics_tick()


READERS = {
    "synchronize": lambda crate: crate.synchronize(),
    "particles": lambda crate: crate.particles,
    "download": lambda crate: crate.engine.download(),
    "count_then_particles": lambda crate: (crate.particle_count, crate.particles),
}


def expect_error_once(crate, reader, code, *words):
    """The first reader of the flags raises `code` with `words` in its text; after that every reader is clean."""
    from sand_crate_amd import _native as N
    with pytest.raises(N.NativeError) as e:
        READERS[reader](crate)
    assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
    for again in READERS.values():
        again(crate)


def wall_fixed(p, coef=rc.COEF):
    from oracle.tick import hard_wall_fix, wall_contacts
    orc = ORACLES[id(coef)]
    V, u, _ = wall_contacts(p, orc.segments, orc.body_states(), coef["particle_radius"])
    return hard_wall_fix(p, V, u, coef["particle_radius"])


def oracle_tick(state, noise, tick, coef=rc.COEF, eta=None):
    """tick_core on (p, v, ids); counter noise is keyed by `tick`, the number the context gave the tick."""
    from oracle.tick import counter_noise_key, counter_noise_u01, tick_core
    p, v, ids = state
    orc = ORACLES[id(coef)]
    if noise == "counter":
        eta = counter_noise_u01(ids, counter_noise_key(SEED, tick))
    with np.errstate(all="ignore"):
        return tick_core(p, v, orc.segments, orc.body_states(), orc.coef, eta_u01=eta)


def assert_tick(got, out, ids, keep=None):
    gp, gv, gpr, gids = got
    keep = slice(None) if keep is None else keep
    assert np.array_equal(gids, ids[keep])
    np.testing.assert_allclose(gp, out["particles"][keep], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gv, out["velocities"][keep], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(gpr, out["pressure"][keep], rtol=1e-9, atol=1e-12)


def assert_sort_tap(eng, state, coef=rc.COEF):
    """One more tick, begun and finished on the engine with the inputs it already has: its sort tap is the oracle's strip
    sort of the wall-fixed positions, bit for bit."""
    from oracle.neighbors import strip_sort
    p, _, ids = state
    eng.step_begin()
    rows, sorted_ids = eng.download_sort()
    eng.step_finish()
    ref_rows, ref_order = strip_sort(wall_fixed(p, coef), 2 * coef["particle_radius"])
    assert np.array_equal(rows, ref_rows) and np.array_equal(sorted_ids, ids[ref_order])


def abandon(crate, path, k=rc.ABANDONED):
    crate.engine.set_scan_patience(-1)  # every workgroup of the scan but the first gives up without having looked
    run_ticks(crate, path, k)
    crate.engine.set_scan_patience(PATIENCE)


def assert_state_as_found(before, after, coef=rc.COEF):
    """Velocities, ids, count and pressures exactly; positions exactly but for the wall fix, applied once."""
    U.same_bytes(after[1], before[1])
    U.same_bytes(after[3], before[3])
    U.same_bytes(after[2], before[2])
    U.same_bytes(after[0], wall_fixed(before[0], coef))


# ---------------------------------------------------------------- every reader, every tick path
@pytest.mark.parametrize("path", ["physics_tick", "run"])
@pytest.mark.parametrize("reader", list(READERS))
@pytest.mark.parametrize("world", ["quiet", "walls"])
def test_every_reader_recovers_on_every_tick_path(sc, world, reader, path):
    """Two good ticks, A abandoned ones, the reader, three good ticks -- with counter noise, which is keyed by the tick
    numbers the context actually used: the abandoned ticks have taken theirs."""
    from sand_crate_amd import _native as N
    band = rc.band() if world == "walls" else None
    n = len(rc.quiet()[0]) + (len(band[0]) if band else 0)
    crate = make_crate(sc, rc.quiet(), "counter", rc.capacity(n))
    eng = crate.engine
    run_ticks(crate, path, rc.GOOD_BEFORE)
    if band:
        eng.append(*band)  # inside r of the floor: the abandoned tick's wall fix has something to move
    before = eng.download()
    assert len(before[0]) == n and before[2][:6000].max() > 0 and not before[2][6000:].any()
    abandon(crate, path)
    expect_error_once(crate, reader, N.ERR_HIP, "bucket scan", "skipped")
    after = eng.download()
    assert_state_as_found(before, after)
    if world == "quiet":
        U.same_bytes(after[0], before[0])
    else:
        assert (after[0] != before[0]).any(axis=1).sum() == len(band[0])
    state = (after[0], after[1], after[3])
    for k in range(rc.GOOD_AFTER):
        run_ticks(crate, path, 1)
        out = oracle_tick(state, "counter", rc.GOOD_BEFORE + rc.ABANDONED + k)
        got = eng.download()
        assert crate.particle_count == n
        assert_tick(got, out, state[2])
        state = (got[0], got[1], got[3])
    assert_sort_tap(eng, state)


# ---------------------------------------------------------------- big buckets: k_sort_big's task list
def recovered_pile(sc, reader):
    from sand_crate_amd import _native as N
    n = max(len(rc.pile()[0]), len(rc.pile_after()[0])) + len(rc.extra()[0])
    crate = make_crate(sc, rc.pile(), "none", rc.capacity(n), coef=rc.PILE_COEF)
    run_ticks(crate, "physics_tick", rc.GOOD_BEFORE)  # (the second one has seen the first one's big buckets: it sorts them)
    before = crate.engine.download()
    assert before[2].max() > 1.0  # a pile's pressures
    abandon(crate, "physics_tick")
    expect_error_once(crate, reader, N.ERR_HIP, "bucket scan", "skipped")
    after = crate.engine.download()
    assert_state_as_found(before, after, rc.PILE_COEF)
    U.same_bytes(after[0], before[0])
    return crate, (after[0], after[1], after[3])


def engine_tick(eng, state, coef):
    """A tick on the engine with the inputs it has, its sort tap taken: -> the downloaded state, checked."""
    from oracle.neighbors import strip_sort
    p, v, ids = state
    eng.step_begin()
    rows, sorted_ids = eng.download_sort()
    eng.step_finish()
    out = oracle_tick(state, "none", 0, coef)
    ref_rows, ref_order = strip_sort(out["fixed_positions"], 2 * coef["particle_radius"])
    assert np.array_equal(rows, ref_rows) and np.array_equal(sorted_ids, ids[ref_order])
    got = eng.download()
    assert_tick(got, out, ids)
    return got[0], got[1], got[3]


@pytest.mark.parametrize("then", ["tick", "upload", "append"])
@pytest.mark.parametrize("reader", ["synchronize", "download"])
def test_pile_recovers(sc, reader, then):
    """After the recovery: a tick on the pile itself; another state whose buckets in the listed cells are shorter than
    the chunks listed for them, and two ticks; a few more particles in and beside the pile, and a tick.  The sorted
    order bit for bit, the tick within the tolerances."""
    crate, state = recovered_pile(sc, reader)
    eng = crate.engine
    if then == "upload":
        p, v = rc.pile_after()
        eng.upload(p, v)
        state = (p, v, np.arange(len(p)))
        state = engine_tick(eng, state, rc.PILE_COEF)
    elif then == "append":
        p, v = rc.extra()
        eng.append(p, v)
        n = len(state[0])
        state = (np.concatenate((state[0], p)), np.concatenate((state[1], v)), np.arange(n + len(p)))
    state = engine_tick(eng, state, rc.PILE_COEF)
    assert len(state[0]) == len(eng.download()[0])


# ---------------------------------------------------------------- the stream of noise="host", held on the device
@pytest.mark.parametrize("reader", ["synchronize", "download"])
@pytest.mark.parametrize("world", ["quiet", "dense"])
def test_device_stream_does_not_move_for_abandoned_ticks(sc, world, reader):
    """A: two ticks, A abandoned ones, the reader, two ticks.  B: four ticks.  The same state in the end, byte for byte,
    and the generator right after the recovery where it stood before the abandoned ticks.  `dense` hands out more than
    65,536 ids: the offsets and the noise come from k_count_by_id and k_rng_noise, not from the one small launch."""
    from sand_crate_amd import _native as N
    state = getattr(rc, world)()
    cap = rc.capacity(len(state[0]))
    a = make_crate(sc, state, "host", cap)
    run_ticks(a, "physics_tick", 2)
    key0, pos0 = a.engine.rng_get_state()
    found = a.engine.download()
    abandon(a, "physics_tick")
    key1, pos1 = a.engine.rng_get_state()  # (before the reader, too)
    expect_error_once(a, reader, N.ERR_HIP, "bucket scan", "skipped")
    key2, pos2 = a.engine.rng_get_state()
    U.same_bytes(key1, key0)
    U.same_bytes(key2, key0)
    assert pos0 == pos1 == pos2
    assert_state_as_found(found, a.engine.download())  # (dense has particles at the walls by now: the fix, once)
    run_ticks(a, "physics_tick", 2)
    b = make_crate(sc, state, "host", cap)
    run_ticks(b, "physics_tick", 4)
    got, want = a.engine.download(), b.engine.download()
    assert not np.array_equal(want[0], found[0])
    for x, y in zip(got, want):
        U.same_bytes(x, y)
    ka, pa = a.engine.rng_get_state()
    kb, pb = b.engine.rng_get_state()
    U.same_bytes(ka, kb)
    assert pa == pb and (pa != pos0 or not np.array_equal(ka, key0))


# ---------------------------------------------------------------- noise="host-sync": the host draws, from np.random
def test_host_sync_draws_nothing_for_an_abandoned_tick(sc):
    from sand_crate_amd import _native as N
    p, v = rc.quiet()
    n = len(p)
    crate = make_crate(sc, (p, v), "host-sync", rc.capacity(n))  # (Crate seeds np.random with 0)
    host = np.random.RandomState(0)  # ... and this is the oracle's copy of that stream
    state = (p, v, np.arange(n))

    def good_tick(state):
        crate.physics_tick()
        assert crate.last_stats.flags == 0 and crate.last_stats.particles == n
        out = oracle_tick(state, "host-sync", 0, eta=lambda total: host.rand(total, 2))
        assert crate.last_stats.neighbor_slots == int(out["neighbor_counts"].sum())
        got = crate.engine.download()
        assert_tick(got, out, state[2])
        return got[0], got[1], got[3]

    for _ in range(rc.GOOD_BEFORE):
        state = good_tick(state)
    before = crate.engine.download()
    crate.engine.set_scan_patience(-1)
    for _ in range(rc.ABANDONED):
        name, key, pos, has_gauss, gauss = np.random.get_state()
        crate.physics_tick()
        s = crate.last_stats
        assert s.flags & N.FLAG_SCAN_TIMEOUT
        assert (s.particles, s.neighbor_slots, s.max_neighbors, s.wall_particles) == (n, 0, 0, 0)
        now = np.random.get_state()
        assert now[0] == name and np.array_equal(now[1], key) and now[2:] == (pos, has_gauss, gauss)
        assert crate.particle_count == n
    crate.engine.set_scan_patience(PATIENCE)
    expect_error_once(crate, "particles", N.ERR_HIP, "bucket scan", "skipped")
    after = crate.engine.download()
    assert_state_as_found(before, after)
    U.same_bytes(np.random.get_state()[1], host.get_state()[1])  # the two streams stand at the same place
    assert np.random.get_state()[2] == host.get_state()[2]
    for _ in range(rc.GOOD_AFTER):
        state = good_tick(state)
        assert crate.particle_count == n


# ---------------------------------------------------------------- the state on the device, before and after the reader
@pytest.mark.parametrize("world", ["quiet", "walls"])
def test_export_before_the_first_reader(sc, world):
    """sc_export_state_device never reads the flags.  Between the abandoned ticks and the first reader it delivers what
    the header says: positions (the wall fix applied once), velocities, ids and the count exactly, the pressures of the
    last finished tick -- none for particles appended since.  After the recovery it is the download again."""
    import torch
    from sand_crate_amd import _native as N
    from test_gpu_state import assert_export_is_download
    band = rc.band() if world == "walls" else None
    n = len(rc.quiet()[0]) + (len(band[0]) if band else 0)
    crate = make_crate(sc, rc.quiet(), "counter", rc.capacity(n))
    run_ticks(crate, "physics_tick", rc.GOOD_BEFORE)
    if band:
        crate.engine.append(*band)
    before = crate.engine.download()
    assert before[2].max() > 0
    abandon(crate, "physics_tick")
    torch.cuda.synchronize()
    *tensors, count = crate.state_tensors(ids=True, sync=False)  # (sync=True would read the flags: Engine.synchronize)
    torch.cuda.synchronize()  # (waits for the library's stream too, and reads no flag)
    assert int(count.item()) == n
    exported = tuple(t[:n].cpu().numpy() for t in tensors)
    assert_state_as_found(before, exported)
    expect_error_once(crate, "download", N.ERR_HIP, "bucket scan", "skipped")  # ... and it was still there to be read
    for x, y in zip(crate.engine.download(), exported):
        U.same_bytes(x, y)
    assert_export_is_download(crate.engine)
    crate.physics_tick()
    got = assert_export_is_download(crate.engine)
    assert got[2].max() > 0


# ---------------------------------------------------------------- the logs
def test_logs_hold_no_row_for_an_abandoned_tick(sc):
    """observe() and track(every=1): a row and a frame for every tick that happened, none for an abandoned one, none
    counted as dropped; every row is probe_spec's, every frame track_spec's, of the state downloaded after that tick."""
    from sand_crate_amd import _native as N
    p, v = rc.quiet()
    crate = make_crate(sc, (p, v), "counter", rc.capacity(len(p)))
    crate.observe(capacity=16, bins=8)
    crate.track(every=1)
    states = {}

    def good(k):
        for _ in range(k):
            crate.physics_tick()
            states[crate.tick] = crate.engine.download()

    good(rc.GOOD_BEFORE)
    abandon(crate, "physics_tick")
    expect_error_once(crate, "synchronize", N.ERR_HIP, "bucket scan", "skipped")
    good(rc.GOOD_AFTER)
    ticks = [1, 2, 5, 6, 7]
    assert sorted(states) == ticks and crate.tick == 7
    obs = crate.observations()
    assert obs["tick"].tolist() == [float(t) for t in ticks] and obs["dropped"] == 0
    for k, t in enumerate(ticks):
        xy, vxy, pressure, _ = states[t]
        probe_spec.compare_row(np.array([obs[name][k] for name in probe_spec.FIELDS]), xy, vxy, pressure, t, 8)
        count, top = probe_spec.profile(xy, 8, 0.0, 1.0)
        assert np.array_equal(obs["count"][k], count) and np.array_equal(obs["top"][k], top)
    frames, dropped = crate.tracked()
    assert dropped == 0 and [track_spec.header(f)["tick"] for f in frames] == ticks
    for f, t in zip(frames, ticks):
        xy, _, pressure, ids = states[t]
        want = track_spec.pack(t, xy, pressure, ids, crate.segments, pressure_valid=True)
        assert track_spec.canonical(f) == track_spec.canonical(want)


# ---------------------------------------------------------------- a particle dropped as NaN
@pytest.mark.parametrize("reader", ["particles", "synchronize"])
def test_nan_drop_read_first_by(sc, reader):
    """crate.py:206: a particle exactly on a wall becomes NaN; it is dropped and reported once, by whichever call reads
    the flags first.  The survivors are the oracle's other rows, and the ticks after it are right on them."""
    from sand_crate_amd import _native as N
    p, v = rc.nan()
    n = len(p)
    crate = make_crate(sc, (p, v), "counter", rc.capacity(n))
    crate.physics_tick()
    out = oracle_tick((p, v, np.arange(n)), "counter", 0)
    keep = ~np.isnan(out["particles"]).any(axis=1)
    assert keep.sum() == n - 1 and not keep[rc.NAN_AT]
    expect_error_once(crate, reader, N.ERR_DOMAIN, "NaN")
    got = crate.engine.download()
    assert_tick(got, out, np.arange(n), keep)
    assert crate.particle_count == n - 1
    state = (got[0], got[1], got[3])
    for k in range(3):
        crate.physics_tick()
        out = oracle_tick(state, "counter", 1 + k)
        got = crate.engine.download()
        assert crate.particle_count == n - 1
        assert_tick(got, out, state[2])
        state = (got[0], got[1], got[3])
    assert_sort_tap(crate.engine, state)
