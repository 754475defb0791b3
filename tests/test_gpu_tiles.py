"""The tiled passes (csrc/sc_tiled.h) on the worlds of tests/tile_cases.py: tiles, reaches and scan ranges of exactly the
sizes at which pass A and pass B change path or table format -- 960, 1024 / 1100, 4095, 65535 entries, scans of 32, 128
and 256 candidates, scans on the half-window grid -- and the sizes next to them.  Lists bit for bit against the oracle
with both pass A tiles, ticks against the oracle restarted from the device's state, the fused run against single ticks.
tests/test_tile_cases_cpu.py proves that every world has the size it is named after."""
import functools

import numpy as np
import pytest

import tile_cases as tc
from gpu_support import sc  # noqa: F401
from test_gpu_parity import wave_world

pytestmark = pytest.mark.gpu

D = tc.D
WORLDS = {f"lone{n}": functools.partial(tc.lone_bucket, n) for n in tc.LONE_SIZES}
WORLDS.update({f"ranges{t}": (lambda t=t: tc.three_ranges(t)[0]) for t in tc.RANGE_SIZES})
WORLDS.update({f"reach{r}": (lambda r=r: tc.reach_edge(r)[0]) for r in tc.REACH_SIZES})
WORLDS["scans"] = lambda: tc.scan_lengths()[0]
BIG = {f"lone{n}": functools.partial(tc.lone_bucket, n) for n in tc.LONE_BIG_SIZES}
# the worlds around 960 and 4095, lone and three-range: the DENS-only launch of host noise reads rows with its own slots_fit
HOST_WORLDS = [f"{kind}{t + k}" for kind in ("lone", "ranges") for t in (960, 4095) for k in (-1, 0, 1, 2)]
FUSED_WORLDS = [f"{kind}{t}" for kind in ("lone", "ranges") for t in tc.EDGES] + ["reach960", "reach4095"]


@functools.lru_cache(maxsize=None)
def world(name):
    """-> (points, (rows, order, counts, table) of the reference); computed once, never written to."""
    from oracle.neighbors import neighbor_lists, strip_sort
    pts = (WORLDS.get(name) or BIG[name])()
    lists = tc.cluster_lists(pts, D) if name in BIG else neighbor_lists(pts, D)
    for a in (pts,) + lists:
        a.setflags(write=False)
    return pts, strip_sort(pts, D) + lists


@pytest.mark.parametrize("tile", ["narrow", "wide"])
@pytest.mark.parametrize("name", list(WORLDS) + list(BIG))
def test_lists_bit_for_bit(sc, name, tile, monkeypatch):
    monkeypatch.setenv("SANDCRATE_TILE", tile)  # read by sc_create: both pass A tile sizes, whatever the grid
    pts, (ref_rows, ref_order, ref_counts, ref_table) = world(name)
    rows, order, counts, table = sc.neighbor_search(pts, D)
    assert np.array_equal(rows, ref_rows) and np.array_equal(order, ref_order)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(table, ref_table)


def _crate(sc, pts, noise, seed=5):
    """A crate with the world's particles, each moving about a cell per tick (any direction): the second tick has another
    sorted order, and the host has seen the first one's big buckets by then."""
    wc = wave_world(sc, D, 0.0 if noise == "none" else 0.1)
    wc.coefficients["max_particles"] = len(pts)
    v = (np.random.RandomState(seed).rand(len(pts), 2) - 0.5) * 2 * D / wc.coefficients["dt"]
    crate = sc.Crate(wc, noise=noise, noise_seed=77)
    crate.particles, crate.particle_velocities = pts, v
    return crate, wc, v


def _ticks_against_oracle(sc, pts, noise, ticks, lists=None, neighbor_fn=None, v_atol=1e-10):
    """`lists`: the reference lists of `pts`, which the first tick searches as they are (no wall near them to move any)."""
    from oracle.neighbors import neighbor_lists
    from oracle.scene import OracleCrate
    from oracle.tick import counter_noise_key, counter_noise_u01, remove_outside, tick_core
    from oracle.world import World
    crate, wc, v = _crate(sc, pts, noise)
    if neighbor_fn is not None:
        v = np.zeros_like(pts)
        crate.particle_velocities = v
    else:
        def neighbor_fn(q, d):
            return lists if lists is not None and d == D and np.array_equal(q, pts) else neighbor_lists(q, d)
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))
    host = np.random.RandomState(0)  # noise "host-sync": Crate seeds np.random with 0 and draws one block per tick
    p, ids = pts, np.arange(len(pts))
    for t in range(ticks):
        crate.physics_tick()
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        p, v, ids = remove_outside(p, v, orc.coef["particle_radius"], ids)
        eta = {"none": None, "counter": counter_noise_u01(ids, counter_noise_key(77, t)),
               "host-sync": lambda total: host.rand(total, 2)}[noise]
        out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef, eta_u01=eta, neighbor_fn=neighbor_fn)
        gp, gv, gpr, gids = crate.engine.download()
        assert np.array_equal(gids, ids)
        np.testing.assert_allclose(gpr, out["pressure"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gv, out["velocities"], rtol=1e-9, atol=v_atol)
        np.testing.assert_allclose(gp, out["particles"], rtol=1e-9, atol=1e-12)
        p, v = gp, gv


@pytest.mark.parametrize("noise", ["none", "counter"])
@pytest.mark.parametrize("name", list(WORLDS))
def test_two_ticks_match_the_oracle(sc, name, noise):
    pts, ref = world(name)
    _ticks_against_oracle(sc, pts, noise, 2, lists=ref[2:])


@pytest.mark.parametrize("name", HOST_WORLDS)
def test_two_ticks_with_host_noise_match_the_oracle(sc, name):
    """Search and density in separate launches: the density launch reads the lists back from the rows of the published tile."""
    pts, ref = world(name)
    _ticks_against_oracle(sc, pts, "host-sync", 2, lists=ref[2:])


@pytest.mark.parametrize("name", list(BIG))
def test_one_tick_of_a_bucket_around_65535(sc, name):
    pts, ref = world(name)
    _ticks_against_oracle(sc, pts, "none", 1, neighbor_fn=lambda q, d: ref[2:])  # (a tick searches the positions it was given)


@pytest.mark.parametrize("name", FUSED_WORLDS)
def test_fused_run_equals_single_ticks(sc, name):
    pts = world(name)[0]
    single, _, _ = _crate(sc, pts, "none")
    for _ in range(3):
        single.physics_tick()
    sp, sv, spr, sids = single.engine.download()
    fused, _, _ = _crate(sc, pts, "none")
    fused.run(1)
    fused.synchronize()  # (the host has seen the first tick's big bucket: the next call launches the grouping variants)
    fused.run(2)
    fp, fv, fpr, fids = fused.engine.download()
    assert np.array_equal(fids, sids)
    assert np.array_equal(fp, sp) and np.array_equal(fv, sv) and np.array_equal(fpr, spr)
