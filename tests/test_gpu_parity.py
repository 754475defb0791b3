"""Parity of the HIP path, called through the C ABI, against
  (1) golden vectors captured from the unmodified reference (tests/golden/*.npz),
  (2) the reference's own known-answer tests (tests/test_distance.py:16-70), re-expressed,
  (3) the CPU oracle on seeded inputs.
Bar: integer results (row index, sort permutation, neighbor lists) and every position that feeds a
decision (post wall-fix) bit-exact; float positions / velocities / pressure within 1e-5 relative
(BASELINE.json north_star) -- the tests assert a much tighter 1e-9 where only summation order differs.
"""
import itertools
from math import ceil, floor

import copy

import numpy as np
import pytest

from conftest import golden_names, load_golden
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

RTOL = 1e-5


# ------------------------------------------------------------------ (1) golden: neighbor search
@pytest.mark.parametrize("name", golden_names("nbr_"))
def test_neighbor_search_bit_exact(sc, name):
    g = load_golden(name)
    rows, order, counts, table = sc.neighbor_search(g["particles"], float(g["diameter"]))
    assert np.array_equal(rows, g["y_floored"])
    assert np.array_equal(order, g["sorted_indices"])
    assert np.array_equal(counts, g["counts"])
    assert np.array_equal(table, g["table"])


@pytest.mark.parametrize("name", ["dist_row", "dist_wave"])
def test_points_to_segments_bit_exact(sc, name):
    g = load_golden(name)
    near, dist = sc.points_to_segments_distance(g["particles"], g["segments"])
    assert np.array_equal(near, g["nearest"])
    assert np.array_equal(dist, g["distances"])


def test_pad_segments_host(sc):
    g = load_golden("pad_wave")
    assert np.array_equal(sc.pad_segments(g["segments"], float(g["pad"])), g["padded"])


# ------------------------------------------------------------------ (2) the reference's KATs
PARTICLES_COUNT, SEGMENTS_COUNT = 35, 5


def test_row_distance(sc):  # tests/test_distance.py:16-25
    p = np.array([[i, 0] for i in range(PARTICLES_COUNT)])
    segments = np.array([[[i, -1], [i, 1]] for i in range(SEGMENTS_COUNT)])
    points, distances = sc.points_to_segments_distance(p, segments)
    assert distances.shape == (PARTICLES_COUNT, SEGMENTS_COUNT)
    for i in range(SEGMENTS_COUNT):
        for j in range(PARTICLES_COUNT):
            assert distances[j, i] == abs(j - i)


@pytest.mark.parametrize("diameter,min_neighbors,max_neighbors", [(0.5, 0, 0), (1, 1, 2), (2, 2, 4)])
def test_collider_particles_row(sc, diameter, min_neighbors, max_neighbors):  # :38-48
    p = np.array([[i, 0] for i in range(PARTICLES_COUNT)])
    nb = sc.detect_particle_collisions(p, diameter)
    for i, n in enumerate(nb):
        for j in range(max(0, ceil(i - diameter)), min(floor(i + diameter), PARTICLES_COUNT - 1)):
            assert j in n or j == i
    assert len(nb) == p.shape[0]
    assert all(min_neighbors <= len(n) <= max_neighbors for n in nb)
    assert any(min_neighbors == len(n) for n in nb)
    assert any(max_neighbors == len(n) for n in nb)


@pytest.mark.parametrize("diameter,min_neighbors,max_neighbors", [(0.5, 0, 0), (1, 2, 4), (2, 5, 12)])
def test_collider_particles_grid(sc, diameter, min_neighbors, max_neighbors):  # :51-58
    p = np.array([[i, j] for i, j in itertools.product(range(PARTICLES_COUNT), range(PARTICLES_COUNT))])
    nb = sc.detect_particle_collisions(p, diameter)
    assert len(nb) == p.shape[0]
    assert all(min_neighbors <= len(n) <= max_neighbors for n in nb)
    assert any(min_neighbors == len(n) for n in nb)
    assert any(max_neighbors == len(n) for n in nb)


def test_collider_random_space(sc):  # :61-70
    np.random.seed(0)
    diameter = 0.1
    ps = np.random.rand(PARTICLES_COUNT, 2)
    nb = sc.detect_particle_collisions(ps, diameter)
    for i, p in enumerate(ps):
        if len(nb[i]) == 0:
            continue
        distances = np.linalg.norm(ps[nb[i]] - p, axis=1)
        assert all(d <= diameter * 3 for d in distances)


# ------------------------------------------------------------------ (1) golden: single ticks
def run_engine_tick(sc, g, eta=None, noise="host"):
    from sand_crate_amd import _native as N
    P = len(g["in_particles"])
    eng = sc.Engine(max(P, 1))
    eng.set_noise_mode({"host": N.NOISE_HOST, "none": N.NOISE_NONE}[noise], 0)
    eng.upload(g["in_particles"], g["in_velocities"])
    coef = {k[5:]: (g[k] if g[k].ndim else float(g[k])) for k in g if k.startswith("coef_")}
    eng.set_params(**coef)
    bodies = [(g["body_position"][b], g["body_velocity"][b], float(g["body_omega"][b]), int(g["body_nseg"][b]))
              for b in range(len(g["body_nseg"]))]
    eng.set_segments(g["segments"], sc.pad_segments(g["segments"], coef["particle_radius"]), bodies)
    eng.step_begin()
    stats = eng.step_stats()
    rows, sorted_ids = eng.download_sort()
    ids, counts, nbrs, fixed = eng.download_neighbors()
    if noise == "host":
        eng.set_noise_host(eta)
    eng.step_finish()
    p, v, pr, out_ids = eng.download()
    normals = eng.download_normals()
    eng.close()
    inv = np.argsort(ids)  # sorted slot of each particle id
    return dict(stats=stats, rows=rows, sorted_ids=sorted_ids, counts=counts[inv], table=nbrs[inv], fixed=fixed[inv],
                particles=p, velocities=v, pressure=pr, ids=out_ids, normals=normals)


@pytest.mark.parametrize("name", golden_names("tick_"))
def test_single_tick_matches_reference(sc, name):
    g = load_golden(name)
    out = run_engine_tick(sc, g, eta=g["eta_u01"])
    P = len(g["in_particles"])
    assert out["stats"].particles == P
    assert out["stats"].neighbor_slots == int(g["neighbor_counts"].sum())
    assert out["stats"].wall_particles == int((g["wall_count"] > 0).sum())
    # decisions, bit exact
    assert np.array_equal(out["fixed"], g["fixed_positions"])
    assert np.array_equal(out["counts"], g["neighbor_counts"])
    assert np.array_equal(out["table"], g["neighbor_table"])
    d = 2 * float(g["coef_particle_radius"])
    ref_rows = np.floor(g["fixed_positions"][:, 1] / d).astype(np.int64)
    ref_order = np.lexsort((g["fixed_positions"][:, 0], ref_rows))
    assert np.array_equal(out["sorted_ids"], ref_order)
    assert np.array_equal(out["rows"], ref_rows[ref_order])
    # floats
    assert np.array_equal(out["ids"], np.arange(P))
    np.testing.assert_allclose(out["pressure"], g["out_pressure"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(out["normals"], g["surface_normals"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(out["velocities"], g["out_velocities"], rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(out["particles"], g["out_particles"], rtol=1e-9, atol=1e-12)


# ------------------------------------------------------------------ (1) golden: whole scenes through Crate
@pytest.mark.parametrize("scene", ["stirring_cup", "wave_machine"])
def test_scene_trajectory_matches_reference(sc, scene):
    g = load_golden(f"traj_{scene}")
    crate = sc.Crate(sc.load_config(f"config/{scene}.yaml").world_config)
    ticks = [int(t) for t in g["ticks"]]
    for t in range(1, max(ticks) + 1):
        crate.physics_tick()
        if t in ticks:
            assert crate.particles.shape == g[f"particles_t{t}"].shape, f"particle count differs at tick {t}"
            assert np.array_equal(crate.segments, g[f"segments_t{t}"])
            np.testing.assert_allclose(crate.particles, g[f"particles_t{t}"], rtol=RTOL, atol=1e-9)
            np.testing.assert_allclose(crate.particle_velocities, g[f"velocities_t{t}"], rtol=RTOL, atol=1e-7)
            np.testing.assert_allclose(crate.particles_pressure, g[f"pressure_t{t}"], rtol=RTOL, atol=1e-9)


# ------------------------------------------------------------------ (3) oracle on seeded inputs
def synthetic(n, seed=1234, margin=0.02, vel=0.1):
    """uniform particles, diameter for ~12 neighbors, wave_machine coefficients."""
    rs = np.random.RandomState(seed)
    d = float(np.sqrt(12 / (np.pi * n)))
    p = rs.rand(n, 2) * (1 - 2 * margin) + margin
    v = (rs.rand(n, 2) - 0.5) * vel
    return p, v, d


def wave_world(sc, d, noise_level, warm_ticks=0):
    cfg = sc.load_config("config/wave_machine.yaml")
    co = cfg.world_config.coefficients
    co["particle_radius"] = d / 2
    co["dt"] = 0.002 * (d / 0.01)
    co["collider_noise_level"] = noise_level
    cfg.world_config.particle_sources = []
    return cfg.world_config


@pytest.mark.parametrize("n,noise,margin,vel", [(20000, "none", 0.02, 0.1), (20000, "counter", 0.0, 30.0),
                                                 (65536, "counter", 0.02, 0.1)])
def test_ticks_match_oracle(sc, n, noise, margin, vel):
    """Several consecutive ticks, each checked against the oracle started from the SAME state (the
    GPU's previous output).  Re-synchronising every tick is deliberate: the algorithm is
    ill-conditioned over many ticks -- particles stopped at a wall by the continuous-collision fix
    share x up to an ulp, the sort order inside such a near-tie group decides the neighbor slot, and
    the collider noise is indexed by slot (crate.py:169) -- so two correct float64 implementations
    that differ by 1e-16 in tick t can differ by 1e-2 in tick t+1 for those particles."""
    from oracle.scene import OracleCrate
    from oracle.tick import counter_noise_key, counter_noise_u01, remove_outside, tick_core
    from oracle.world import World
    p, v, d = synthetic(n, seed=n, margin=margin, vel=vel)
    wc = wave_world(sc, d, 0.1 if noise == "counter" else 0.0)
    wc.coefficients["max_particles"] = n
    crate = sc.Crate(wc, noise=noise, noise_seed=77)
    crate.particles = p
    crate.particle_velocities = v
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))
    ids = np.arange(n)
    for t in range(4):
        crate.physics_tick()
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        p, v, ids = remove_outside(p, v, orc.coef["particle_radius"], ids)
        eta = None if noise == "none" else counter_noise_u01(ids, counter_noise_key(77, t))
        out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef, eta_u01=eta)
        gp, gv, gpr, gids = crate.engine.download()
        assert np.array_equal(gids, ids)
        np.testing.assert_allclose(gp, out["particles"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gv, out["velocities"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(gpr, out["pressure"], rtol=1e-9, atol=1e-12)
        p, v = gp, gv


# ------------------------------------------------------------------ edge cases
def test_empty_and_single(sc):
    wc = wave_world(sc, 0.01, 0.1)
    crate = sc.Crate(wc, noise="host")
    crate.physics_tick()  # no particles at all
    assert crate.particle_count == 0 and crate.particles.shape == (0, 2)
    crate.particles = np.array([[0.5, 0.5]])
    crate.particle_velocities = np.array([[0.1, -0.2]])
    crate.physics_tick()
    dt, g = crate.dt, crate.gravity
    v = np.array([0.1, -0.2]) + dt * g
    np.testing.assert_allclose(crate.particle_velocities[0], v, rtol=1e-14)
    np.testing.assert_allclose(crate.particles[0], np.array([0.5, 0.5]) + dt * v, rtol=1e-14)
    assert crate.particles_pressure[0] == 0.0


def test_particles_outside_are_removed(sc):
    wc = wave_world(sc, 0.01, 0.0)
    crate = sc.Crate(wc, noise="none")
    r = crate.particle_radius
    pts = np.array([[0.5, 0.5], [-r * 1.01, 0.5], [0.5, 1 + r * 1.01], [0.3, 0.3], [1 + r * 0.5, 0.5]])
    crate.particles = pts
    crate.particle_velocities = np.zeros_like(pts)
    crate.physics_tick()
    assert crate.particle_count == 3  # crate.py:152: strictly outside [-r, 1+r] only


# ------------------------------------------------------------------ multi-rank slabs on one GPU
@pytest.mark.parametrize("nproc,mixed", [(2, False), (3, False), (2, True)])  # ranks + launcher + this process <= 6 GPU users
def test_slabs_on_gpu_equal_single_gpu(sc, tmp_path, nproc, mixed):
    """The HIP slab path (ownership by column, ghosts, halo pack/unpack, migration) with `nproc`
    gloo ranks sharing cuda:0 must reproduce the single-GPU run bit for bit: every owned particle
    sees the same neighbor list, in the same order, with the same counter noise.  Inside run() every tick
    promises the next one's inputs, so the force kernel packs the halo message and the unpack kernel does the
    wall pass of what it appends; `mixed` alternates that with unpromised ticks (explicit pack, k_wall_bin)."""
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from slab_worker import synthetic_world
    from test_slab_gloo_cpu import run_workers
    n, ticks, vel = 40000, 6, 30.0
    got = run_workers(nproc, tmp_path / "slab.npz", "--backend", "hip", "--particles", str(n), "--ticks", str(ticks),
                      "--vel", str(vel), "--noise", "counter", *(["--mixed"] if mixed else []))
    wc, p, v = synthetic_world(n, 0.1, vel)
    crate = sc.Crate(wc, noise="counter", noise_seed=9, capacity=n + 1024)
    crate.particles = p
    crate.particle_velocities = v
    crate.run(ticks)
    gp, gv, gpr, gids = crate.engine.download()
    assert int(got["count"]) == len(gids)
    assert np.array_equal(got["ids"], gids)
    assert np.array_equal(got["particles"], gp)
    assert np.array_equal(got["velocities"], gv)
    assert np.array_equal(got["pressure"], gpr)


# ------------------------------------------------------------------ full benchmark sizes
def bench_like_crate(sc, n, noise="counter"):
    import bench
    wc, d = bench.world_for(n)
    p, v = bench.synthetic_state(n)
    crate = sc.Crate(wc, noise=noise, noise_seed=1, capacity=n + 1024)
    crate.particles = p
    crate.particle_velocities = v
    return crate, wc, p, v, d


@pytest.mark.parametrize("n,ticks", [(262144, 2), (1048576, 1)])
def test_full_size_tick_matches_oracle(sc, n, ticks):
    """BASELINE.json configs[1] and configs[2] -- 262,144 and 1,048,576 particles, bench.py's exact inputs, counter noise
    (the headline configuration): ticks against the vectorised oracle started from the same state, every float
    compared."""
    from oracle.scene import OracleCrate
    from oracle.tick import counter_noise_key, counter_noise_u01, tick_core
    from oracle.world import World
    crate, wc, p, v, d = bench_like_crate(sc, n)
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))
    ids = np.arange(n)
    for t in range(ticks):
        crate.physics_tick()
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef,
                        eta_u01=counter_noise_u01(ids, counter_noise_key(1, t)))
        gp, gv, gpr, gids = crate.engine.download()
        assert np.array_equal(gids, ids)
        np.testing.assert_allclose(gp, out["particles"], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gv, out["velocities"], rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(gpr, out["pressure"], rtol=1e-9, atol=1e-12)
        p, v = gp, gv


@pytest.mark.parametrize("n", [262144, 1048576])
def test_full_size_properties(sc, n):
    """Size-independent properties at BASELINE.json configs[1] and configs[2] sizes: the sort tap is
    the lexsort of the fixed positions; every listed neighbor is within one diameter; untrimmed lists
    are symmetric; counts match a brute-force count on a sample; trimming happens only at 20."""
    import bench
    wc, d = bench.world_for(n)
    p, v = bench.synthetic_state(n)
    eng = sc.Engine(n)
    from sand_crate_amd import _native as N
    eng.set_noise_mode(N.NOISE_NONE, 0)
    eng.upload(p, v)
    crate_like = sc.Crate(wc, noise="none", capacity=16)  # only to build the tick inputs
    crate_like._engine.close()
    crate_like._engine = eng
    for b in crate_like.rigid_bodies:
        b.apply_velocity(crate_like.dt)
    crate_like._send_tick_inputs()
    eng.step_begin()
    rows, sorted_ids = eng.download_sort()
    ids, counts, nbrs, fixed = eng.download_neighbors()
    eng.step_finish()
    assert len(rows) == n and np.array_equal(np.sort(sorted_ids), np.arange(n))
    # (1) sort order == lexsort((x, row)) of the fixed positions, ties by id
    fx_by_id = np.empty((n, 2))
    fx_by_id[ids] = fixed
    ref_rows = np.floor(fx_by_id[:, 1] / d).astype(np.int64)
    ref_order = np.lexsort((fx_by_id[:, 0], ref_rows))
    assert np.array_equal(sorted_ids, ref_order)
    assert np.array_equal(rows, ref_rows[ref_order])
    # (2) listed neighbors are within d (the reference's inclusive filter), nobody lists itself
    valid = np.arange(20)[None, :] < counts[:, None]
    assert (nbrs[valid] >= 0).all() and (nbrs[~valid] == -1).all()
    src = np.repeat(ids, counts)
    dst = nbrs[valid]
    assert (src != dst).all()
    delta = fx_by_id[dst] - fx_by_id[src]
    assert (np.sqrt(delta[:, 0] ** 2 + delta[:, 1] ** 2) <= d).all()
    assert counts.max() <= 20
    # (3) where neither side was trimmed the relation is symmetric
    cnt_by_id = np.empty(n, dtype=np.int64)
    cnt_by_id[ids] = counts
    both = (cnt_by_id[src] < 20) & (cnt_by_id[dst] < 20)
    fwd = set(zip(src[both].tolist(), dst[both].tolist()))
    assert all((b, a) in fwd for a, b in list(fwd)[:200000])
    # (4) counts equal a brute-force disc count on a sample (min with 20)
    rs = np.random.RandomState(0)
    sample = rs.choice(n, 300, replace=False)
    for i in sample:
        dd = fx_by_id - fx_by_id[i]
        near = int((np.sqrt(dd[:, 0] ** 2 + dd[:, 1] ** 2) <= d).sum()) - 1
        assert cnt_by_id[i] == min(near, 20)
    eng.close()


def test_bench_plain_run_dumps_the_timed_state(sc, tmp_path):
    """bench.py without --full: one JSON line with the contract keys for exactly --steps timed steps, and --dump-outputs
    writes the state its timed path left -- W + K ticks of `Crate.run` on bench.py's inputs, bit for bit."""
    import json
    import subprocess
    import sys
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    n, warmup, steps = 65536, 2, 5
    res = subprocess.run([sys.executable, str(root / "bench.py"), "--particles", str(n), "--steps", str(steps), "--warmup",
                          str(warmup), "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600,
                         cwd=root)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == "particle-steps/sec" and line["unit"] == "particle-steps/s" and line["higher_is_better"]
    assert line["dtype"] == "f64" and line["steps"] == steps and line["repeats"]["count"] == 1
    assert line["value"] * line["ms_per_step"] / 1000.0 == pytest.approx(n)
    assert "roofline" not in line and "regimes" not in line and "cpu_baseline" not in line
    crate, *_ = bench_like_crate(sc, n)
    crate.run(warmup)
    crate.run(steps)
    gp, gv, gpr, gids = crate.engine.download()
    order = np.argsort(gids, kind="stable")
    for name, want in (("particles", gp), ("velocities", gv), ("pressure", gpr), ("ids", gids)):
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64
        assert np.array_equal(got, want[order])


def test_headless_driver_runs_a_variant(sc, tmp_path):
    """the reference's CLI entry, one sweep variant, state recording."""
    from sand_crate_amd.main import main
    summary = main("config/stirring_cup.yaml", tmp_path, variants=1, ticks=30, record_every=10)
    assert summary[0]["ticks"] == 30 and summary[0]["particles"] > 50
    rec = np.load(tmp_path / "variant_00" / "state.npz")
    assert rec["ticks"].tolist() == [10, 20, 30]
    assert rec["particles_2"].shape == (summary[0]["particles"], 2)
    assert (tmp_path / "variant_00" / "config.yaml").exists()


def test_pile_up_buckets_sort_and_rank(sc):
    """Buckets of thousands with exactly equal x (particles stopped on a wall by the continuous-collision
    fix pile up like this): k_sort_big + slot ranking must give the reference's (row, x, id) order and
    lists.  Checked against the oracle (itself pinned by the golden ties / dense cases)."""
    from oracle.neighbors import neighbor_lists, strip_sort
    rs = np.random.RandomState(3)
    d = 0.05
    wall = np.column_stack((np.full(1500, 0.0123), rs.rand(1500) * d * 0.999))          # one cell, 1500 exact-x ties
    corner = np.column_stack((0.06 + np.round(rs.rand(700) * 4) / 400, d + rs.rand(700) * d))  # 5 x values, 700 points
    spread = rs.rand(3000, 2) * 0.6
    pts = np.vstack((wall, corner, spread))
    pts = pts[rs.permutation(len(pts))]
    rows, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(order, ref_order)
    assert np.array_equal(rows, ref_rows)
    ref_counts, ref_table = neighbor_lists(pts, d)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(table, ref_table)


@pytest.mark.parametrize("origin", [0.0, 3.0, 1000.0])
def test_pairs_at_the_edge_of_the_window(sc, origin):
    """Pairs whose |dx| is within rounding of d -- a lattice of spacing d, the same with the spacing one ulp and 1e-7 d
    off either way, rows of such lattices at dy = 0 and just above -- are decided by the reference's window
    expressions x_i +- d / x_j +- d (collision_detector.py:85-88, :106-119) AND its distance predicate.  Pass A
    evaluates the window expression only for a batch with a hit that close to the edge (World::dsafe): here nearly
    every hit is one.  Small and large coordinates (the rounding of x +- d grows with |x|): lists == oracle."""
    from oracle.neighbors import neighbor_lists, strip_sort
    d = 0.05
    rows = []
    for r, (step, dy) in enumerate([(d, 0.0), (np.nextafter(d, 1.0), 0.0), (np.nextafter(d, 0.0), 0.0), (d * (1 + 1e-7), 0.0),
                                     (d * (1 - 1e-7), 0.0), (d, 1e-9), (d * (1 - 1e-12), 3e-8), (d, d * 1e-4)]):
        k = np.arange(90)
        x = origin + 0.013 + k * step
        y = origin + 0.017 + 3 * r * d + np.where(k % 2 == 0, 0.0, dy)
        rows.append(np.column_stack((x, y)))
    rs = np.random.RandomState(int(origin) + 1)
    pts = np.vstack(rows + [origin + rs.rand(3000, 2) * 4.0])
    pts = pts[rs.permutation(len(pts))]
    rows_, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(order, ref_order)
    ref_counts, ref_table = neighbor_lists(pts, d)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(table, ref_table)


def test_buckets_of_many_sorted_chunks_rank_together(sc):
    """Buckets of many sorted chunks (k_sort_big sorts 1024 slots at a time): k_reorder takes a particle's rank as its
    position in its own chunk plus a binary search in each of the others, the searches advancing kRankSide = 4 chunks at
    a time -- 7 chunks (two groups), 36 chunks (nine groups), exact ties in x, near-ties that spread two chunks
    differently, and buckets whose starts make the waves straddle chunks and buckets.  The order must be the
    reference's (row, x, id)."""
    from oracle.neighbors import strip_sort
    rs = np.random.RandomState(5)
    d = 0.05
    def cell(col, row):
        return np.array([col * d, row * d])
    parts = [
        cell(3, 4) + np.column_stack((np.round(rs.rand(7013) * 40) / 40 * d * 0.9, rs.rand(7013) * d * 0.99)),   # 41 x values: ties
        cell(4, 4) + rs.rand(37, 2) * d * 0.99,                                                                   # its neighbor: small
        cell(5, 4) + np.column_stack((rs.rand(36100) ** 3 * d * 0.99, rs.rand(36100) * d * 0.99)),                # 36 chunks, skewed in x
        cell(6, 4) + np.column_stack((np.full(6500, 0.0321 * d), rs.rand(6500) * d * 0.99)),                      # one x: ranked by id alone
        cell(9, 9) + np.column_stack((np.where(rs.rand(9000) < 0.5, 0.1, 0.9) * d + rs.rand(9000) * 1e-12, rs.rand(9000) * d * 0.99)),
        rs.rand(4000, 2) * 0.9 + 0.02,
    ]
    pts = np.vstack(parts)
    pts = pts[rs.permutation(len(pts))]
    rows, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(order, ref_order)
    assert np.array_equal(rows, ref_rows)


@pytest.mark.parametrize("seed,tile", [(11, "narrow"), (12, "wide")])
def test_dense_regions_windowed_search(sc, seed, tile, monkeypatch):
    """Tiles too large for LDS are searched through a sliding window; every kind of scan must keep the
    reference's order: piles spread over x and y (partial hits), sparse particles that walk a
    whole pile in the next / previous row with hardly a hit, piles that span several rows and columns,
    a tile that ends inside a pile."""
    from oracle.neighbors import neighbor_lists, strip_sort
    monkeypatch.setenv("SANDCRATE_TILE", tile)  # read by sc_create: both pass A tile sizes, whatever the grid
    rs = np.random.RandomState(seed)
    d = 0.04
    parts = [
        np.column_stack((0.40 + rs.rand(1300) * d * 2.2, 0.40 + rs.rand(1300) * d * 0.98)),     # 2+ cells wide, one row
        np.column_stack((0.40 + rs.rand(40) * d * 3.0, 0.40 + d + rs.rand(40) * d)),            # sparse row below it
        np.column_stack((0.40 + rs.rand(40) * d * 3.0, 0.40 - d + rs.rand(40) * d)),            # sparse row above it
        np.column_stack((0.12 + rs.rand(900) * d * 0.5, 0.08 + rs.rand(900) * d * 3.0)),        # a tall pile: 3 rows
        np.column_stack((0.80 + rs.rand(700) * 1e-9, 0.20 + rs.rand(700) * d * 0.2)),           # near-ties in x
        np.column_stack((0.80 + rs.rand(600) * d, 0.20 + d + rs.rand(600) * d)),                # dense row under the ties
        rs.rand(2500, 2) * 0.9 + 0.02,
    ]
    pts = np.vstack(parts)
    pts = pts[rs.permutation(len(pts))]
    rows, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(order, ref_order)
    ref_counts, ref_table = neighbor_lists(pts, d)
    assert np.array_equal(counts, ref_counts)
    assert np.array_equal(table, ref_table)
    assert (counts < 20).sum() > 1000 and (counts == 20).sum() > 2000


def test_pile_up_state_ticks_with_bucket_sort(sc):
    """The same through the tick path: the second tick is launched with the big-bucket hint set."""
    rs = np.random.RandomState(4)
    wc = wave_world(sc, 0.02, 0.1)
    wc.coefficients["max_particles"] = 6000
    d = 0.02
    pile = np.column_stack((np.full(2500, 0.31), 0.5 + rs.rand(2500) * d * 0.9))
    rest = rs.rand(3000, 2) * 0.8 + 0.1
    pts = np.vstack((pile, rest))
    crate = sc.Crate(wc, noise="none")
    crate.particles = pts
    crate.particle_velocities = np.zeros_like(pts)
    eng = crate.engine
    for t in range(3):
        for b in crate.rigid_bodies:
            b.apply_velocity(crate.dt)
        crate._send_tick_inputs()
        eng.step_begin()
        rows, sorted_ids = eng.download_sort()
        ids, counts, nbrs, fixed = eng.download_neighbors()
        fx = np.empty((len(ids), 2))
        fx[np.argsort(np.argsort(ids))] = fixed  # placeholder shape; real mapping below
        by_id = {int(i): k for k, i in enumerate(ids)}
        live_ids = np.sort(ids)
        pos = np.array([fixed[by_id[int(i)]] for i in live_ids])
        r = np.floor(pos[:, 1] / d).astype(np.int64)
        ref = live_ids[np.lexsort((live_ids, pos[:, 0], r))]
        assert np.array_equal(sorted_ids, ref), f"tick {t}"
        eng.step_finish()
        crate._state_changed()


# ------------------------------------------------------------------ C-ABI contract: errors and edge cases
def test_abi_error_behaviour(sc):
    """include/sandcrate_hip.h: every entry point returns a code, the message is sc_last_error(), nothing
    throws across the boundary; the binding turns codes into NativeError."""
    from sand_crate_amd import _native as N
    eng = sc.Engine(64)
    with pytest.raises(N.NativeError, match="sc_set_params"):
        eng.step_begin()                                   # inputs missing
    wc = wave_world(sc, 0.02, 0.0)
    co = {k: wc.coefficients[k] for k in ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier",
                                          "ignored_pressure", "collider_noise_level", "viscosity", "surface_smoothing",
                                          "target_pressure", "gravity")}
    eng.set_params(**co)
    with pytest.raises(N.NativeError, match="sc_step_begin first"):
        eng.step_finish()                                  # call order
    with pytest.raises(N.NativeError) as e:
        eng.upload(np.zeros((65, 2)), np.zeros((65, 2)))   # beyond the context capacity
    assert e.value.code == -3
    seg = np.zeros((17, 2, 2))
    with pytest.raises(N.NativeError) as e:
        eng.set_segments(seg, np.zeros((34, 2, 2)), [((0, 0), (0, 0), 0.0, 17)])
    assert e.value.code == -3                              # SC_MAX_SEGMENTS
    eng.set_noise_mode(N.NOISE_HOST, 0)
    eng.upload(np.array([[0.5, 0.5], [0.505, 0.5]]), np.zeros((2, 2)))
    eng.set_segments(np.zeros((0, 2, 2)), np.zeros((0, 2, 2)), [])
    eng.step_begin()
    with pytest.raises(N.NativeError, match="twice"):
        eng.step_begin()
    with pytest.raises(N.NativeError, match="sc_set_noise_host"):
        eng.step_finish()                                  # host noise not supplied
    st = eng.step_stats()
    assert (st.particles, st.neighbor_slots, st.max_neighbors) == (2, 2, 1)
    eng.set_noise_host(np.full((2, 2), 0.5))
    eng.step_finish()
    with pytest.raises(N.NativeError, match="SC_NOISE_HOST"):
        eng.step(1)
    p, v, pr, ids = eng.download()
    assert len(p) == 2 and ids.tolist() == [0, 1]
    eng.close()


def test_nan_particle_is_dropped_and_reported(sc):
    """crate.py:206 divides by the distance to the wall; a particle exactly ON a wall becomes NaN in
    the reference and lives on as NaN.  Here it is dropped and the next synchronising call says so."""
    from sand_crate_amd import _native as N
    wc = wave_world(sc, 0.02, 0.0)
    crate = sc.Crate(wc, noise="none")
    crate.particles = np.array([[0.0, 0.5], [0.5, 0.5], [0.6, 0.6]])   # the first one sits on the left wall
    crate.particle_velocities = np.zeros((3, 2))
    crate.physics_tick()
    with pytest.raises(N.NativeError) as e:
        crate.synchronize()
    assert e.value.code == N.ERR_DOMAIN and "NaN" in str(e.value)
    assert crate.particle_count == 2


def test_a_scan_that_gives_up_skips_the_tick(sc):
    """The bucket scan's workgroups wait for the workgroups before them, bounded (sc_set_scan_patience).  One that gives
    up abandons the tick: every later kernel returns at once, the particles stay as the tick found them -- through the
    ticks that were queued behind it too -- and the next synchronising call says so; after that the run goes on from
    that state."""
    from sand_crate_amd import _native as N
    crate, wc, p, v, d = bench_like_crate(sc, 262144)   # (a grid of 264 x 264 cells: 35 workgroups in the scan)
    crate.run(2)
    crate.synchronize()
    before = crate.engine.download()
    crate.engine.set_scan_patience(-1)                  # every workgroup but the first gives up without having looked
    crate.run(3)
    with pytest.raises(N.NativeError) as e:
        crate.synchronize()
    assert e.value.code == N.ERR_HIP and "bucket scan" in str(e.value) and "skipped" in str(e.value)
    after = crate.engine.download()
    # velocities and ids exactly; positions too -- but for the hard wall fix of the abandoned tick's first kernel, which
    # runs ahead of the scan and in place (crate.py:202-211: a particle closer than r to a wall is set to r; applying it
    # again changes nothing).  (The pressures are an output of the tick that did not happen.)
    assert np.array_equal(before[1], after[1]) and np.array_equal(before[3], after[3])
    moved = np.flatnonzero((before[0] != after[0]).any(axis=1))
    r = crate.particle_radius
    # (the motored wall kept moving through the abandoned ticks -- the host runs the bodies -- and pushed what it reached)
    assert len(moved) < 0.01 * len(p) and np.abs(before[0][moved] - after[0][moved]).max(initial=0.0) <= 1.2 * r
    crate.engine.set_scan_patience(1 << 22)
    crate.run(2)                                        # ... and the run goes on from there
    crate.synchronize()
    moved = crate.engine.download()
    assert len(moved[0]) == len(p) and not np.array_equal(moved[0], before[0])


def test_live_coefficient_edits_take_effect(sc):
    """playback.py:150-153, :221-226: gravity and coefficients are edited between ticks."""
    wc = wave_world(sc, 0.01, 0.0)
    crate = sc.Crate(wc, noise="none")
    crate.particles = np.array([[0.5, 0.5]])
    crate.particle_velocities = np.zeros((1, 2))
    crate.physics_tick()
    v1 = crate.particle_velocities[0].copy()
    np.testing.assert_allclose(v1, crate.dt * crate.gravity, rtol=1e-14)
    crate.gravity = np.array([3.0, -1.0])
    setattr(crate, "dt", 0.001)
    crate.physics_tick()
    np.testing.assert_allclose(crate.particle_velocities[0], v1 + 0.001 * np.array([3.0, -1.0]), rtol=1e-14)


def test_crate_grows_beyond_its_initial_capacity(sc):
    wc = wave_world(sc, 0.01, 0.0)
    crate = sc.Crate(wc, noise="none", capacity=16)
    rs = np.random.RandomState(2)
    pts = rs.rand(500, 2) * 0.8 + 0.1
    crate.particles = pts
    crate.particle_velocities = np.zeros_like(pts)
    crate.physics_tick()
    assert crate.particle_count == 500


# ------------------------------------------------------------------ look-ahead (fused next-tick wall pass)
@pytest.mark.parametrize("margin,vel", [(0.02, 0.1), (0.0, 25.0)])
def test_run_with_lookahead_equals_tick_by_tick(sc, margin, vel):
    """Crate.run(k) promises every next tick's inputs (sc_set_next_inputs), so pass B also does the next
    tick's removal / wall contacts / wall fix / bucket counts.  It must be the same computation as k
    separate physics_tick() calls, bit for bit -- with a moving wall, wall contacts and removals."""
    n = 30000
    p, v, d = synthetic(n, seed=21, margin=margin, vel=vel)
    a = sc.Crate(wave_world(sc, d, 0.1), noise="counter", noise_seed=5, capacity=n + 16)
    b = sc.Crate(wave_world(sc, d, 0.1), noise="counter", noise_seed=5, capacity=n + 16)
    for c in (a, b):
        c.particles = p
        c.particle_velocities = v
    a.run(7)
    for _ in range(7):
        b.physics_tick()
    pa, va, pra, ida = a.engine.download()
    pb, vb, prb, idb = b.engine.download()
    assert np.array_equal(ida, idb)
    assert np.array_equal(pa, pb) and np.array_equal(va, vb) and np.array_equal(pra, prb)
    assert np.array_equal(a.segments, b.segments) and a.tick == b.tick == 7
    # and the two styles can be mixed
    a.physics_tick()
    b.run(1)
    assert np.array_equal(a.engine.download()[0], b.engine.download()[0])


def test_lookahead_promise_is_binding(sc):
    from sand_crate_amd import _native as N
    wc = wave_world(sc, 0.02, 0.0)
    crate = sc.Crate(wc, noise="none")
    rs = np.random.RandomState(0)
    pts = rs.rand(200, 2) * 0.8 + 0.1
    crate.particles = pts
    crate.particle_velocities = np.zeros_like(pts)
    eng = crate.engine
    crate._send_tick_inputs()
    eng.step_begin()
    coef = {name: getattr(crate, name) for name in ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier",
                                                    "ignored_pressure", "collider_noise_level", "viscosity",
                                                    "surface_smoothing", "target_pressure")}
    bodies = [(b.position, b.center_velocity, b.angular_clockwise_velocity, len(b)) for b in crate.rigid_bodies]
    eng.set_next_inputs(gravity=crate.gravity, segments=crate.segments, bodies=bodies, **coef)
    eng.step_finish()
    with pytest.raises(N.NativeError, match="promised"):
        eng.append(np.array([[0.5, 0.5]]), np.zeros((1, 2)))       # no new particles before the promised tick
    crate.particle_radius = 0.011                                    # different walls/grid than promised
    crate._send_tick_inputs()
    with pytest.raises(N.NativeError, match="promised"):
        eng.step_begin()
    crate.particle_radius = 0.01
    crate._send_tick_inputs()
    eng.step_begin()                                                 # the promised inputs: fine
    eng.step_finish()
    assert eng.count() == 200


# ------------------------------------------------------------------ RCCL transport (one rank talking to itself)
def test_rccl_transport_moves_halo_buffers_in_stream_order(sc):
    """sc_comm_init / sc_halo_exchange on the only GPU there is here: a one-rank communicator whose left and
    right neighbor is the rank itself (tests/rccl_worker.py, in a fresh process so that torch initialises the
    GPU first, as in bench.py).  Proves the dlopen()ed RCCL entry points, the group of two send/recv pairs and
    the ordering with the packing kernel on the same stream; the multi-rank pairing cannot be run on one device
    (RCCL refuses two ranks per GPU)."""
    import subprocess
    import sys
    from pathlib import Path
    worker = Path(__file__).resolve().parent / "rccl_worker.py"
    res = subprocess.run([sys.executable, str(worker)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    assert "RCCL_SELF_EXCHANGE_OK" in res.stdout


def test_hud_shows_kernel_times(sc):
    """N4 of SURVEY.md section 8f: `debug_prints` keeps the reference's layout (crate.py:131-136, timer.py:37-48):
    tick, particle count, a `Timing` block -- per kernel when asked for -- `FPS`, the coefficients."""
    import yaml
    cfg = sc.load_config("config/stirring_cup.yaml")
    crate = sc.Crate(cfg.world_config)
    crate.show_kernel_times()
    for _ in range(12):
        crate.physics_tick()
    text = crate.debug_prints
    assert text.startswith("Tick: 12\nParticles: ")
    head = yaml.safe_load(text.split("\n\n")[0].split("\n", 2)[2])
    assert {"force_integrate", "reorder", "wall_bin"} <= set(head["Timing"]) and "FPS" in head
    assert all("ms" in v for v in head["Timing"].values())
    crate.show_kernel_times(False)
    crate.physics_tick()
    assert "force_integrate" not in crate.debug_prints and "particle_radius" in crate.debug_prints


# ------------------------------------------------------------------ more edge cases of the machinery
def _coef_of(crate):
    return {k: getattr(crate, k) for k in ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier",
                                           "ignored_pressure", "collider_noise_level", "viscosity", "surface_smoothing",
                                           "target_pressure")}


def test_lookahead_survives_a_promised_radius_change(sc):
    """The promised tick may have another particle radius: another cell grid (re-allocated when it grows),
    other wall thresholds.  sc_tick(now, next) + sc_tick(next) must equal two unpromised ticks."""
    from sand_crate_amd.crate import tick_geometry
    n = 20000
    p, v, d = synthetic(n, seed=31, margin=0.02, vel=2.0)
    results = []
    for promised in (True, False):
        crate = sc.Crate(wave_world(sc, d, 0.1), noise="counter", noise_seed=3, capacity=n + 16)
        crate.particles, crate.particle_velocities = p, v
        eng = crate.engine
        packs = []
        for radius in (d / 2, d / 2 * 0.8, d / 2 * 1.1):
            for b in crate.rigid_bodies:
                b.apply_velocity(crate.dt)
            crate.particle_radius = radius
            seg, pad, bodies = tick_geometry(crate.rigid_bodies, radius, {})
            packs.append(eng.pack_inputs(_coef_of(crate), crate.gravity, seg, pad, bodies))
        for k, now in enumerate(packs):
            eng.tick(now, packs[k + 1] if promised and k + 1 < len(packs) else None)
        results.append(eng.download())
    for a, b in zip(*results):
        assert np.array_equal(a, b)


def test_tick_reports_a_bad_promise_and_stays_usable(sc):
    from sand_crate_amd import _native as N
    from sand_crate_amd.crate import tick_geometry
    wc = wave_world(sc, 0.02, 0.0)
    crate = sc.Crate(wc, noise="none")
    pts = np.random.RandomState(1).rand(300, 2) * 0.8 + 0.1
    crate.particles, crate.particle_velocities = pts, np.zeros_like(pts)
    eng = crate.engine
    seg, pad, bodies = tick_geometry(crate.rigid_bodies, crate.particle_radius, {})
    good = eng.pack_inputs(_coef_of(crate), crate.gravity, seg, pad, bodies)
    many = np.tile(seg, (5, 1, 1))[:33]                       # 33 segments: one more than the library takes
    bad = eng.pack_inputs(_coef_of(crate), crate.gravity, many, sc.pad_segments(many, crate.particle_radius),
                          [((0, 0), (0, 0), 0.0, 33)])
    with pytest.raises(N.NativeError, match="segments"):
        eng.tick(good, bad)
    eng.tick(good, good)                                       # the tick itself was completed; carry on
    eng.tick(good)
    assert eng.count() == 300


def test_more_big_buckets_than_the_rank_kernel_lists(sc):
    """4400 cells of 100 particles each, with x ties: 4400 one-chunk tasks for k_sort_big, whose list holds
    kMaxSortTasks = 16,384 tasks (it held 4096 buckets when this test was written, and the rest was ranked inside the
    reorder kernel by counting: a list that overflows is tests/test_gpu_sort_cases.py's `overflow` now).  The sorted order
    must be the reference's."""
    from oracle.neighbors import strip_sort
    rs = np.random.RandomState(8)
    d, side, ncell = 0.01, 90, 4400
    cells = rs.permutation(side * side)[:ncell]
    cx, cy = (cells % side + 2) * d, (cells // side + 2) * d
    pts = np.column_stack(((cx[:, None] + np.round(rs.rand(ncell, 100) * 8) / 8 * d * 0.9).ravel(),
                           (cy[:, None] + rs.rand(ncell, 100) * d * 0.99).ravel()))
    pts = pts[rs.permutation(len(pts))]
    rows, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(rows, ref_rows) and np.array_equal(order, ref_order)
    assert counts.min() == 20                                  # every particle has a full list in such a cell


def test_halo_buffer_overflow_is_reported(sc, tmp_path):
    """A halo message that cannot hold the band is never silently truncated: the ranks fail with the
    library's message at the next synchronising call."""
    import subprocess
    import sys
    from pathlib import Path
    sys.path.insert(0, str(Path(__file__).resolve().parent))
    from test_slab_gloo_cpu import free_port
    root = Path(__file__).resolve().parent.parent
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), str(root / "tests" / "slab_worker.py"), "--out", str(tmp_path / "x.npz"),
           "--backend", "hip", "--particles", "40000", "--ticks", "3", "--halo-capacity", "64"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode != 0
    assert "a halo buffer was too small" in res.stderr


# ------------------------------------------------------------------ randomised worlds
@pytest.mark.parametrize("seed", range(10))
def test_random_worlds_match_oracle(sc, seed):
    """Worlds the two YAML scenes do not have: several fixed bodies with slanted segments inside the box, up
    to two motored bodies that translate and spin, random coefficients and gravity direction,
    particles all over the box (some inside bodies, some touching several segments at once).  Three ticks,
    each against the oracle restarted from the GPU's previous state (see test_ticks_match_oracle)."""
    from oracle.scene import OracleCrate
    from oracle.tick import counter_noise_key, counter_noise_u01, remove_outside, tick_core
    from oracle.world import World
    rs = np.random.RandomState(1000 + seed)
    n = int(rs.randint(1500, 6000))
    d = float(np.sqrt(rs.uniform(4, 14) / (np.pi * n)))
    cfg = sc.load_config("config/wave_machine.yaml")
    wc = cfg.world_config
    co = wc.coefficients
    co.update(particle_radius=d / 2, dt=0.002 * d / 0.01 * rs.uniform(0.5, 2.0), max_particles=n,
              collider_noise_level=float(rs.choice([0.0, 0.1, 0.3])), viscosity=float(rs.uniform(0, 12)),
              pressure_amplifier=float(rs.uniform(5, 60)), ignored_pressure=float(rs.uniform(0, 0.6)),
              surface_smoothing=float(rs.uniform(0, 150)), target_pressure=float(rs.uniform(-4, 2)),
              wall_collision_decay=float(rs.uniform(0, 0.9)), gravity=[float(g) for g in rs.uniform(-9.8, 9.8, 2)])
    wc.particle_sources = []
    bodies = [wc.rigid_bodies[0]]  # the box
    for _ in range(rs.randint(1, 4)):
        k = int(rs.randint(1, 4))
        pts = rs.rand(k + 1, 2) * 0.6 + 0.2
        bodies.append({"fixed": {"name": "obstacle", "segments": [[pts[j].tolist(), pts[j + 1].tolist()] for j in range(k)]}})
    for _ in range(rs.randint(0, 3)):
        a, b, w0 = rs.uniform(-2, 2), rs.uniform(1, 9), rs.uniform(-3, 3)
        bodies.append({"motored": {"name": "paddle", "segments": [[[0.0, 0.0], [0.0, -1.0]], [[0.0, 0.0], [-1.0, 0.0]]],
                                   "velocity_func": f"lambda t: np.array([np.sin(t * {b}) * {a}, {a} * 0.3])",
                                   "angular_velocity_func": f"lambda t: np.cos(t * {b}) * {w0}",
                                   "scale": [float(rs.uniform(0.02, 0.2)), float(rs.uniform(0.1, 0.5))],
                                   "rotation": float(rs.uniform(-180, 180)),
                                   "position": [float(rs.uniform(0.2, 0.8)), float(rs.uniform(0.2, 0.8))]}})
    wc.rigid_bodies = bodies
    noise = "counter" if co["collider_noise_level"] > 0 else "none"
    p = rs.rand(n, 2) * 0.98 + 0.01
    v = (rs.rand(n, 2) - 0.5) * rs.choice([0.1, 3.0, 30.0])
    crate = sc.Crate(wc, noise=noise, noise_seed=seed)
    crate.particles, crate.particle_velocities = p, v
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))
    ids = np.arange(n)
    for t in range(3):
        crate.physics_tick()
        for b in orc.rigid_bodies:
            b.advance(orc.coef["dt"])
        assert np.array_equal(crate.segments, orc.segments)
        p, v, ids = remove_outside(p, v, orc.coef["particle_radius"], ids)
        eta = None if noise == "none" else counter_noise_u01(ids, counter_noise_key(seed, t))
        out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef, eta_u01=eta)
        gp, gv, gpr, gids = crate.engine.download()
        keep = ~np.isnan(out["particles"]).any(axis=1)   # the reference keeps NaN particles, the library drops them
        assert np.array_equal(gids, ids[keep])
        np.testing.assert_allclose(gp, out["particles"][keep], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(gv, out["velocities"][keep], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(gpr, out["pressure"][keep], rtol=1e-9, atol=1e-12)
        p, v, ids = gp, gv, gids


# ------------------------------------------------------------------ one gigantic bucket (tiles beyond 65,535 entries)
from tile_cases import cluster_lists as _cluster_lists  # noqa: E402  (the closed form lives with the tile worlds)


def test_one_gigantic_bucket(sc):
    """70,000 particles in a patch of one cell: the blocks inside it have tiles of more than 65,535 entries,
    whose neighbor entries are sorted indices in the 32-bit table instead of 16-bit tile slots.  Sort, lists
    (k_sort_big: dozens of sorted chunks, ranks by binary search across them; the direct search) and one full tick through that table."""
    from oracle.neighbors import strip_sort
    from oracle.scene import OracleCrate
    from oracle.tick import tick_core
    from oracle.world import World
    rs = np.random.RandomState(12)
    d, n = 0.05, 70000
    pts = np.column_stack((0.5 + rs.rand(n) * d * 0.3, 0.5 + 0.01 + rs.rand(n) * d * 0.3))
    rows, order, counts, table = sc.neighbor_search(pts, d)
    ref_rows, ref_order = strip_sort(pts, d)
    assert np.array_equal(rows, ref_rows) and np.array_equal(order, ref_order)
    ref_counts, ref_table = _cluster_lists(pts, d)
    assert np.array_equal(counts, ref_counts) and np.array_equal(table, ref_table)
    wc = wave_world(sc, d, 0.0)
    wc.coefficients["max_particles"] = n
    crate = sc.Crate(wc, noise="none")
    crate.particles, crate.particle_velocities = pts, np.zeros_like(pts)
    crate.physics_tick()
    orc = OracleCrate(World(wc.rigid_bodies, [], dict(wc.coefficients)))
    for b in orc.rigid_bodies:
        b.advance(orc.coef["dt"])
    out = tick_core(pts, np.zeros_like(pts), orc.segments, orc.body_states(), orc.coef,
                    neighbor_fn=lambda p, dd: _cluster_lists(p, dd))
    gp, gv, gpr, gids = crate.engine.download()
    assert np.array_equal(gids, np.arange(n))
    np.testing.assert_allclose(gpr, out["pressure"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(gv, out["velocities"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(gp, out["particles"], rtol=1e-9, atol=1e-12)


def test_run_zero_ticks_is_a_no_op(sc):
    crate = sc.Crate(wave_world(sc, 0.02, 0.0), noise="none")
    pts = np.random.RandomState(2).rand(100, 2) * 0.8 + 0.1
    crate.particles, crate.particle_velocities = pts, np.zeros_like(pts)
    seg = crate.segments.copy()
    crate.run(0)
    assert crate.tick == 0 and np.array_equal(crate.segments, seg) and np.array_equal(crate.particles, pts)
