"""The force pair's arithmetic at the edges of its pair math (tests/force_cases.py), against the oracle.

Every world puts one rule of pass A's pair math, of pass B or of pair_offset in charge of the result: particles at one
point (rsqrt_nr(0) = NaN, overlap 1, a finite pressure), noise that pushes most listed neighbors beyond d (the upper
clip), a clamp that acts on half a cloud and an empty list under a negative ignored_pressure, one term of the folded
weights at a time and their corners, every list length in a tile of each regime of the tiled passes, ids up to 2^31 - 2,
V = 1 and V = 2 under pressure.  Each of two ticks is checked against the oracle restarted from the device's previous
state: the sort, the rows, the wall-fixed positions, the lists and the surviving ids bit for bit; positions, pressures
and the surface normals to rtol 1e-9, atol 1e-12, velocities to atol 1e-11 -- the tolerances of
test_single_tick_matches_reference.  A second context runs the same ticks with every next tick's inputs promised (the
fused path of Crate.run) and is held to the first bit for bit.  Host noise goes through step_begin / step_stats /
set_noise_host with the block in particle-major, slot-minor order.
tests/test_force_cases_cpu.py proves on the oracle alone that every world has the property it is named for, that none
but the noise-free piles ever has a NaN row -- so `keep = ~isnan` hides nothing --, and that each is well-conditioned;
the property is asserted again here on the oracle's first tick."""
import numpy as np
import pytest

import force_cases as fc
import test_force_cases_cpu as premises
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

COEF = ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
        "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure")
PHASES = ("tension", "gravity", "pressure", "viscosity", "wall_bounce", "continuous_collision")


class Blocks:
    """The host's generator, remembering the block of the last draw: the oracle draws it, the device is given the same."""

    def __init__(self, seed):
        self.rs, self.last = np.random.RandomState(seed), np.zeros((0, 2))

    def rand(self, *shape):
        self.last = self.rs.rand(*shape)
        return self.last


def expect_nan_report(eng):
    """The NaN rows the last tick left were dropped: the first synchronising call says so, once."""
    from sand_crate_amd import _native as N
    with pytest.raises(N.NativeError) as e:
        eng.synchronize()
    assert e.value.code == N.ERR_DOMAIN and "NaN" in str(e.value)
    eng.synchronize()


def phase_means(out, v0, coef):
    """Mean |dv| of the six force phases (force_monitor.py:23-33 around crate.py:110-123) from the oracle's tick."""
    dt, g = coef["dt"], np.asarray(coef["gravity"], dtype=np.float64)
    norm = lambda a: float(np.mean(np.sqrt(a[:, 0] ** 2 + a[:, 1] ** 2)))  # noqa: E731
    return {"tension": norm(out["v_after_tension"] - v0),
            "gravity": float(np.sqrt(((dt * g) ** 2).sum())),
            "pressure": norm(out["v_after_pressure"] - (out["v_after_tension"] + dt * g[None])),
            "viscosity": norm(out["v_after_viscosity"] - out["v_after_pressure"]),
            "wall_bounce": norm(out["v_after_bounce"] - out["v_after_viscosity"]),
            "continuous_collision": norm(out["v_after_bounce"] * out["ccd_factor"][:, None] - out["v_after_bounce"])}


def drive(sc, name, noise, fused=True, monitor=False, ticks=fc.TICKS):
    """`ticks` device ticks of the case, each compared with the oracle's tick on the device's previous state.
    fused: a second context runs the same ticks with every next tick's inputs promised; its taps, velocities, pressures
    and ids must equal the first context's bit for bit every tick, its whole state after the last.  (Between promised
    ticks a context holds the positions after the NEXT tick's wall fix.)
    monitor: a further context runs them with the force monitor on -- another instantiation of pass B --: its state must
    equal the plain one's bit for bit, its six phase means the oracle's.
    A tick that leaves NaN rows (the piles without noise) is reported by the tick that drops them -- the next one, or the
    fused epilogue of the same -- at its first synchronising call, once: expected here, and nowhere else."""
    from oracle.neighbors import strip_sort
    from sand_crate_amd import _native as N
    case = fc.CASES[name]()
    orc = case.oracle()
    coef = fc.coefficients(case, noise)
    seg, st = orc.segments, orc.body_states()   # a fixed box: the same walls every tick
    bodies = [(b.position, b.center_velocity, b.omega, b.n_segments) for b in st]
    cf = {k: coef[k] for k in COEF}
    r, d = coef["particle_radius"], case.d
    n = len(case.p)
    kinds = ["plain"] + (["fused"] if fused else []) + (["monitor"] if monitor else [])
    engines = {}
    for kind in kinds:
        eng = sc.Engine(n + 64)
        eng.set_noise_mode({"none": N.NOISE_NONE, "counter": N.NOISE_COUNTER, "host": N.NOISE_HOST}[noise], fc.SEED)
        if case.upload_order is None:
            eng.upload(case.p, case.v)
        else:
            o = case.upload_order
            eng.upload_with_ids(case.p[o], case.v[o], case.ids[o])
        if kind == "monitor":
            eng.enable_force_monitor(True)
        engines[kind] = eng
    host = Blocks(fc.HOST_SEED)
    state = (case.p, case.v, case.ids)
    dropped_before = False                      # the previous tick left NaN rows
    for t in range(ticks):
        where = f"{name} {noise} tick {t}"
        (p, v, ids), out = fc.oracle_tick(case, noise, t, state, host)
        nan = np.isnan(out["particles"]).any(axis=1)
        if t == 0 and noise == case.noises[0]:  # the case's property, on the first noise it runs with
            premises.PREMISES[name]((p, v, ids), out)
        if (name, noise) != ("pile_pairs", "none") or t > 0:
            assert not nan.any() and not premises.has_nan(out), where
        assert nan.sum() < 0.1 * len(p), where  # what `keep` below may hide
        keep = ~nan
        taps, got = {}, {}
        for kind, eng in engines.items():
            promised = kind == "fused" and t + 1 < ticks
            eng.set_params(gravity=coef["gravity"], **cf)
            eng.set_segments(seg, sc.pad_segments(seg, r), bodies)
            eng.step_begin()
            if dropped_before and not (kind == "fused"):
                expect_nan_report(eng)          # this tick's wall pass dropped them
            s = eng.step_stats()
            assert s.flags == 0, where
            taps[kind] = ((s.particles, s.wall_particles, s.neighbor_slots), *eng.download_sort(), *eng.download_neighbors())
            if noise == "host":
                assert len(host.last) == s.neighbor_slots, where
                eng.set_noise_host(host.last)
            if promised:
                eng.set_next_inputs(gravity=coef["gravity"], segments=seg, bodies=bodies, **cf)
            eng.step_finish()
            if kind == "plain":                 # taps of the finished tick: every row, those it left NaN included
                got["normals"], got["pressure"] = eng.download_normals(), eng.download_pressure()
            if promised and nan.any():
                expect_nan_report(eng)          # the fused epilogue ran the next tick's wall pass
            got[kind] = eng.download()
        # ---- the plain context against the oracle
        (particles, wall_particles, slots), rows, sorted_ids, slot_ids, counts, nbrs, fixed = taps["plain"]
        assert particles == len(p) and slots == int(out["neighbor_counts"].sum()), where
        assert wall_particles == int((out["wall_count"] > 0).sum()), where
        ref_rows, ref_order = strip_sort(out["fixed_positions"], d)
        assert np.array_equal(sorted_ids, ids[ref_order]) and np.array_equal(slot_ids, sorted_ids), where
        assert np.array_equal(rows, ref_rows), where
        assert np.array_equal(fixed, out["fixed_positions"][ref_order]), where
        assert np.array_equal(counts, out["neighbor_counts"][ref_order]), where
        table = out["neighbor_table"][ref_order]
        assert np.array_equal(nbrs, np.where(table >= 0, ids[np.maximum(table, 0)], -1)), where
        gp, gv, gpr, gids = got["plain"]
        assert np.array_equal(gids, ids[keep]), where
        for what, have, want in (("positions", gp, out["particles"][keep]), ("velocities", gv, out["velocities"][keep]),
                                 ("pressure", gpr, out["pressure"][keep]), ("every pressure", got["pressure"], out["pressure"]),
                                 ("normals", got["normals"], out["surface_normals"])):
            assert np.array_equal(np.isnan(have), np.isnan(want)), f"{where}: {what}"
            atol = fc.ATOL["velocities"] if what == "velocities" else 1e-12
            np.testing.assert_allclose(have, want, rtol=fc.RTOL, atol=atol, err_msg=f"{where}: {what}")
        assert np.isfinite(got["pressure"]).all(), where
        # ---- the other contexts against the plain one, bit for bit
        if fused:
            assert taps["fused"][0] == taps["plain"][0], where
            for a, b in zip(taps["fused"][1:], taps["plain"][1:]):
                assert np.array_equal(a, b), where
            first = 1 if t + 1 < ticks else 0   # (the last tick promised nothing: the positions are comparable too)
            for a, b in zip(got["fused"][first:], got["plain"][first:]):
                assert np.array_equal(a, b), where
        if monitor:
            for a, b in zip(got["monitor"], got["plain"]):
                assert np.array_equal(a, b), where
            sums, count = engines["monitor"].force_monitor()
            assert count == len(p), where
            for phase, total, want in zip(PHASES, sums, phase_means(out, v, coef).values()):
                assert total / count == pytest.approx(want, rel=1e-7, abs=1e-13), f"{where}: {phase}"
        dropped_before = bool(nan.any())
        state = (gp, gv, gids)
    for eng in engines.values():
        eng.synchronize()                       # nothing is left to report
        eng.close()


@pytest.mark.parametrize("name,noise", fc.paths())
def test_two_ticks_match_the_oracle_single_and_fused(sc, name, noise):
    drive(sc, name, noise)


@pytest.mark.parametrize("name,noise", [("list_lengths_lds", "counter"), ("clipped_noise_4", "counter"), ("floor_pile", "none")])
def test_the_monitor_instantiation_changes_nothing_and_matches_the_phases(sc, name, noise):
    drive(sc, name, noise, fused=False, monitor=True)
