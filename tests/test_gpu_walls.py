"""The wall pass and the crossing test at the edges of their shortcuts (tests/wall_cases.py), against the oracle.

Every world is built so that one shortcut decides the result -- a particle just beyond far_box that moves just over 2d,
one that crosses a segment in the last cell of its block's near_now mask or far outside it, one that lands on a segment
its block's near_next mask does not hold, positions on the edges of floor(p * (1/d)) and of the sqrt rule, waves that
mix the lanes of the wave-wide ballots.  Each tick is checked against the oracle restarted from the device's previous
state (see test_gpu_parity.py: test_ticks_match_oracle): the sort, the wall-fixed positions and the count of particles
with wall contacts bit for bit, the rest to 1e-9.  `fused` also runs a second context whose ticks promise the next
tick's inputs, so that its pass B runs the next tick's wall pass (the path of Crate.run), and holds it to the first
context bit for bit, tick by tick.
Each test first asserts its world's premises on the oracle (tests/test_wall_cases_cpu.py)."""
import numpy as np
import pytest

import test_wall_cases_cpu as premises
import wall_cases as wc
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

COEF = ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
        "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure")
TICKS = 3
SEED = 11


def _bodies(states):
    return [(b.position, b.center_velocity, b.omega, b.n_segments) for b in states]


def drive(sc, case, noise, fused, ticks=TICKS):
    """`ticks` device ticks of `case`, each compared with the oracle's tick core on the device's previous state.
    fused: a second context runs the same ticks with every next tick's inputs promised, so that its pass B also runs
    the next tick's wall pass (the path of Crate.run); its sort, wall-fixed positions, contact count, velocities and
    pressures must equal the first context's bit for bit every tick, and its whole state after the last tick.  (Between
    promised ticks a context holds the positions after the NEXT tick's wall fix, so its positions are compared there.)"""
    from oracle.neighbors import strip_sort
    from oracle.tick import counter_noise_key, counter_noise_u01, remove_outside, tick_core
    from sand_crate_amd import _native as N
    orc = case.oracle()
    coef = dict(orc.coef)
    if noise == "none":
        coef["collider_noise_level"] = 0.0
    geo = []
    for _ in range(ticks):  # the bodies' motion does not depend on the particles
        for b in orc.rigid_bodies:
            b.advance(coef["dt"])
        geo.append((orc.segments.copy(), orc.body_states()))
    cf = {k: coef[k] for k in COEF}
    r, d = coef["particle_radius"], 2 * coef["particle_radius"]
    n = len(case.p)
    engines = []
    for _ in range(2 if fused else 1):
        eng = sc.Engine(n + 64)
        eng.set_noise_mode(N.NOISE_COUNTER if noise == "counter" else N.NOISE_NONE, SEED)
        eng.upload(case.p, case.v)
        engines.append(eng)
    p, v, ids = case.p, case.v, np.arange(n)
    for t in range(ticks):
        seg, st = geo[t]
        where = f"{case.name} tick {t}"
        taps = []
        for k, eng in enumerate(engines):
            eng.set_params(gravity=coef["gravity"], **cf)
            eng.set_segments(seg, sc.pad_segments(seg, r), _bodies(st))
            eng.step_begin()
            s = eng.step_stats()
            taps.append(((s.particles, s.wall_particles, s.neighbor_slots), *eng.download_sort(), *eng.download_neighbors()))
            if k == 1 and t + 1 < ticks:
                eng.set_next_inputs(gravity=coef["gravity"], segments=geo[t + 1][0], bodies=_bodies(geo[t + 1][1]), **cf)
            eng.step_finish()
        (particles, wall_particles, _), rows, sorted_ids, slot_ids, _, _, fixed = taps[0]
        gp, gv, gpr, gids = engines[0].download()
        if fused:
            assert taps[1][0] == taps[0][0], where
            for a, b in zip(taps[1][1:], taps[0][1:]):
                assert np.array_equal(a, b), where
            fp, fv, fpr, fids = engines[1].download()
            assert np.array_equal(fids, gids) and np.array_equal(fv, gv) and np.array_equal(fpr, gpr), where
        p, v, ids = remove_outside(p, v, r, ids)
        eta = None if noise == "none" else counter_noise_u01(ids, counter_noise_key(SEED, t))
        out = tick_core(p, v, seg, st, coef, eta_u01=eta)
        # decisions, bit for bit: who touches a wall, where the wall fix puts it, its row and its place in the order
        assert particles == len(p), where
        assert wall_particles == int((out["wall_count"] > 0).sum()), where
        assert np.array_equal(fixed, out["fixed_positions"][np.searchsorted(ids, slot_ids)]), where
        ref_rows, ref_order = strip_sort(out["fixed_positions"], d)
        assert np.array_equal(sorted_ids, ids[ref_order]), where
        assert np.array_equal(rows, ref_rows), where
        keep = ~np.isnan(out["particles"]).any(axis=1)
        assert np.array_equal(gids, ids[keep]), where
        np.testing.assert_allclose(gp, out["particles"][keep], rtol=1e-9, atol=1e-12, err_msg=where)
        np.testing.assert_allclose(gv, out["velocities"][keep], rtol=1e-9, atol=1e-10, err_msg=where)
        np.testing.assert_allclose(gpr, out["pressure"][keep], rtol=1e-9, atol=1e-12, err_msg=where)
        p, v, ids = gp, gv, gids
    if fused:  # the last tick promised nothing: the states are comparable whole
        for a, b in zip(engines[1].download(), engines[0].download()):
            assert np.array_equal(a, b), case.name
    for eng in engines:
        eng.close()


PATHS = [pytest.param(n, f, id=f"{n}-{'fused' if f else 'ticks'}") for n in ("none", "counter") for f in (False, True)]


@pytest.mark.parametrize("noise,fused", PATHS)
def test_far_box_and_ccd_skip(sc, noise, fused):
    """Particles beyond far_box moving just over 2d (the crossing test runs), just under (no crossing possible) and
    particles just inside far_box moving under 2d into the wall."""
    premises.test_far_box_case()
    drive(sc, wc.far_box_case(), noise, fused)


@pytest.mark.parametrize("noise,fused", PATHS)
def test_near_now_band_and_fallback(sc, noise, fused):
    """Crossings in the last cell of near_now and far outside it (the wave's fallback), in blocks of one strip, of four
    strips and in a pile whose tiles pass B cannot hold in LDS."""
    premises.test_near_now_case()
    drive(sc, wc.near_now_case(), noise, fused)


@pytest.mark.parametrize("noise", ["none", "counter"])
def test_near_next_and_strayed(sc, noise):
    """The fused wall pass: particles that land on a next-tick segment beyond near_next after moving more than 8 cells
    (strayed: the wave must look at every segment) and inside it after moving 5; the tick after is checked against the
    oracle, and the promised run against unpromised ticks bit for bit."""
    premises.test_near_next_case()
    drive(sc, wc.near_next_case(), noise, True)


@pytest.mark.parametrize("noise,fused", PATHS)
def test_floor_div_edges(sc, noise, fused):
    """Positions whose row or column floor(p * (1/d)) gets wrong: rows and order bit for bit, in the tick's own wall pass
    and (fused) in the previous tick's epilogue."""
    premises.test_floor_case()
    drive(sc, wc.floor_case(), noise, fused)


@pytest.mark.parametrize("noise,fused", PATHS)
def test_sqrt_rule_threshold(sc, noise, fused):
    """Contacts decided by the last ulp of the sqrt rule at segment ends and interiors."""
    premises.test_threshold_case()
    drive(sc, wc.threshold_case(), noise, fused)


@pytest.mark.parametrize("noise,fused", PATHS)
def test_junctions_and_ballots(sc, noise, fused):
    """16 segments of 8 bodies meeting at junctions (3 to 5 contacts, the slot-overwrite rule with motored bodies),
    waves mixing V = 1/2/4 lanes with V = 3/5 and single contacts with corners; forces on."""
    premises.test_junction_case()
    drive(sc, wc.junction_case(), noise, fused)
