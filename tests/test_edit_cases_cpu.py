"""The premises of tests/edit_cases.py, proved on the oracle alone: which radius steps move the grid beyond its
allocation, inside it, and to fewer cells; that every tick of every case is well-conditioned and has lists the kernels
take whole; that the GPU tests are sharp -- one tick without one of its edits ends at least 1,000 tolerances from the
right result, for every edit --; and what NumPy's generator does where the device has to follow it: binomial(n, 0.6),
which the device refuses, and binomial(0, p), which it draws."""
import numpy as np
import pytest

import edit_cases as E
import force_cases as fc
import growth_cases as G
import wall_cases as wc

ORACLE_NOISES = ("none", "counter", "host-sync")      # ("host" is the stream of "host-sync", drawn elsewhere)


@pytest.fixture(scope="module")
def runs():
    """Every case on the oracle under every noise, once: {(case, noise): [record per tick]}."""
    out = {}
    for name, build in E.CASES.items():
        case = build()
        for noise in ORACLE_NOISES:
            out[name, noise] = list(E.run(case, noise, stale=noise == "counter", ulp=True))
    return out


def same_stream(a, b):
    return a[2] == b[2] and np.array_equal(a[1], b[1])


def doubles_between(before, after, most=64):
    """How many doubles np.random draws from the state `before` to stand at `after`."""
    rs = np.random.RandomState()
    rs.set_state(before)
    for k in range(most + 1):
        if same_stream(rs.get_state(), after):
            return k
        rs.random_sample()
    raise AssertionError(f"more than {most} doubles")


def test_the_tolerances_are_the_suites():
    assert (fc.RTOL, fc.ATOL["particles"], fc.ATOL["velocities"]) == (1e-9, 1e-12, 1e-11) and G.SHARP == 1000.0


# ------------------------------------------------------------------ the grid
def test_radius_steps_reallocate_change_inside_and_shrink():
    case = E.radius_steps()
    stage = G.Stage(case.bodies, case.coef)
    radii = []
    for t in range(case.ticks):
        case.apply(stage, t)
        radii.append(stage.coef["particle_radius"])
    assert radii == [wc.R * f for f in E.RADIUS_STEPS] and radii[-1] == radii[0] == wc.R
    plan = E.grid_plan(radii)
    cells = [c for c, _, _ in plan]
    assert cells == [11881, 11881, 20164, 20164, 13456, 7396, 7396, 11881, 11881]
    assert [w for _, w, _ in plan] == [6, 6, 10, 10, 7, 4, 4, 6, 6]
    assert len({w for _, w, _ in plan}) >= 3
    # the context's first tick allocates; the step to 0.75 R passes 11,881 + 1 + 11,881 / 4; nothing else does
    assert [g for _, _, g in plan] == [True, False, True, False, False, False, False, False, False]
    assert 20164 + 1 > 11881 + 1 + 11881 // 4
    room = 20164 + 1 + 20164 // 4
    changed = [t for t in range(1, case.ticks) if cells[t] != cells[t - 1]]
    assert changed == sorted(case.edits) == [2, 4, 5, 7]
    inside = [t for t in changed if not plan[t][2]]
    assert inside == [4, 5, 7] and all(cells[t] + 1 <= room for t in inside)
    assert cells[7] > cells[6] and cells[4] < cells[3] and cells[5] < cells[4]   # more cells inside the allocation, and fewer
    # the promises across an edit name these steps
    kinds = {kind: (name, t) for name, t, kind in E.PROMISE_EDITS}
    assert kinds["radius smaller, past the allocation"] == ("radius_steps", 1) and plan[2][2] and radii[2] < radii[1]
    assert kinds["radius smaller, inside the allocation"] == ("radius_steps", 6) and not plan[7][2] and radii[7] < radii[6]
    assert kinds["radius larger"] == ("radius_steps", 4) and radii[5] > radii[4]


def test_promise_edits_differ_in_the_way_they_say():
    for name, t, kind in E.PROMISE_EDITS:
        case = E.CASES[name]()
        assert not case.sources_active(t + 1) or name == "every_coefficient"   # (nothing may be emitted behind a promise)
        stage = G.Stage(case.bodies, case.coef, case.sources)
        for k in range(t + 1):
            case.apply(stage, k)
        now = (dict(stage.coef, gravity=stage.coef["gravity"].copy()), stage.segments.copy())
        case.apply(stage, t + 1)
        nxt = (stage.coef, stage.segments)
        differs = [k for k in now[0] if not np.array_equal(now[0][k], nxt[0][k])]
        walls_moved = now[1].shape != nxt[1].shape or not np.array_equal(now[1], nxt[1])
        if kind.startswith("radius"):
            assert differs == ["particle_radius"] and not walls_moved
        elif kind == "another coefficient":
            assert len(differs) == 1 and differs != ["particle_radius"] and not walls_moved
        elif kind == "a moved wall":
            assert not differs and now[1].shape == nxt[1].shape and walls_moved
        else:
            assert kind == "another segment count" and not differs and len(now[1]) != len(nxt[1])
    assert {kind for _, _, kind in E.PROMISE_EDITS} == {
        "radius smaller, past the allocation", "radius smaller, inside the allocation", "radius larger",
        "another coefficient", "a moved wall", "another segment count"}
    case = E.every_coefficient()
    assert not case.sources_active(2) and case.sources_active(1)      # the source rests from tick 2 on: `run` may take over


# ------------------------------------------------------------------ every tick of every case
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_every_tick_is_well_conditioned(runs, name):
    for noise in ORACLE_NOISES:
        for rec in runs[name, noise]:
            worst, same = rec["sensitivity"]
            assert same and worst < 1.0, (name, noise, rec["tick"], worst)


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_lists_fit_and_no_row_is_nan(runs, name):
    case = E.CASES[name]()
    for noise in ORACLE_NOISES:
        assert len(runs[name, noise]) == case.ticks
        for rec in runs[name, noise]:
            out, where = rec["out"], (name, noise, rec["tick"])
            lengths = E.list_lengths(out, 2 * rec["coef"]["particle_radius"])
            assert lengths.max(initial=0) <= E.MAX_NEIGHBORS, where
            assert np.array_equal(out["neighbor_counts"], lengths), where       # nothing was cut
            if case.forces_on:
                assert lengths.mean() >= 2.0, where
            for key in ("particles", "velocities", "pressure"):
                assert np.isfinite(out[key]).all(), where
    assert len(runs[name, "counter"][-1]["ids"]) > 200


def test_the_worlds_are_the_sizes_they_say(runs):
    assert len(E.radius_steps().p) == len(E.every_coefficient().p) == 2700
    assert 200 < len(E.walls_edited().p) < 500
    for noise in ORACLE_NOISES:
        walls = [int((rec["out"]["wall_count"] > 0).sum()) for rec in runs["radius_steps", noise]]
        assert walls[4] > walls[3] and walls[5] > walls[4] and min(walls[4], walls[5]) > 10   # after each growth of the radius
        assert all((rec["out"]["wall_count"] > 0).sum() > 30 for rec in runs["walls_edited", noise])
    segments = [rec["n_segments"] for rec in runs["walls_edited", "counter"]]
    assert segments == [4, 4, 4, 5, 16, 16, 16, 16, 5, 5] and segments[E.WALLS_FULL_AT] == E.MAX_SEGMENTS == 16


# ------------------------------------------------------------------ sharp
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_every_edit_is_sharp(runs, name):
    """The tick without one of its edits -- what a crate that remembered the earlier inputs would compute -- is at
    least SHARP tolerances away, for every edit of every case."""
    case = E.CASES[name]()
    seen = 0
    for rec in runs[name, "counter"]:
        assert [n for n, _ in rec["stale"]] == [e.name for e in case.edits_at(rec["tick"])]
        for edit, far in rec["stale"]:
            seen += 1
            assert far >= G.SHARP, (name, rec["tick"], edit, far)
    assert seen == sum(len(e) for e in case.edits.values()) > 0


def test_every_coefficient_edits_each_thing_once():
    case = E.every_coefficient()
    names = [e.name for t in sorted(case.edits) for e in case.edits[t]]
    assert names == ["max_particles", "dt", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
                     "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure", "gravity", "gravity[1]"]
    assert all(len(e) == 1 for e in case.edits.values())
    # the gravity is written into the array that is there
    stage = G.Stage(case.bodies, case.coef)
    case.apply(stage, 10)
    array = stage.coef["gravity"]
    case.apply(stage, 11)
    assert stage.coef["gravity"] is array and array.tolist() == [1.5, -4.0]


def test_max_particles_is_raised_after_it_clipped(runs):
    first, second = runs["every_coefficient", "counter"][:2]
    (drawn, count), = first["emitted"]
    assert 0 < count < drawn and count == 40                   # tick 0: clipped by the room
    (drawn, count), = second["emitted"]
    assert drawn == count > 0                                   # tick 1: the room was raised
    assert all(rec["emitted"] == [] for rec in runs["every_coefficient", "counter"][2:])


def test_wall_edits_keep_or_replace_the_array_as_they_say():
    case = E.walls_edited()
    stage = G.Stage(case.bodies, case.coef)
    box = stage.bodies[0]
    array = box.segments
    case.apply(stage, 1)
    assert box.segments is array and array[0, 1].tolist() == [1.0, 0.0035]
    case.apply(stage, 2)
    assert box.segments is not array and box.segments.shape == array.shape


# ------------------------------------------------------------------ the sources
def test_flow_zero_and_back(runs):
    for noise in ORACLE_NOISES:
        run = runs["sources_edited", noise]
        for rec in run[:10]:                                      # (the three sources of the start, all active)
            third = rec["emitted"][2]
            assert (third == (0, 0)) == (rec["tick"] in E.FLOW_ZERO_TICKS), (noise, rec["tick"])
        assert [len(rec["emitted"]) for rec in run] == [3] * 10 + [2, 3, 3]      # active_ticks, and the source appended


def test_binomial_of_flow_zero_draws_one_double():
    """NumPy's legacy binomial(0, p) returns 0 and advances the stream by exactly one double: what the device's
    inversion loop does with qn = exp(0) = 1 and bound 0 (sc_emit_particles, k_rng_emit)."""
    for seed, p in ((0, 0.002), (1, 0.002024), (2, 0.3), (3, 0.5)):
        np.random.seed(seed)
        before = np.random.get_state()
        assert np.random.binomial(0, p) == 0
        assert doubles_between(before, np.random.get_state()) == 1


def test_binomial_above_one_half_and_what_it_draws(runs):
    """dt = 0.6: the oracle's emission draws binomial(flow, 0.6) from np.random -- the draw the device refuses."""
    case = E.dt_above_half()
    assert case.warns_at == (3,) and sorted(case.edits) == [3, 5] and not case.forces_on
    assert fc.OFF.items() <= {k: v for k, v in case.coef.items()}.items()
    run = runs["dt_above_half", "host-sync"]
    assert [rec["coef"]["dt"] for rec in run] == [0.002] * 3 + [0.6] * 2 + [0.002] * 2
    np.random.seed(0)
    stage = G.Stage(case.bodies, case.coef, case.sources)
    state = E.start_of(case)
    for t in range(3):
        _, state, _, _ = E.oracle_tick(stage, t, state, "host-sync")
    before = np.random.get_state()
    drawn = np.random.binomial(E.DT_HALF_FLOW, 0.6)
    assert doubles_between(before, np.random.get_state()) == E.DT_HALF_DRAWS
    assert run[3]["emitted"] == [(drawn, drawn)] and 0.55 * E.DT_HALF_FLOW < drawn < 0.65 * E.DT_HALF_FLOW
