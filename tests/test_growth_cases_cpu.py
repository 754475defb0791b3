"""The premises of tests/growth_cases.py, proved on the oracle: where each capacity is passed, that the ids have gaps
when it is, that the exact-fit worlds fill to the last slot and emit nothing afterwards -- and that the GPU tests are
sharp: one tick with the key of a context that lost its tick, or with the ids of a context that renumbered its
particles, differs from the right tick by at least 1,000 times the suite's tolerances, at every tick after a growth."""
import numpy as np
import pytest

import force_cases as fc
import growth_cases as G


@pytest.fixture(scope="module")
def two_growths():
    case = G.sources_two_growths()
    return case, list(G.run(case, G.FIRST_CAPACITY))


def test_the_tolerances_are_the_suites():
    assert (fc.RTOL, fc.ATOL["particles"], fc.ATOL["velocities"]) == (1e-9, 1e-12, 1e-11) and G.SHARP == 1000.0


def test_two_growths_pass_each_capacity_where_the_case_says(two_growths):
    case, run = two_growths
    growths = [(rec["tick"], cap) for rec in run for cap, _, _ in rec["grew"]]
    assert tuple(growths) == case.growths[G.FIRST_CAPACITY] == G.TWO_GROWTHS
    (t1, c1), (t2, c2) = growths
    assert t1 < 4 and t2 < 16 and t2 + 3 < case.ticks            # within 4 and 16 ticks, and ticks behind the second
    assert case.coef["max_particles"] <= 3000
    # the capacities are the crate's: int(needed * 1.5) + 1024 of the count that did not fit
    room = G.FIRST_CAPACITY
    for rec in run:
        for cap, ids, needed in rec["grew"]:
            assert needed > room >= len(ids) and cap == G.grown(needed) == int(needed * 1.5) + 1024
            room = cap
    assert len(run[t1 - 1]["ids"]) <= G.FIRST_CAPACITY < len(run[t1]["ids"]) + 2
    assert len(run[t2 - 1]["ids"]) <= c1 < len(run[t2]["ids"]) + 8
    assert max(len(rec["ids"]) for rec in run) < c2 < case.ample  # no third growth; the ample run never grows
    assert [rec["grew"] for rec in G.run(case, case.ample)] == [[]] * case.ticks


def test_ids_have_gaps_at_each_growth(two_growths):
    _, run = two_growths
    seen = 0
    for rec in run:
        for _, ids, _ in rec["grew"]:
            seen += 1
            assert len(ids) and np.all(np.diff(ids) > 0)
            holes = np.setdiff1d(np.arange(ids.max() + 1), ids)
            assert len(holes) >= 1 and holes.min() < ids.max()    # a gap in the middle: renumbering moves ids
            assert not np.array_equal(ids, np.arange(len(ids)))
    assert seen == 2


def test_the_shooter_leaves_within_a_few_ticks(two_growths):
    case, run = two_growths
    removed = sum(rec["removed"] for rec in run)
    shot = sum(rec["emitted"][0][1] for rec in run)
    assert shot > 30 and shot - 12 <= removed <= shot             # all but the last two ticks' have left
    assert all(rec["removed"] <= run[k - 1]["emitted"][0][1] + run[k - 2]["emitted"][0][1] for k, rec in enumerate(run) if k >= 2)


def test_two_growths_are_sharp_at_every_tick_after_a_growth(two_growths):
    case, run = two_growths
    first = G.TWO_GROWTHS[0][0]
    checked = 0
    for rec in run:
        if rec["tick"] < first:
            assert rec["out_old_key"] is None
            continue
        checked += 1
        assert G.worst(rec["out"], rec["out_old_key"]) >= G.SHARP, rec["tick"]
        assert G.worst(rec["out"], rec["out_renumbered"]) >= G.SHARP, rec["tick"]
        assert G.worst(rec["out"], rec["out"]) == 0.0
    assert checked == case.ticks - first
    assert all((rec["out"]["neighbor_counts"] > 0).any() for rec in run)   # (noise needs a neighbor: every tick has some)


def test_no_particle_reaches_the_wall(two_growths):
    _, run = two_growths
    for rec in run:
        assert (rec["out"]["wall_count"] == 0).all() and (rec["out"]["ccd_factor"] == 1.0).all()
        assert np.isfinite(rec["out"]["particles"]).all() and np.isfinite(rec["out"]["velocities"]).all()


@pytest.mark.parametrize("count", G.EXACT_COUNTS)
def test_exact_fit_fills_to_the_last_slot(count):
    case = G.exact_fit(count)
    assert case.coef["max_particles"] == count and count in case.capacities
    runs = {cap: list(G.run(case, cap)) for cap in case.capacities}
    for cap, run in runs.items():
        growths = tuple((rec["tick"], c) for rec in run for c, _, _ in rec["grew"])
        assert growths == case.growths[cap]
        counts = [len(rec["ids"]) for rec in run]
        full = counts.index(count)                                # reached exactly ...
        assert 2 <= full < case.ticks - 2 and counts[full:] == [count] * (case.ticks - full)
        clipped = [(drawn, k) for drawn, k in run[full]["emitted"] if k < drawn]
        assert clipped and clipped[0][1] > 0                      # ... by an emission the room clipped
        for rec in run[full + 1:]:                                # later ones draw and emit nothing
            assert all(drawn > 0 and k == 0 for drawn, k in rec["emitted"])
        assert all(rec["removed"] == 0 for rec in run)
        assert all((rec["out"]["wall_count"] == 0).all() for rec in run)
    assert case.growths[G.FIRST_CAPACITY] == (G.EXACT_FIRST_GROWTH,) and case.growths[count] == ()
    first = runs[G.FIRST_CAPACITY]
    assert len(first[0]["grew"][0][1]) == 0                      # (that growth leaves an empty context)
    for a, b in zip(first, runs[case.ample]):                    # on the oracle the capacity changes nothing
        assert np.array_equal(a["out"]["particles"], b["out"]["particles"]) and np.array_equal(a["ids"], b["ids"])


def test_set_state_growth_is_sharp_after_the_replacement():
    case = G.set_state_growth()
    small, ample = case.capacities
    assert len(case.first[0]) == 50 <= small < len(case.second) == 2200 <= ample and case.ticks_before == 3
    ticks = list(G.run_set_state(case))
    assert [t for t, _, _ in ticks] == list(range(case.ticks_before + case.ticks_after))
    for t, out, old_key in ticks:
        if t < case.ticks_before:
            assert old_key is None and len(out["particles"]) == 50
        else:
            assert G.worst(out, old_key) >= G.SHARP, t
            assert len(out["particles"]) > small
