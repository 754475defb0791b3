"""The premises of tests/rng_block_cases.py, proved without a device: the model of the block loop is NumPy's generator
from every position, the oracle's restatement holds at odd positions too, every named case meets the border it is named
for and tells a wrong generator from the right one, the worlds consume the rows they claim, the id tables have the bound
they claim, and the emission cases take both binomial branches, refill inside a double and leave position 624 to the
next launch."""
import numpy as np
import pytest

import rng_block_cases as K
from oracle.neighbors import neighbor_lists
from oracle.rng import MT19937, binomial
from rng_cases import takes_btpe

CASES = {c.name: c for c in K.NOISE_CASES}
ROW_COUNTS = sorted({c.rows for c in K.NOISE_CASES} | {2 * K.ID_BOUND_PAIRS})


def same_walk(got: K.Walk, want) -> bool:
    doubles, key, pos = want
    return np.array_equal(got.doubles, doubles) and np.array_equal(got.key, key) and got.pos == pos


# ------------------------------------------------------------------ the model is NumPy's generator
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_block_walk_equals_numpy_from_every_position(rows):
    for pos in range(K.N + 1):
        assert same_walk(K.block_walk(pos, rows), K.numpy_walk(pos, rows)), pos


def test_block_walk_equals_numpy_with_other_keys_and_row_counts():
    for seed, pos, rows in ((0, 624, 1), (1, 623, 1), (2, 311, 79), (3, 1, 77), (4, 622, 78), (5, 17, 240), (6, 623, 313)):
        key = K.key_of(seed)
        assert same_walk(K.block_walk(pos, rows, key), K.numpy_walk(pos, rows, key)), (seed, pos, rows)


def test_oracle_stream_agrees_at_odd_positions():
    """oracle/rng.py draws word by word, so an odd position needs nothing special -- which is why it is the reference
    for `RngSerial`; here it is held against NumPy where tests/test_oracle_rng.py does not go: doubles from every odd
    position, a block and a half from the borders, and both binomial branches from the odd emission starts."""
    for pos in range(1, K.N, 2):
        mine = MT19937(K.KEY, pos)
        doubles, key, at = K.numpy_walk(pos, 2)
        assert np.array_equal(mine.rand(2, 2), doubles) and mine.pos == at and np.array_equal(mine.mt, key), pos
    for pos in (1, 311, 621, 623):
        mine = MT19937(K.KEY, pos)
        doubles, key, at = K.numpy_walk(pos, 240)
        assert np.array_equal(mine.rand(240, 2), doubles) and mine.pos == at and np.array_equal(mine.mt, key), pos
    for flow in (1, 500, 20000):
        for pos in (1, 621, 623):
            mine, rs = MT19937(K.KEY, pos), K.numpy_state(pos)
            for _ in range(40):
                assert binomial(mine, flow, K.EMIT_DT) == rs.binomial(flow, K.EMIT_DT)
            assert mine.pos == rs.get_state()[2] and mine.pos % 2 == 1
            assert np.array_equal(mine.mt, rs.get_state()[1])


# ------------------------------------------------------------------ the named cases meet what they are named for
def walk_of(case: K.NoiseCase, fault=None) -> K.Walk:
    return K.block_walk(case.start, case.rows, fault=fault)


def test_the_case_list_is_the_one_the_borders_ask_for():
    listed = {(c.family, c.start, c.rows) for c in K.NOISE_CASES}
    assert {("quiet", s, 0) for s in (0, 1, 623, 624)} <= listed
    assert {("ends", *c) for c in ((8, 154), (616, 2), (0, 156), (7, 154), (615, 2), (623, 156))} <= listed
    assert {("begins", s, rows) for s in (624, 623, 622, 621) for rows in (2, 156)} <= listed
    assert {("blocks", s, 480) for s in (1, 312, 623)} <= listed
    assert any(c.family == "second_tick" and c.start == 1 and c.ticks == 2 for c in K.NOISE_CASES)
    assert len(CASES) == len(K.NOISE_CASES)
    for c in K.NOISE_CASES:  # a few hundred particles at most
        assert len(K.world_of(c).p) <= 500 and K.world_of(c).rows == c.rows


def test_quiet_cases_draw_nothing():
    for c in K.NOISE_CASES:
        if c.family != "quiet":
            continue
        w = walk_of(c)
        assert w.trace == () and w.pos == c.start and np.array_equal(w.key, K.KEY) and w.doubles.shape == (0, 2)
        assert len(K.world_of(c).p) > 0


def test_ends_cases_stop_on_the_border():
    ends = {c.start: walk_of(c) for c in K.NOISE_CASES if c.family == "ends"}
    for s in (8, 616, 0):   # the last word drawn is word 623: the position is 624, and nothing is regenerated for it
        assert ends[s].pos == K.N and ends[s].regenerations == 0 and ends[s].carry_taken == 0 and ends[s].trace[-1].startswith("draw")
        assert np.array_equal(ends[s].key, K.KEY)
    for s in (7, 615):      # one word is left and no double wants it: no carry
        assert ends[s].pos == K.N - 1 and ends[s].regenerations == 0 and ends[s].carry_taken == 0
    w = ends[623]           # a whole block from 623: carry, regenerate, 311 doubles, and again one word left over
    assert w.trace == ("draw 0", "carry_taken", "regenerate", "carry_used", "draw 311") and w.pos == K.N - 1


def test_begins_cases_start_on_the_border():
    begins = {(c.start, c.rows): walk_of(c) for c in K.NOISE_CASES if c.family == "begins"}
    for rows, rest in ((2, 4), (156, 312)):
        assert begins[624, rows].trace[:2] == ("regenerate", f"draw {rest}")
        assert begins[623, rows].trace[:4] == ("draw 0", "carry_taken", "regenerate", "carry_used")
        assert begins[623, rows].empty_stretch == 1
        assert begins[622, rows].trace[:3] == ("draw 1", "regenerate", f"draw {rest - 1}")
        assert begins[622, rows].carry_taken == 0
        assert begins[621, rows].trace[:4] == ("draw 1", "carry_taken", "regenerate", "carry_used")
        assert begins[621, rows].empty_stretch == 0
    for (s, rows), w in begins.items():
        assert w.regenerations == 1 and w.pos == (s + 4 * rows - 1) % K.N + 1, (s, rows)  # (an end position is 1..624)
        assert w.carry_taken == w.carry_used == s % 2


def test_blocks_cases_regenerate_three_times_and_more():
    for c in K.NOISE_CASES:
        if c.family != "blocks":
            continue
        w = walk_of(c)
        # 1920 words are three blocks and 48 words: three regenerations -- and a fourth from 623, whose first double
        # already straddles
        assert 4 * c.rows == 1920 and w.regenerations == (4 if c.start == 623 else 3)
        assert w.carry_taken == w.carry_used == (w.regenerations if c.start % 2 else 0)
        assert w.empty_stretch == (c.start == 623)
        assert w.pos == c.start + 1920 - w.regenerations * K.N


def test_second_tick_begins_where_the_first_ended():
    """Two ticks of the pair world on the oracle from position 1: the second tick starts at 17, odd, in the block the
    first one regenerated, and has pairs to draw for -- a carry in each tick."""
    c = CASES["second_tick_s1_P160"]
    world = K.world_of(c)
    stage = K.oracle_stage()
    rs = K.numpy_state(c.start)
    p, v = world.p, world.v
    starts, rows = [], []
    for _ in range(c.ticks):
        starts.append(rs.get_state()[2])
        out = K.oracle_tick(stage, p, v, lambda total: (rows.append(total), rs.rand(total, 2))[1])
        p, v = out["particles"], out["velocities"]
    assert starts == [1, 17] and rows[0] == c.rows and rows[1] > 0
    for s, r in zip(starts, rows):
        w = K.block_walk(s, r)
        assert w.carry_taken == w.carry_used == 1 and w.regenerations == 1


def test_oracle_tick_checks_the_block_length():
    world = K.pair_world(1)
    with pytest.raises(AssertionError):
        K.oracle_tick(K.oracle_stage(), world.p, world.v, np.zeros((3, 2)))


# ------------------------------------------------------------------ ... and tell a wrong generator from a right one
def differs(case: K.NoiseCase, fault: str) -> bool:
    right, wrong = walk_of(case), walk_of(case, fault)
    return not (np.array_equal(right.doubles, wrong.doubles) and np.array_equal(right.key, wrong.key) and right.pos == wrong.pos)


@pytest.mark.parametrize("fault,event", [("drop_carry", "carry_taken"), ("swap_straddle", "carry_used"),
                                         ("stale_phase2", "regenerations")])
def test_cases_tell_a_wrong_generator(fault, event):
    """Every case that meets the event is changed by the fault -- doubles, key or position --, every case that does not
    is left alone (the fault is the one it says it is), and the cases named for the branch are among the former."""
    caught = {c.name for c in K.NOISE_CASES if differs(c, fault)}
    meets = {c.name for c in K.NOISE_CASES if getattr(walk_of(c), event) > 0}
    assert caught == meets
    named = {"drop_carry": ("begins_s623_P2", "begins_s623_P156", "begins_s621_P2", "begins_s621_P156",
                            "ends_at_623_s623_P156", "blocks_s1_P480", "blocks_s623_P480", "second_tick_s1_P160"),
             "swap_straddle": ("begins_s623_P2", "begins_s623_P156", "begins_s621_P2", "begins_s621_P156",
                               "ends_at_623_s623_P156", "blocks_s1_P480", "blocks_s623_P480", "second_tick_s1_P160"),
             "stale_phase2": tuple(c.name for c in K.NOISE_CASES if c.family in ("begins", "blocks", "second_tick"))}[fault]
    assert set(named) <= caught
    # the doubles themselves change, not only the state left behind: the tick's result shows it.  (A stale third phase
    # spoils words 454..623 of the new block: a case that stops before them shows it in the key it leaves alone.)
    for name in named:
        c = CASES[name]
        if fault == "stale_phase2" and not (c.family == "blocks" or (c.family == "begins" and c.rows == 156)):
            assert not np.array_equal(walk_of(c).key, walk_of(c, fault).key), name
            continue
        assert not np.array_equal(walk_of(c).doubles, walk_of(c, fault).doubles), name


def test_a_dropped_carry_in_a_case_of_two_rows_shifts_the_position():
    right, wrong = walk_of(CASES["begins_s623_P2"]), walk_of(CASES["begins_s623_P2"], "drop_carry")
    assert (right.pos, wrong.pos) == (7, 8)


# ------------------------------------------------------------------ the worlds
def worlds():
    out = {K.world_of(c).name: K.world_of(c) for c in K.NOISE_CASES}
    out.update({K.id_bound_world(b).name: K.id_bound_world(b) for b in K.ID_BOUNDS})
    return out


@pytest.mark.parametrize("name", sorted(worlds()))
def test_pair_worlds_consume_two_rows_a_pair(name):
    """P = sum C_i = 2k by oracle/neighbors.py -- on the positions as uploaded and, through the oracle's tick, on the
    positions the wall fix leaves (no particle touches a wall, the motored one included): every pair member lists its
    partner and nothing else, every lone particle nothing."""
    world = worlds()[name]
    counts, table = neighbor_lists(world.p, K.D)
    assert int(counts.sum()) == world.rows == 2 * world.pairs
    assert sorted(np.bincount(counts, minlength=2)) == sorted([len(world.p) - world.rows, world.rows])
    members = np.flatnonzero(counts == 1)
    assert np.array_equal(table[table[members, 0], 0], members)          # partners list each other
    assert np.all(np.abs(table[members, 0] - members) >= 1) and len(world.p) <= 500
    out = K.oracle_tick(K.oracle_stage(), world.p, world.v, np.full((world.rows, 2), 0.5))
    assert not out["wall_count"].any() and np.array_equal(out["neighbor_counts"], counts)
    assert np.array_equal(out["fixed_positions"], world.p)
    assert world.p.min() > 0.05 and world.p.max() < 0.95
    assert np.array_equal(np.sort(world.order), np.arange(len(world.p))) and np.all(np.diff(world.ids) > 0)


def test_pairs_are_isolated_by_the_lattice():
    world = K.pair_world(240)
    d2 = ((world.p[:, None, :] - world.p[None, :, :]) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    nearest = np.sqrt(np.sort(d2, axis=1)[:, :2])
    members = nearest[:, 0] < K.D
    assert members.sum() == 480 and np.allclose(nearest[members, 0], K.TOUCH * K.D)
    assert nearest[members, 1].min() > 2.5 * K.D and nearest[~members, 0].min() > 2.5 * K.D


# ------------------------------------------------------------------ the id bounds
def test_id_bound_cases_have_the_bound_they_claim():
    assert K.ID_BOUNDS == (2, 255, 256, 257, 511, 513, 65535, 65536)
    assert [K.scan_run(b) for b in K.ID_BOUNDS] == [1, 1, 1, 2, 2, 3, 256, 256]
    for bound in K.ID_BOUNDS:
        w = K.id_bound_world(bound)
        assert K.host_id_bound(w.ids) == bound <= K.SMALL_IDS
        assert w.ids[-1] == bound - 1 and w.ids[0] == 0 and len(np.unique(w.ids)) == len(w.ids)
        assert not np.array_equal(w.stored()[2], np.sort(w.stored()[2]))  # id order is not slot order
        if bound > 2:
            per = K.scan_run(bound)
            assert {per - 1, per} <= set(w.ids.tolist())                   # both sides of the first thread's run
            assert len(w.ids) < bound / 5                                  # sparse: most ids count zero
            assert w.rows == 2 * K.ID_BOUND_PAIRS
        walk = K.block_walk(K.ID_BOUND_START, w.rows)
        assert walk.carry_used == 1 and walk.regenerations == 1
    assert K.ID_BOUND_ORACLE in K.ID_BOUNDS


def test_scanned_variants_only_move_the_top_id():
    for w in [K.id_bound_world(b) for b in K.ID_BOUNDS] + [K.world_of(c) for c in K.NOISE_CASES]:
        up = w.with_top_id(K.SMALL_IDS)
        assert K.host_id_bound(up.ids) == K.SMALL_IDS + 1 > K.SMALL_IDS >= K.host_id_bound(w.ids)
        assert np.array_equal(up.ids[:-1], w.ids[:-1]) and np.all(np.diff(up.ids) > 0)
        assert up.p is w.p and up.v is w.v and up.order is w.order


# ------------------------------------------------------------------ emission
TRACES = {case: K.emission_trace(*case) for case in K.EMIT_CASES}


def test_emission_cases_are_the_ones_listed():
    assert K.EMIT_STARTS == (0, 1, 2, 620, 621, 622, 623, 624) and K.EMIT_CALLS == 3
    for name in ("flow_1", "inversion_500", "btpe_20000", "mixed_9"):
        assert {(name, s) for s in K.EMIT_STARTS} <= set(K.EMIT_CASES)
    assert [s.flow for s in K.EMIT_LISTS["flow_1"]] == [1] and [s.flow for s in K.EMIT_LISTS["inversion_500"]] == [500]
    assert [s.flow for s in K.EMIT_LISTS["btpe_20000"]] == [20000] and len(K.EMIT_LISTS["mixed_9"]) == 9
    for case, trace in TRACES.items():
        launches = -(-len(K.EMIT_LISTS[case[0]]) // K.LAUNCH_SOURCES)
        assert len(trace) == K.EMIT_CALLS * launches
        assert sum(t["emitted"] for t in trace) <= 2 * K.EMIT_ROOM
        assert all(a["end"] == b["start"] for a, b in zip(trace, trace[1:]))  # every launch continues the stream


def test_emission_takes_both_binomial_branches():
    branches = {name: {takes_btpe(s.flow, K.EMIT_DT) for s in srcs} for name, srcs in K.EMIT_LISTS.items()}
    assert branches["flow_1"] == branches["inversion_500"] == {False} and branches["btpe_20000"] == {True}
    assert branches["mixed_9"] == branches["eight_quiet_then_btpe"] == {False, True}
    assert any(t["emitted"] > 20 for t in TRACES["btpe_20000", 0]) and any(t["emitted"] > 0 for s in K.EMIT_STARTS for t in TRACES["inversion_500", s])


def test_emission_refills_inside_a_double():
    """From an odd position every double sits on an odd word, so a launch that regenerates the block does it between a
    double's two words.  From 623 the very first double is the one -- the binomial's, of both branches."""
    inside = [(case, t) for case, trace in TRACES.items() for t in trace if t["refilled"] and t["start"] % 2 == 1]
    assert len(inside) >= 8
    for name in ("flow_1", "inversion_500", "btpe_20000", "mixed_9"):
        first = TRACES[name, 623][0]
        assert first["start"] == 623 and first["refilled"]
    # ... and launches that follow one that refilled, and ones that follow one that did not (the key's write-back)
    for name in ("flow_1", "inversion_500"):
        assert [t["refilled"] for t in TRACES[name, 623]] == [True, False, False]
        assert [t["refilled"] for t in TRACES[name, 0]] == [False, False, False]
    assert [t["refilled"] for t in TRACES["btpe_20000", 0]] == [False, True, False]


def test_emission_leaves_624_to_the_next_launch():
    """A launch that ends on the block's last word writes position 624 back and the next one regenerates before it
    draws: the next call (flow 1 draws one double a call), and the second launch of one call of nine sources."""
    handed = [(case, t) for case, trace in TRACES.items() for t in trace[1:] if t["start"] == K.N]
    assert any(case == ("flow_1", 622) and t["call"] == 1 for case, t in handed)
    assert any(case == ("flow_1", 620) and t["call"] == 2 for case, t in handed)
    second = TRACES["eight_quiet_then_btpe", 608][1]
    assert second["launch"] == 1 and second["call"] == 0 and second["start"] == K.N and second["refilled"]
    assert second["flows"] == [20000] and second["emitted"] > 0
    straddle = TRACES["eight_quiet_then_btpe", 607][1]                  # ... and one that starts inside the straddling double
    assert straddle["launch"] == 1 and straddle["start"] == K.N - 1 and straddle["refilled"]
    for name in ("flow_1", "inversion_500", "btpe_20000", "mixed_9"):   # a call that begins at 624
        assert TRACES[name, 624][0]["start"] == K.N and TRACES[name, 624][0]["refilled"]
