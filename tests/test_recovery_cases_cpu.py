"""The premises of tests/recovery_cases.py, proved on the oracle, and the counter model under the rule before the
recovery was written and under the rule of `recover_flags`: what tests/test_gpu_recovery.py relies on, and why each of
its assertions would fail on a library that recovers the old way.  No device."""
import functools

import numpy as np
import pytest

import recovery_cases as rc
from oracle.neighbors import strip_sort
from oracle.tick import hard_wall_fix, tick_core, wall_contacts

TICKS = rc.GOOD_BEFORE + rc.GOOD_AFTER


@functools.lru_cache(maxsize=None)
def history(name):
    """The oracle's states of world `name`: before its first tick and after each of TICKS ticks (without noise: the
    premises hold with margins far beyond what the noise moves); `walls` gets its band after GOOD_BEFORE ticks, so
    state GOOD_BEFORE is what the abandoned ticks find in every world.  Computed once, never written to."""
    p, v = getattr(rc, name)()
    orc = rc.oracle(rc.PILE_COEF if name.startswith("pile") else rc.COEF)
    states = [(p, v)]
    for k in range(TICKS):
        with np.errstate(all="ignore"):  # (nan: the particle on the wall)
            out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef)
        keep = ~np.isnan(out["particles"]).any(axis=1)
        p, v = out["particles"][keep], out["velocities"][keep]
        if name == "walls" and k + 1 == rc.GOOD_BEFORE:
            p, v = np.concatenate((p, rc.band()[0])), np.concatenate((v, rc.band()[1]))
        states.append((p, v))
    for a, b in states:
        a.setflags(write=False)
        b.setflags(write=False)
    return states


def fixed(p, coef=rc.COEF):
    orc = rc.oracle(coef)
    V, u, _ = wall_contacts(p, orc.segments, orc.body_states(), coef["particle_radius"])
    return hard_wall_fix(p, V, u, coef["particle_radius"]), V


def test_the_grid_has_several_scan_workgroups():
    """One workgroup cannot give up on a predecessor: the worlds need at least three."""
    row0, n = rc.grid()
    assert (row0, n) == (-5, 93)
    assert n * n > 2 * rc.SCAN_PER_BLOCK and rc.scan_workgroups() == 5
    # the last workgroup's cells are rows floor(y / d) >= 83, y >= 0.996: beyond where the wall fix leaves a particle of the
    # box.  Its partial sum, the C_NT an abandoned tick leaves, is therefore 0 in every world: no slot keeps its pressure
    last = (n * n // rc.SCAN_PER_BLOCK) * rc.SCAN_PER_BLOCK
    assert last // n - 5 == 83 and 83 * rc.D > 1 - rc.R
    for name in ("quiet", "walls", "pile", "nan"):
        for p, _ in history(name)[:rc.GOOD_BEFORE + 1]:
            with np.errstate(all="ignore"):
                q = fixed(p)[0]
            q = q[~np.isnan(q).any(axis=1)]
            assert int(rc.cell_counts(q)[last:].sum()) == 0 < len(q), name


@pytest.mark.parametrize("name", ["quiet", "walls", "nan"])
def test_sparse_worlds_have_no_big_bucket(name):
    for p, _ in history(name):
        counts = rc.cell_counts(p)
        assert counts.max() <= 24 and counts.sum() == len(p)
    assert 5800 <= len(history(name)[0][0]) <= 6400


def test_dense_world_takes_the_large_noise_path():
    p, _ = rc.dense()
    counts = rc.cell_counts(p)
    assert len(p) > rc.SMALL_IDS and counts.max() <= rc.SORT_THRESHOLD and rc.wall_distance(p).min() > 1.2 * rc.R


def test_quiet_has_pressures_to_lose():
    """The last finished tick's pressures are the part of the state an abandoned tick's partial C_NT would cut."""
    orc = rc.oracle()
    for k in range(rc.GOOD_BEFORE):
        p, v = history("quiet")[k]
        pressure = tick_core(p, v, orc.segments, orc.body_states(), orc.coef)["pressure"]
        assert (pressure > 0).sum() > len(p) // 10


def test_quiet_stays_clear_of_the_walls():
    """Nothing within 1.2 r of a wall in any state the GPU test passes through: the wall fix is the identity."""
    for p, _ in history("quiet"):
        assert rc.wall_distance(p).min() > 2 * 1.2 * rc.R
        q, V = fixed(p)
        assert not V.any() and np.array_equal(q, p)


def test_walls_has_a_band_that_the_fix_moves():
    """The state the abandoned ticks find: the fix moves the 160 appended particles, each in contact with the floor alone,
    and nobody else; before the band arrives it moves nobody -- and never would: a tick leaves nobody inside r."""
    for k in range(rc.GOOD_BEFORE):
        p, _ = history("walls")[k]
        assert np.array_equal(fixed(p)[0], p)
    p, _ = history("walls")[rc.GOOD_BEFORE]
    n = len(rc.quiet()[0])
    assert len(p) == n + 160 and np.array_equal(p[n:], rc.band()[0])
    q, V = fixed(p)
    moved = (q != p).any(axis=1)
    assert np.array_equal(np.flatnonzero(moved), np.arange(n, n + 160)) and (V[moved] == 1).all()
    assert (rc.wall_distance(p[moved]) < 0.9 * rc.R).all() and (rc.wall_distance(q[moved]) >= rc.R * (1 - 1e-12)).all()
    for p, _ in history("walls")[rc.GOOD_BEFORE + 1:]:  # ... and the good ticks after it leave nobody inside r again
        assert len(p) == n + 160 and np.array_equal(fixed(p)[0], p)


def test_pile_buckets_on_both_sides_of_the_thresholds():
    sizes = {}
    for k in (0, rc.GOOD_BEFORE):  # as uploaded, and as the abandoned ticks find it
        p, _ = history("pile")[k]
        counts = rc.cell_counts(p)
        big = [int(counts[rc.cell_index(*c)]) for c in rc.PILE_CELLS]
        assert big == list(rc.PILE_SIZES)
        assert big[0] > rc.SORT_CHUNK and rc.SORT_THRESHOLD < big[1] <= rc.SORT_CHUNK  # two chunks; one
        others = np.delete(counts, [rc.cell_index(*c) for c in rc.PILE_CELLS])
        assert others.max() <= 1 < rc.SORT_THRESHOLD
        sizes[k] = counts
    assert len(rc.sort_tasks(sizes[0])) == 3
    p, _ = rc.pile()
    rows, order = strip_sort(p, rc.D)
    assert not np.array_equal(order, np.arange(len(p)))  # random storage order
    assert (np.diff(order) < 0).sum() > len(p) // 4
    # exact ties in x inside the big bucket: the id decides
    cell = rc.cells_of(p) == rc.cell_index(*rc.PILE_CELLS[0])
    assert len(np.unique(p[cell, 0])) <= cell.sum() - 64


def test_pile_after_shrinks_the_listed_buckets():
    """The tasks listed for `pile` -- chunk lengths 1024, 476 and 300 -- all run past the 200 and 120 particles that
    pile_after keeps in those cells; its own piles sit in other cells, on both sides of kSortChunk."""
    before = rc.cell_counts(rc.pile()[0])
    after = rc.cell_counts(rc.pile_after()[0])
    old = [rc.cell_index(*c) for c in rc.PILE_CELLS]
    new = [rc.cell_index(*c) for c in rc.PILE_AFTER_CELLS]
    assert [int(after[c]) for c in old] == list(rc.PILE_AFTER_SIZES)
    assert [int(after[c]) for c in new] == list(rc.PILE_AFTER_OWN)
    assert all(before[c] == 0 for c in new)
    assert after[new[0]] > rc.SORT_CHUNK and rc.SORT_THRESHOLD < after[new[1]] <= rc.SORT_CHUNK
    assert all(after[c] > rc.SORT_THRESHOLD for c in old)
    assert sorted(t[2] for t in rc.sort_tasks(before)) == [300, 476, 1024]
    for cell, chunk, length in rc.sort_tasks(before):
        assert chunk * rc.SORT_CHUNK + length > after[cell]
    for k in (0, 2):  # ... and stays so through its two ticks
        p, _ = history("pile_after")[k]
        assert np.array_equal(rc.cell_counts(p)[old + new], after[old + new])


def test_the_appended_particles_land_in_and_beside_the_pile():
    p, _ = rc.extra()
    cells = rc.cells_of(p)
    row, col = rc.PILE_CELLS[0]
    assert (cells == rc.cell_index(row, col)).sum() == 4 and (cells == rc.cell_index(row, col + 1)).sum() == 3


def test_nan_world_has_exactly_one_nan():
    p, v = rc.nan()
    assert np.array_equal(p[rc.NAN_AT], [0.0, 0.5]) and 0 < rc.NAN_AT < len(p) - 1
    with np.errstate(all="ignore"):
        q, V = fixed(p)
    bad = np.isnan(q).any(axis=1)
    assert bad.sum() == 1 and bad[rc.NAN_AT] and V[rc.NAN_AT] == 1
    assert np.array_equal(np.delete(q, rc.NAN_AT, axis=0), np.delete(p, rc.NAN_AT, axis=0))
    # the survivors are `quiet`, which stays clear of the walls: nothing else is ever dropped
    assert np.array_equal(np.delete(p, rc.NAN_AT, axis=0), rc.quiet()[0])


def test_capacity_bound():
    """(A + 2) n: the bucket starts of A abandoned ticks' counts and the next tick's on top end at (A + 1) n <= capacity,
    inside keys / keyCell, which are sized by the capacity."""
    for name in ("quiet", "walls", "pile", "nan"):
        n = len(history(name)[rc.GOOD_BEFORE][0])  # (walls: with its band)
        assert rc.capacity(n) >= (rc.ABANDONED + 2) * n > (rc.ABANDONED + 1) * n
    n = max(len(rc.pile()[0]), len(rc.pile_after()[0]) + len(rc.extra()[0]))
    assert rc.capacity(len(rc.pile()[0]), len(rc.pile_after()[0])) >= (rc.ABANDONED + 1) * n


# ---------------------------------------------------------------- the counter model
def run_model(rule, name, reader):
    """GOOD_BEFORE ticks, ABANDONED abandoned ones, the reader -- on the oracle's states of `name`."""
    states = history(name)
    m = rc.Counters(rule)
    m.upload(states[0][0])
    for k in range(rc.GOOD_BEFORE):
        top = m.tick(states[k][0])
        assert top == len(states[k][0]) == m.nt == m.ns
        assert not m.cell_count.any() and (m.nbig, m.ntasks) == (0, 0)
    found = fixed(states[rc.GOOD_BEFORE][0])[0]  # (K1 bins the position the wall fix leaves)
    m.append(len(found) - m.ns)  # walls: the band
    for _ in range(rc.ABANDONED):
        m.tick(found, abandon=True)
    return m, found


@pytest.mark.parametrize("reader", ["synchronize", "download"])
@pytest.mark.parametrize("name", ["quiet", "walls", "pile"])
def test_model_old_rule_is_wrong_on_these_worlds(name, reader):
    """What test_gpu_recovery.py would have seen before `recover_flags`."""
    m, found = run_model("old", name, reader)
    n = len(found)
    # before the reader: every abandoned tick's K1 counted, every scan listed, C_NT is the last workgroup's share
    assert m.cell_count.sum() == rc.ABANDONED * n
    assert m.nt == 0 < n == m.ns  # -> no pressure at all in a download, an export, a probe row, a frame; count 0 in stats
    listed = len(rc.sort_tasks(rc.cell_counts(found)))
    if name == "pile":
        # the second abandoned scan sees doubled buckets: 3000 and 600 particles are 3 + 1 chunks
        assert listed == 3 and m.ntasks == 3 + 4 and m.nbig == 4
    else:
        assert listed == 0 and m.ntasks == 0
    m.read_by(reader)
    assert (m.nbig, m.ntasks) == ((4, 7) if name == "pile" else (0, 0))  # never reset
    assert m.nt < n  # never restored
    top = m.tick(found)
    if reader == "download":
        assert top == (rc.ABANDONED + 1) * n  # bucket starts up to (A + 1) n: past every array sized for n
        assert m.cell_count.sum() == rc.ABANDONED * n  # ... and the surplus stays for good
    else:
        assert top == n
    if name == "pile":
        stale = m.ran[:7]
        if reader == "synchronize":  # the tick's own three tasks and, beside them, the stale seven
            assert len(m.ran) == 7 + 3 and m.ran[7:] == rc.sort_tasks(rc.cell_counts(found))
            assert all(t in stale for t in m.ran[7:])  # two workgroups sort the same chunk in place
        # a state with smaller buckets in those cells: every stale task runs past its bucket
        after = rc.cell_counts(rc.pile_after()[0])
        assert all(chunk * rc.SORT_CHUNK + length > after[cell] for cell, chunk, length in stale)


@pytest.mark.parametrize("reader", ["synchronize", "download"])
@pytest.mark.parametrize("name", ["quiet", "walls", "pile"])
def test_model_new_rule_restores_the_counters(name, reader):
    m, found = run_model("new", name, reader)
    n = len(found)
    assert m.cell_count.sum() == n  # the ticks behind the first abandoned one did not count again
    m.read_by(reader)
    had = len(history(name)[rc.GOOD_BEFORE - 1][0])  # (walls: the band's slots have no pressure yet)
    assert not m.cell_count.any() and (m.nbig, m.ntasks) == (0, 0) and m.ns == n and m.nt == had
    top = m.tick(found)
    assert top == n and m.nt == n and not m.cell_count.any()
    assert m.ran == rc.sort_tasks(rc.cell_counts(found))  # this tick's tasks and no others
    # another state on the same context: its own tasks only, each inside its bucket
    m.upload(rc.pile_after()[0])
    after = rc.cell_counts(rc.pile_after()[0])
    assert m.tick(rc.pile_after()[0]) == len(rc.pile_after()[0])
    assert m.ran == rc.sort_tasks(after)
    assert all(chunk * rc.SORT_CHUNK + length <= after[cell] for cell, chunk, length in m.ran)


def test_model_noise_stream_position():
    """The device-held stream of noise="host": a tick draws 2 sum C_i doubles over the rows of its first C_NT sorted slots.
    Under the old rule an abandoned tick drew for the rows the last finished tick left there; under the new one it draws
    nothing.  On these worlds C_NT is 0 after an abandoned scan (see above), so the old rule drew nothing either: the
    stream tests of test_gpu_recovery.py hold the gate to its contract, but what they would have caught before it is the
    count -- sc_step_stats reported 0 particles, and "host-sync" recorded that."""
    from oracle.neighbors import neighbor_lists
    states = history("quiet")
    counts = neighbor_lists(states[rc.GOOD_BEFORE - 1][0], rc.D)[0]
    assert counts.sum() > len(counts)  # the world has lists to draw for: more than a neighbor per particle
    m, found = run_model("old", "quiet", "download")
    _, order = strip_sort(states[rc.GOOD_BEFORE - 1][0], rc.D)  # the table the abandoned ticks find: the last tick's
    assert int(counts[order][:m.nt].sum()) == 0 and m.nt != len(found)
    m, found = run_model("new", "quiet", "download")
    m.read_by("download")
    assert m.nt == len(found)
