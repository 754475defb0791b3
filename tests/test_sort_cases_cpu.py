"""tests/sort_cases.py on the CPU: every world has the property it is named for, a tick with dt = 0 changes nothing, and a
plain model of the sort chain -- buckets filled in any arrival order, k_sort_big chunk by chunk, K4's five ways to rank --
gives np.lexsort((ids, x, row)) on both routes, reaches both sides of every edge the worlds were built around, and stops
doing so under each of the wrong rules listed at the end.  No device."""
import re
from pathlib import Path

import numpy as np
import pytest

import recovery_cases as rc
import sort_cases as sc

ROOT = Path(__file__).resolve().parent.parent
WINDOW, SERIAL, COOP, SORTED1, SORTEDN = "window", "serial", "cooperative", "one sorted chunk", "several sorted chunks"


def test_constants_mirror_the_kernels():
    text = (ROOT / "sand_crate_amd" / "csrc" / "sc_kernels.h").read_text()
    for name, value in sc.CONSTANTS.items():
        assert int(re.search(r"constexpr int " + name + r"\s*=\s*(\d+)\s*;", text).group(1)) == value, name
    assert re.search(r"constexpr int kScanPerBlock\s*=\s*kBlock \* kScanPerThread;", text)
    assert re.search(r"constexpr int kSampleStride\s*=\s*kSortChunk / kSortBins;", text)
    device = (ROOT / "sand_crate_amd" / "csrc" / "sc_device.h").read_text()
    assert int(re.search(r"constexpr int kBlock\s*=\s*(\d+)\s*;", device).group(1)) == sc.SCATTER_BLOCK
    assert sc.SCAN_PER_BLOCK == sc.SCATTER_BLOCK * sc.SCAN_PER_THREAD
    assert "((unsigned)cell * 2654435761u) >> 23" in text  # table_hash


# ---------------------------------------------------------------- the worlds are what they are named for
def buckets_of(name):
    """-> (p, ids, d, cells, counts, order = reference order, start of every cell in it)."""
    (p, v, ids), d = sc.world(name)
    q = fixed(name)
    cells = sc.cells_of(q, d)
    counts = np.bincount(cells, minlength=sc.grid(d)[1] ** 2)
    return q, ids, d, cells, counts, sc.reference_order(q, ids, d), np.cumsum(counts) - counts


def fixed(name):
    """The positions the sort sees: after the hard wall fix, which moves nobody but in wall_pile."""
    from oracle.tick import hard_wall_fix, wall_contacts
    (p, _, _), d = sc.world(name)
    if name != "wall_pile":
        assert rc.wall_distance(p).min() > 1.2 * d / 2
        return p
    orc = rc.oracle(rc.PILE_COEF)
    V, u, _ = wall_contacts(p, orc.segments, orc.body_states(), d / 2)
    return hard_wall_fix(p, V, u, d / 2)


@pytest.mark.parametrize("name", list(sc.WORLDS))
def test_every_world_is_a_state(name):
    (p, v, ids), d = sc.world(name)
    n = len(p)
    assert p.shape == v.shape == (n, 2) and ids.shape == (n,) and (v != 0).any()
    assert np.array_equal(np.sort(ids), np.arange(n)) and (ids != np.arange(n)).mean() > 0.9
    z = p[:, 0] + 1j * p[:, 1]
    assert len(np.unique(z)) == n  # no two particles in one place: every pair has a direction
    assert (p > 0).all() and (p < 1).all()
    if name not in ("table_collisions",):  # storage order says nothing about the cell
        cells = sc.cells_of(p, d)
        assert (np.diff(cells) < 0).sum() > 50


def test_ladder_has_every_size_in_every_kind():
    p, ids, d, cells, counts, order, start = buckets_of("ladder")
    assert len(p) == 3 * sum(sc.LADDER_SIZES) == 130116
    for kind in sc.KINDS:
        for k, n in enumerate(sc.LADDER_SIZES):
            c = sc.cell_index(sc.LADDER_ROWS[kind], sc.LADDER_COL0 + k)
            assert counts[c] == n
            x = p[cells == c, 0]
            distinct = len(np.unique(x))
            assert distinct == dict(distinct=n, five=min(n, 5), one=1)[kind]
            if kind == "five" and n >= 10:
                assert np.bincount(np.unique(x, return_inverse=True)[1]).min() >= n // 5  # every value is a tie
        row = sc.cell_index(sc.LADDER_ROWS[kind], sc.LADDER_COL0) + np.arange(len(sc.LADDER_SIZES))
        assert np.array_equal(counts[row], sc.LADDER_SIZES)  # side by side: neighbours in the sorted order
    assert counts.sum() == counts[counts > 0].sum() and (counts > 0).sum() == 3 * len(sc.LADDER_SIZES)


def test_ends_first_last_and_one_workgroup_with_three_big_buckets():
    p, ids, d, cells, counts, order, start = buckets_of("ends")
    n = len(p)
    sorted_cells = cells[order]
    first, second = sorted_cells[0], sorted_cells[13]
    assert (sorted_cells[:13] == first).all() and (sorted_cells[13:38] == second).all() and sorted_cells[38] != second
    assert first == sc.cell_index(2, 2) and counts[first] == 13 and counts[second] == 25
    last, before = sorted_cells[-1], sorted_cells[-14]
    assert (sorted_cells[-13:] == last).all() and (sorted_cells[-110:-13] == before).all() and sorted_cells[-111] != before
    assert counts[last] == 13 and counts[before] == 97
    assert n % sc.REORDER_BLOCK not in (0, sc.REORDER_BLOCK - 1)
    run = [sc.cell_index(r, c) for r, c, _ in sc.ENDS_RUN]
    assert [counts[c] for c in run] == [97, 25, 1025] and run[1] == run[0] + 1 and run[2] == run[1] + 1
    group = start[run[1]] // sc.REORDER_BLOCK  # the workgroup of the 25's first slot
    held = set(sorted_cells[group * sc.REORDER_BLOCK:(group + 1) * sc.REORDER_BLOCK])
    assert held == set(run)  # ... holds all of the 25, the 97's tail and the 1025's head
    assert all(counts[c] > sc.BIG_BUCKET for c in run)


def test_scan_neighbours_sit_where_the_scan_splits_its_work():
    p, ids, d, cells, counts, order, start = buckets_of("scan_neighbours")
    pairs = sc.scan_pairs()
    for name, ((row, col), sizes) in pairs.items():
        i = sc.cell_index(row, col, d)
        assert sc.cell_index(row, col + 1, d) == i + 1
        assert (counts[i], counts[i + 1]) == sizes and min(sizes) > sc.SORT_THRESHOLD
        thread = lambda c: (c % sc.SCAN_PER_BLOCK) // sc.SCAN_PER_THREAD  # noqa: E731
        block = lambda c: c // sc.SCAN_PER_BLOCK  # noqa: E731
        if name == "same_thread":
            assert block(i) == block(i + 1) and thread(i) == thread(i + 1)
        elif name == "lanes":
            assert block(i) == block(i + 1) and thread(i) % 64 == 63 and thread(i + 1) == thread(i) + 1
        else:
            assert block(i + 1) == block(i) + 1 and (i + 1) % sc.SCAN_PER_BLOCK == 0
    assert (counts > sc.SORT_THRESHOLD).sum() == 6
    assert sc.grid(d)[1] ** 2 + 1 > 4 * sc.SCAN_PER_BLOCK  # five workgroups


def probe(cells, order):
    """cell_tab_insert for `cells` in that order -> {cell: slot}."""
    table = {}
    used = set()
    for c in np.asarray(cells)[order]:
        if c in table:
            continue
        s = int(sc.table_hash(c))
        while s in used:
            s = (s + 1) & (sc.CELL_TAB_SLOTS - 1)
        used.add(s)
        table[int(c)] = s
    return table


def test_table_collisions_fill_a_chain_across_the_tables_end():
    p, ids, d, cells, counts, order, start = buckets_of("table_collisions")
    B = sc.SCATTER_BLOCK
    first, second, third = cells[:B], cells[B:2 * B], cells[2 * B:]
    assert len(set(first)) == B <= sc.CELL_TAB_SLOTS // 2
    h = sc.table_hash(first)
    value, many = np.bincount(h).argmax(), np.bincount(h).max()
    assert many >= 40 and value + many > sc.CELL_TAB_SLOTS  # the chain needs `many` slots and has fewer before the end
    same = set(first[h == value])
    rs = np.random.RandomState(1)
    for _ in range(5):  # whatever the order the threads arrive in
        slots = probe(first, rs.permutation(B))
        chain = sorted(slots[c] for c in same)
        assert chain[0] < value and len(set(chain)) == many  # some of it sits at the table's start
    pile = sc.cell_index(*sc.TABLE_BUCKET_CELL, d)
    assert counts[pile] == sc.TABLE_BUCKET == 300 and pile not in set(first)
    assert same <= set(second) and (second == pile).sum() == 156 and (third == pile).all() and len(third) == 144
    assert len(set(second)) == 101 and (counts > sc.SORT_THRESHOLD).sum() == 1
    slots = probe(second, rs.permutation(B))
    assert any(slots[c] < value for c in same)


def test_wall_pile_touches_the_left_wall():
    (p, v, ids), d = sc.world("wall_pile")
    r = d / 2
    q, _, _, cells, counts, order, start = buckets_of("wall_pile")
    for (row, col), n in zip(sc.WALL_PILE_CELLS, sc.WALL_PILE_SIZES):
        c = sc.cell_index(row, col)
        assert counts[c] == n
        assert (p[cells == c, 0] <= 1.2 * r).all() and (p[cells == c, 0] < r).mean() > 0.5
        assert (np.abs(q[cells == c, 0] - r) < 1e-15).mean() > 0.5  # ... and the fix leaves them on x = r: near-ties, ties
    assert (counts > sc.SORT_THRESHOLD).sum() == 2 and not v[p[:, 0] < d].any()
    moved = (q != p).any(axis=1)
    assert moved.sum() > 900 and (p[moved, 0] < r).all()
    assert rc.PILE_COEF["dt"] == rc.DT / 20 and rc.PILE_COEF["particle_radius"] == r


def test_overflow_lists_more_tasks_than_fit():
    p, ids, d, cells, counts, order, start = buckets_of("overflow")
    sizes = np.bincount(counts)
    assert sizes[97] == 16300 and sizes[2049] == 30 and sizes[1:].sum() == 16330
    assert len(p) == 16300 * 97 + 30 * 2049 == 1642570
    tasks = sc.sort_tasks(counts)
    assert len(tasks) == sc.OVERFLOW_TASKS == 16390 > sc.MAX_SORT_TASKS
    assert d == 1.0 / 160


# ---------------------------------------------------------------- no time passes: a tick changes nothing
@pytest.mark.parametrize("name", ["ends", "scan_neighbours", "table_collisions", "short_ladder", "prime"])
def test_a_tick_with_no_time_step_changes_nothing(name):
    """The oracle's tick under quiet_coef: positions and velocities come back bit for bit (every update is
    v + 0 * finite, and every listed pair has a direction: no two particles coincide), so every particle stays in its cell.
    (`ladder` and `overflow` differ from short_ladder in their bucket sizes only: the same generator, the same premise --
    distinct places: test_every_world_is_a_state --, and lists of 20 neighbours either way.)"""
    from oracle.tick import tick_core
    if name == "short_ladder":
        state, d = sc.ladder(tuple(n for n in sc.LADDER_SIZES if n <= 513)), sc.D
    elif name == "prime":
        state, d = sc.prime(sc.D_FINE), sc.D_FINE
    else:
        state, d = sc.world(name)
    p, v, ids = state
    coef = sc.quiet_coef(d, len(p))
    orc = rc.oracle(coef)
    out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef)
    assert np.isfinite(out["pressure"]).all() and out["neighbor_counts"].max() == 20
    for got, want in ((out["particles"], p), (out["velocities"], v), (out["fixed_positions"], p)):
        assert got.tobytes() == np.ascontiguousarray(want).tobytes()
    assert not out["wall_count"].any()
    assert np.array_equal(sc.cells_of(out["particles"], d), sc.cells_of(p, d))


def test_prime_raises_the_hint():
    for d in (sc.D, sc.D_SCAN, sc.D_FINE):
        p, v, ids = sc.prime(d)
        counts = np.bincount(sc.cells_of(p, d))
        assert counts.max() == 97 and (counts > sc.SORT_THRESHOLD).sum() == 1
        assert rc.wall_distance(p).min() > 1.2 * d / 2


# ---------------------------------------------------------------- the chain, as a model
RULES = ("tie by storage index", "own chunk only", "first group of four only", "last chunk taken as full",
         "cooperative stops after 256", "serial padding counts as below", "window resolves at twelve",
         "cut bucket keeps its cell", "search by x alone", "slot before the start is the same cell")


def less(xa, ta, xb, tb, rule=None):
    """key_less: (x, id) in their total order."""
    if rule == "search by x alone":
        return xa < xb
    return (xa < xb) | ((xa == xb) & (ta < tb))


def chain(q, ids, d, route, seed, rule=None, max_tasks=sc.MAX_SORT_TASKS):
    """-> (storage indices in the chain's final order, or -1 where no particle landed; path of every particle; notes).
    `q`: the wall-fixed positions.  route "plain": no k_sort_big, nothing stamped; "sorting": the listed buckets are sorted
    chunk by chunk and stamped.  `seed`: the order in which particles arrive in their buckets and buckets in the list."""
    n = len(q)
    x = q[:, 0]
    tie = np.arange(n) if rule == "tie by storage index" else ids
    cells = sc.cells_of(q, d)
    counts = np.bincount(cells, minlength=sc.grid(d)[1] ** 2)
    start = np.cumsum(counts) - counts
    rs = np.random.RandomState(seed)
    src = np.lexsort((rs.rand(n), cells))  # the scatter: a bucket's slots in arrival order
    notes = dict(chunk_lengths=set(), steps={}, groups={}, cut=0, spans={})
    stamped = set()
    if route == "sorting":  # k_scan_cells' list, in the order the atomics hand out, and k_sort_big
        first = 0
        for cell in rs.permutation(np.flatnonzero(counts > sc.SORT_THRESHOLD)):
            size = int(counts[cell])
            nt = -(-size // sc.SORT_CHUNK)
            fits = first + nt <= max_tasks or rule == "cut bucket keeps its cell"
            notes["cut"] += not fits
            for j in range(nt):
                if first + j < max_tasks and fits:
                    length = min(sc.SORT_CHUNK, size - j * sc.SORT_CHUNK)
                    if rule == "last chunk taken as full":
                        length = sc.SORT_CHUNK
                    lo = start[cell] + j * sc.SORT_CHUNK
                    seg = src[lo:min(lo + length, n)]
                    src[lo:lo + len(seg)] = seg[np.lexsort((tie[seg], x[seg]))]
                    notes["chunk_lengths"].add(length)
                    if j == 0:
                        stamped.add(int(cell))
            first += nt
    order = np.full(n, -1, dtype=np.int64)
    path = np.empty(n, dtype=object)
    W = sc.RANK_WINDOW
    for cell in np.flatnonzero(counts):
        b, size = int(start[cell]), int(counts[cell])
        e = b + size
        seg = src[b:e]
        if (cells[seg] != cell).any():  # a task sorted across the bucket's end: nothing below is meaningful
            return order, path, notes
        kx, kt, pos = x[seg], tie[seg], np.arange(size)
        notes["spans"][size] = (e - 1) // sc.REORDER_BLOCK - b // sc.REORDER_BLOCK + 1
        nl, nr = np.minimum(pos, W), np.minimum(size - 1 - pos, W)  # same-cell slots either side, as far as the window shows
        if rule == "slot before the start is the same cell" and b == 0:
            nl = np.full(size, W)  # the slots before slot 0 read slot 0's cell: this bucket's
        resolved = (nl <= W) & (nr <= W) if rule == "window resolves at twelve" else (nl < W) & (nr < W)
        rank = np.zeros(size, dtype=np.int64)
        presorted = size > sc.SORT_THRESHOLD and cell in stamped
        for k in np.flatnonzero(resolved):  # 1. from the window, four entries per step
            lo, hi = k - nl[k], k + nr[k]
            for w in range(lo, hi + 1, 4):
                for u in range(4):
                    m = min(w + u, hi)
                    rank[k] += bool(w + u <= hi and less(kx[m], kt[m], kx[k], kt[k], rule))
            path[seg[k]] = WINDOW
        rest = np.flatnonzero(~resolved)
        if len(rest) == 0:
            pass
        elif presorted:  # 4., 5. the position in the particle's chunk, and a lower bound in each of the others
            nch = -(-size // sc.SORT_CHUNK)
            mine = rest // sc.SORT_CHUNK
            rank[rest] = rest - mine * sc.SORT_CHUNK
            groups = 0
            for r0 in range(0, nch, sc.RANK_SIDE):
                if rule == "own chunk only" or (rule == "first group of four only" and r0 > 0):
                    break
                groups += 1
                for r in range(r0, min(r0 + sc.RANK_SIDE, nch)):
                    who = rest[mine != r]
                    lo = np.full(len(who), r * sc.SORT_CHUNK)
                    hi = np.full(len(who), min((r + 1) * sc.SORT_CHUNK, size))
                    while (lo < hi).any():
                        live = lo < hi
                        mid = np.where(live, (lo + hi) >> 1, 0)
                        below = less(kx[mid], kt[mid], kx[who], kt[who], rule)
                        lo = np.where(live & below, mid + 1, lo)
                        hi = np.where(live & ~below, mid, hi)
                    rank[who] += lo - r * sc.SORT_CHUNK
            notes["groups"][size] = groups
            path[seg[rest]] = SORTED1 if nch == 1 else SORTEDN
        elif size > sc.BIG_BUCKET:  # 3. cooperatively, the bucket's keys in steps of 256
            steps = 0
            for base in range(0, size, sc.RANK_CHUNK):
                cx, ct = kx[base:base + sc.RANK_CHUNK], kt[base:base + sc.RANK_CHUNK]
                rank[rest] += less(cx[None, :], ct[None, :], kx[rest, None], kt[rest, None], rule).sum(axis=1)
                steps += 1
                if rule == "cooperative stops after 256":
                    break
            notes["steps"][size] = steps
            path[seg[rest]] = COOP
        else:  # 2. serially, four keys per step; a slot past the bucket's end counts as the particle itself
            for k in rest:
                for t in range(0, size, 4):
                    for u in range(4):
                        if t + u < size:
                            rank[k] += bool(less(kx[t + u], kt[t + u], kx[k], kt[k], rule))
                        elif rule == "serial padding counts as below":
                            rank[k] += 1
                path[seg[k]] = SERIAL
        dst = b + np.where(resolved, pos - nl, 0) + rank  # (resolved: the bucket starts where the particle's run does, s - nl)
        ok = (dst >= 0) & (dst < n)
        order[dst[ok]] = seg[ok]
    return order, path, notes


_runs = {}


def run(name, route, seed=0, rule=None, max_tasks=sc.MAX_SORT_TASKS):
    key = (name, route, seed, rule, max_tasks)
    if key not in _runs:
        q, ids, d, cells, counts, order, start = buckets_of(name)
        _runs[key] = chain(q, ids, d, route, seed, rule, max_tasks) + (order, counts[cells])
    return _runs[key]


SMALL = ("ends", "scan_neighbours", "table_collisions", "wall_pile")


@pytest.mark.parametrize("route", ["plain", "sorting"])
@pytest.mark.parametrize("name", list(sc.WORLDS))
def test_the_model_gives_the_order_whatever_the_arrival_order(name, route):
    for seed in ((0, 1, 2) if name in SMALL else (0,)):
        got, path, notes, want, _ = run(name, route, seed)
        assert np.array_equal(got, want)
        if name == "overflow" and route == "sorting":
            assert notes["cut"] >= 1  # whichever buckets the list's end falls on
    if name in SMALL and route == "sorting":  # a list of two tasks, or none: buckets are cut, and ranked all the same
        got, path, notes, want, _ = run(name, route, 3, max_tasks=0 if name == "table_collisions" else 2)
        assert np.array_equal(got, want) and notes["cut"] >= 1


# ---------------------------------------------------------------- both sides of every edge
def paths_by_size(name, route):
    got, path, notes, want, size_of = run(name, route)
    return {int(n): set(path[size_of == n]) for n in np.unique(size_of)}, notes


def test_both_sides_of_every_edge_are_ranked():
    """The coverage table: for every edge the worlds were built around, the particles of the ladder (and of `ends`) that
    the model ranks by the path on either side of it.  Every row is asserted."""
    plain, pn = paths_by_size("ladder", "plain")
    sort, sn = paths_by_size("ladder", "sorting")
    table = []

    def row(edge, below, above):
        table.append((edge, below, above))

    for ways in (plain, sort):  # the small buckets go the same ways on both routes
        row("kRankWindow: both ends show (12) / one does not (13)", ways[12] == {WINDOW}, ways[13] == {WINDOW, SERIAL})
        row("2 kRankWindow - 1 = 23: some resolved / 24: none", ways[23] == {WINDOW, SERIAL}, ways[24] == {SERIAL})
        row("kBigBucket: 24 serial / 25 cooperative", ways[24] == {SERIAL}, ways[25] == {COOP} and ways[26] == {COOP})
        row("1 and 2: the window alone", ways[1] == {WINDOW}, ways[2] == {WINDOW})
    row("kSortThreshold, plain: 96 and 97 cooperative", plain[96] == {COOP}, plain[97] == {COOP} and plain[8193] == {COOP})
    row("kSortThreshold, sorting: 96 cooperative / 97 sorted", sort[96] == {COOP}, sort[97] == {SORTED1} and sort[98] == {SORTED1})
    row("kRankChunk: one step (255, 256) / two (257)", pn["steps"][255] == pn["steps"][256] == 1, pn["steps"][257] == 2)
    row("kRankChunk: 32 steps (8192) / 33 (8193)", pn["steps"][8192] == 32, pn["steps"][8193] == 33)
    row("kRankChunk, sorting route: only up to kSortThreshold", max(sn["steps"]) == 96, min(sn["steps"]) == 25)
    row("kSortChunk: one chunk (1023, 1024) / two (1025)", sort[1023] == sort[1024] == {SORTED1}, sort[1025] == {SORTEDN})
    row("kSortChunk: two chunks (2047, 2048) / three (2049)", sn["groups"][2048] == 1, sn["groups"][2049] == 1 and sort[2049] == {SORTEDN})
    row("kRankSide: four chunks, one group (4096) / five, two (4097)", sn["groups"][4096] == 1, sn["groups"][4097] == 2)
    row("kRankSide: eight chunks, two groups (8192) / nine, three (8193)", sn["groups"][8192] == 2, sn["groups"][8193] == 3)
    lengths = sn["chunk_lengths"]
    row("kSortBlock: a chunk of 511, 512: one key per thread / 513: two", {511, 512} <= lengths, 513 in lengths)
    row("a last chunk of 4: one sample / of 5: two", 4 in lengths and -(-4 // sc.SAMPLE_STRIDE) == 1, 5 in lengths and -(-5 // sc.SAMPLE_STRIDE) == 2)
    row("a last chunk of 1 (1025, 2049, 4097, 8193) / a full one", 1 in lengths, 1024 in lengths)
    row("a chunk of 1023: 256 samples, the last one its last key but three", 1023 in lengths, 97 in lengths)
    row("kReorderBlock: a bucket inside one workgroup / across two", any(v == 1 for v in pn["spans"].values()), pn["spans"][65] >= 2 and pn["spans"][8193] >= 128)
    ends_plain, en = paths_by_size("ends", "plain")
    ends_sort, _ = paths_by_size("ends", "sorting")
    row("ends: 13 first and last, window and serial", ends_plain[13] == {WINDOW, SERIAL}, ends_sort[13] == {WINDOW, SERIAL})
    row("ends: three pending buckets (plain) / one (sorting)", ends_plain[25] == ends_plain[97] == ends_plain[1025] == {COOP},
        ends_sort[25] == {COOP} and ends_sort[97] == {SORTED1} and ends_sort[1025] == {SORTEDN})
    for kind in sc.KINDS:  # every kind of x goes every way: the buckets of a size are three, one per kind
        q, ids, d, cells, counts, order, start = buckets_of("ladder")
        got, path, notes, want, size_of = run("ladder", "sorting")
        mine = np.floor(q[:, 1] / d).astype(int) == sc.LADDER_ROWS[kind]
        row(f"{kind}: all five ways", set(path[mine]) == {WINDOW, SERIAL, COOP, SORTED1, SORTEDN}, mine.sum() == sum(sc.LADDER_SIZES))
    missed = [edge for edge, below, above in table if not (below and above)]
    assert not missed and len(table) >= 24, missed


# ---------------------------------------------------------------- wrong rules are seen
SEEN_ON = {  # rule -> (world, route, max_tasks): where the model under that rule gives another order
    "tie by storage index": ("ends", "plain", sc.MAX_SORT_TASKS),
    "own chunk only": ("ends", "sorting", sc.MAX_SORT_TASKS),
    "first group of four only": ("ladder", "sorting", sc.MAX_SORT_TASKS),
    "last chunk taken as full": ("ends", "sorting", sc.MAX_SORT_TASKS),
    "cooperative stops after 256": ("scan_neighbours", "plain", sc.MAX_SORT_TASKS),
    "serial padding counts as below": ("ends", "plain", sc.MAX_SORT_TASKS),
    "window resolves at twelve": ("ends", "plain", sc.MAX_SORT_TASKS),
    "cut bucket keeps its cell": ("scan_neighbours", "sorting", 2),
    "search by x alone": ("scan_neighbours", "sorting", sc.MAX_SORT_TASKS),
}


@pytest.mark.parametrize("rule", RULES)
def test_a_wrong_rule_gives_another_order(rule):
    """Each rule is a one-line change of `chain` (search for the rule's name).  Nine of them give another order on the
    world named in SEEN_ON, whose right order the same call without the rule gives.
    The tenth does not, on any world, and that is a property of K4 worth holding: a window slot before slot 0 taken as the
    bucket's own cell makes the left run twelve long, the bucket counts as unresolved and is ranked from its keys in
    global memory, rightly (2 kRankWindow - 1 <= kBigBucket: what the window would have resolved, the serial loop can).
    It changes the path of the first bucket's particles, never the order."""
    if rule in SEEN_ON:
        name, route, max_tasks = SEEN_ON[rule]
        right, _, _, want, _ = run(name, route, 0, None, max_tasks)
        wrong, _, _, _, _ = run(name, route, 0, rule, max_tasks)
        assert np.array_equal(right, want) and not np.array_equal(wrong, want)
        return
    assert rule == "slot before the start is the same cell"
    for name in ("ends", "scan_neighbours", "table_collisions", "wall_pile"):
        for route in ("plain", "sorting"):
            right, path, _, want, _ = run(name, route)
            wrong, other, _, _, _ = run(name, route, 0, rule)
            assert np.array_equal(wrong, want)
            if name == "ends":
                moved = np.flatnonzero(path != other)
                assert len(moved) == 11 and set(path[moved]) == {WINDOW} and set(other[moved]) == {SERIAL}
                assert np.isin(want[:13], moved).sum() == 11  # the first bucket's, but the two its own ends leave unresolved


def test_the_tie_break_is_seen_by_id_only_where_ids_are_not_the_index():
    """What neighbor_search's worlds cannot see: with ids = arange the rule "tie by storage index" is the right one."""
    q, ids, d, cells, counts, order, start = buckets_of("ends")
    same, _, _ = chain(q, np.arange(len(q)), d, "plain", 0, "tie by storage index")
    assert np.array_equal(same, sc.reference_order(q, np.arange(len(q)), d))
