"""Every world of tests/tile_cases.py is what it claims to be: exact totals, exact reach, exact scan ranges, block
alignment -- by the helpers and the oracle alone.  These are not tolerances: a world that misses its size by one fails."""
import numpy as np
import pytest

import tile_cases as tc
from oracle.neighbors import neighbor_lists, strip_sort

TILE = tc.TILE


def _named(points, d, block):
    counts, table = neighbor_lists(points, d)
    lo, hi = tc.list_reach(points, d, counts, table)
    return lo[block], hi[block], counts


@pytest.mark.parametrize("n", tc.LONE_SIZES + tc.LONE_BIG_SIZES)
def test_lone_bucket(n):
    pts = tc.lone_bucket(n)
    assert len(pts) <= 70000
    totals = tc.tile_totals(pts, tc.D)
    full = n // TILE
    assert full >= 3 and np.array_equal(totals[:full], np.tile([n, 0, 0], (full, 1)))
    rows, order = strip_sort(pts, tc.D)
    cols = np.floor(pts[order, 0] / tc.D).astype(np.int64)
    assert np.all(rows[:n] == rows[0]) and np.all(cols[:n] == cols[0])  # one cell, first in the order
    rest = slice(n, None)
    assert not np.any((np.abs(rows[rest] - rows[0]) <= 2) & (np.abs(cols[rest] - cols[0]) <= 2))
    if n > 2 * tc.ROW_SLOT_MAX:  # the closed form's premise: everybody within d of everybody
        assert len(pts) == n and np.ptp(pts[:, 0]) ** 2 + np.ptp(pts[:, 1]) ** 2 < tc.D ** 2


def _check_banded(pts, block, total, reach):
    d = tc.D
    totals = tc.tile_totals(pts, d)[block]
    assert totals.sum() == total and np.all(totals > 0) and totals[0] == TILE
    rows, _ = strip_sort(pts, d)
    blk = slice(block * TILE, (block + 1) * TILE)
    assert np.all(rows[blk] == rows[block * TILE])                    # one row holds the block ...
    assert rows[block * TILE - 1] < rows[block * TILE] < rows[(block + 1) * TILE]  # ... and nothing else
    lo, hi, counts = _named(pts, d, block)
    assert tc.reach_total(lo[None], hi[None])[0] == reach
    first = np.array([0, totals[0], totals[0] + totals[1]])
    extra = (total - reach) // 4  # particles beyond the reach at each end of the two outer ranges
    assert np.array_equal(lo, first + [0, extra, extra])
    assert np.array_equal(hi, first + totals - 1 - [0, extra, extra])
    return counts


@pytest.mark.parametrize("t", tc.RANGE_SIZES)
def test_three_ranges(t):
    pts, block = tc.three_ranges(t)
    counts = _check_banded(pts, block, t, t)  # (the highest slot named is t - 1: the end of the previous rows' range)
    assert counts.max() <= 20 and (counts < 20).sum() > TILE


@pytest.mark.parametrize("r", tc.REACH_SIZES)
def test_reach_edge(r):
    pts, block = tc.reach_edge(r)
    _check_banded(pts, block, r + 1600, r)
    assert r + 1600 > tc.TILE_CAP_B + 500 and r + 1600 < tc.SLOT_MAX


def test_stacked_worlds_keep_their_blocks():
    worlds = [tc.three_ranges(961), tc.three_ranges(1101)]
    pts, blocks = tc.stacked(worlds)
    assert 2500 < len(pts) < 3500 and len(pts) % TILE == 0
    totals = tc.tile_totals(pts, tc.D)
    assert [int(totals[b].sum()) for b in blocks] == [961, 1101] and np.all(totals[blocks] > 0)
    lo, hi, _ = _named(pts, tc.D, blocks)
    assert np.array_equal(tc.reach_total(lo, hi), [961, 1101])


def test_scan_lengths():
    d = tc.D
    pts, below, above = tc.scan_lengths()
    counts, first = tc.scan_ranges(pts, d)
    nb_counts, nb_table = neighbor_lists(pts, d)
    rows, order = strip_sort(pts, d)
    pos = np.empty(len(pts), dtype=np.int64)
    pos[order] = np.arange(len(pts))
    bounds = tc.tile_bounds(pts, d)
    totals = tc.tile_totals(pts, d)
    pile = len(pts) - 2 * TILE
    assert 2000 < pile < 8000 and np.all(rows[TILE:TILE + pile] == rows[TILE])
    seen = {1: [], 3: []}
    slots = {1: [], 3: []}
    for watchers, scan in ((below, 1), (above, 3)):
        for k, n in watchers:
            blk = k // TILE
            assert k // TILE in (0, len(totals) - 1)
            # the block of the watchers: its own 256, the pile in the row the scan looks at and nothing in the other one;
            # wider than either pass A window, so the search goes through the sliding window
            rng = 1 if scan == 1 else 2
            assert totals[blk][0] == TILE and totals[blk][3 - rng] == 0 and totals[blk][rng] > 1536
            assert counts[k, scan] == n and counts[k, 0] == 0 and counts[k, 2] == 0 and counts[k, 4 - scan] == 0
            # one neighbor: the last but one candidate of the scan
            me = order[k]
            assert nb_counts[me] == 1
            hit = pos[nb_table[me, 0]]
            assert hit == (first[k, 1] + n - 2 if scan == 1 else first[k, 3] - (n - 2))
            seen[scan].append(n)
            a = bounds[blk][2 * rng]
            slots[scan].append(TILE + int(first[k, scan]) - int(a))  # tile slot of the scan's first candidate
    for scan in (1, 3):
        assert set(tc.SCAN_LENGTHS) <= set(seen[scan])
    starts = slots[1]
    ends = [s + n for s, (_, n) in zip(starts, below)]
    for half in tc.HALF.values():
        cap = 2 * half
        on_grid = [s for s in starts if s % half == 0 and s > 0]
        assert set(tc.SCAN_STARTS_ON_GRID) <= set(on_grid)
        # a window is staged at the half-window grid point at or below the scan that is furthest behind: scans that start
        # on the grid with nothing unfinished less than half a window below place it on themselves
        for w in tc.SCAN_STARTS_ON_GRID:
            assert not [s for s in starts if w - half <= s < w]
            assert [e for e in ends if w < e and 1 <= w + cap - e <= 3]
    for name, half in tc.HALF.items():
        for e, w in zip(tc.SCAN_ENDS[name], tc.SCAN_STARTS_ON_GRID):
            assert e in ends and 1 <= w + 2 * half - e <= 3


@pytest.mark.parametrize("seed", [1, 2])
def test_tile_totals_against_a_cell_start_array(seed):
    """The lexicographic interval is the row-major interval of a grid with a ring of empty cells (sc_tiled.h, header):
    counted here directly from an explicit cellStart array."""
    rs = np.random.RandomState(seed)
    n, d = 3000 + 500 * seed, 0.031
    pts = np.vstack((rs.rand(n, 2) * 0.9 + 0.05, 0.4 + rs.rand(700, 2) * d * 1.5))
    rows, order = strip_sort(pts, d)
    cols = np.floor(pts[order, 0] / d).astype(np.int64)
    row0, col0 = rows.min() - 1, cols.min() - 1                # the ring
    nrows, ncols = rows.max() - row0 + 2, cols.max() - col0 + 2
    cell = (rows - row0) * ncols + (cols - col0)
    assert np.all(np.diff(cell) >= 0)
    cell_start = np.searchsorted(cell, np.arange(nrows * ncols + 1), side="left")
    expect = []
    for i0 in range(0, len(pts), TILE):
        cf, cl = cell[i0], cell[min(i0 + TILE, len(pts)) - 1]
        expect.append([cell_start[cl + 2 + s] - cell_start[cf - 1 + s] for s in (0, ncols, -ncols)])
    assert np.array_equal(tc.tile_totals(pts, d), np.array(expect))
    assert max(sum(e) for e in expect) > 960  # (some tile of the patch is beyond pass B's budget)
