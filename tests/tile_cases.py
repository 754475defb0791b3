"""Worlds whose tiles have exactly the sizes at which the tiled passes change path (tests/test_gpu_tiles.py,
tests/test_tile_cases_cpu.py, tests/golden/make_golden.py: nbr_tile_edges), and a CPU restatement of the tile geometry.

csrc/sc_tiled.h compares a block's tile size, or the reach of its lists, with a handful of constants:
  1024 / 1100   pass A: LDS tile or sliding window (narrow / wide tile, SANDCRATE_TILE);
  960           pass A renumbers the table to the reach of the lists, pass B stages the tile in LDS or gathers;
  4095          12-bit row entries or the 32-bit table (one writer, three readers);
  65535         u16 tile slots or sorted indices straight into the 32-bit table;
  32, 128, 256  candidates of a windowed scan: serial stretch, wave-wide turn, probe skip; the half-window grid.
The builders below put a tile, a reach or a scan range on each of these numbers and one or two beside it.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import numpy as np

from oracle.neighbors import strip_sort

TILE = 256          # particles per block of the tiled passes (sc_device.h: kTileW)
TILE_CAP_B = 960    # sc_tiled.h: kTileCapB
ROW_SLOT_MAX = 4095  # sc_tiled.h: kRowSlotMax
SLOT_MAX = 65535    # sc_tiled.h: kSlotMax
HALF = {"narrow": 512, "wide": 768}  # sc_tiled.h: kHalf = CAP / 2 of the two pass A tiles
D = 1.0 / 256       # a power of two: (k + f) * D lies in cell k for every fraction f

EDGES = (960, 1024, 1100, 4095)
LONE_SIZES = tuple(t + k for t in EDGES for k in (-1, 0, 1, 2))
LONE_BIG_SIZES = (65534, 65535, 65536, 65537)
RANGE_SIZES = LONE_SIZES
REACH_SIZES = (959, 960, 961, 962, 4094, 4095, 4096, 4097)
SCAN_LENGTHS = (31, 32, 33, 35, 127, 128, 129, 255, 256, 257, 261)


# ---------------------------------------------------------------- the tile geometry, restated
def _sorted_cells(points, d):
    rows, order = strip_sort(points, d)
    cols = np.floor(points[order, 0] / d).astype(np.int64)
    return rows, cols, order


def _cell_keys(rows, cols):
    """(row, column) in lexicographic order as one integer; two columns of room on either side."""
    c0 = cols.min() - 2
    width = cols.max() - c0 + 3
    return lambda r, c: r * width + (c - c0)


def tile_bounds(points, d):
    """Per block of TILE sorted particles the six bounds [a0, e0, a1, e1, a2, e2) of its candidate ranges (sc_tiled.h,
    header): the sorted positions whose cell lies between the cell before the block's first cell and the cell after its
    last one, for the same rows, one row up and one row down."""
    rows, cols, _ = _sorted_cells(points, d)
    key = _cell_keys(rows, cols)
    keys = key(rows, cols)  # non-decreasing: the order is (row, x)
    n = len(rows)
    first = np.arange(0, n, TILE)
    last = np.minimum(first + TILE, n) - 1
    out = np.empty((len(first), 6), dtype=np.int64)
    for k, shift in enumerate((0, 1, -1)):
        out[:, 2 * k] = np.searchsorted(keys, key(rows[first] + shift, cols[first] - 1), side="left")
        out[:, 2 * k + 1] = np.searchsorted(keys, key(rows[last] + shift, cols[last] + 1), side="right")
    return out


def tile_totals(points, d):
    """(n0, n1, n2) per block: int64[blocks, 3]."""
    b = tile_bounds(points, d)
    return b[:, 1::2] - b[:, 0::2]


def list_reach(points, d, counts, table):
    """Per block and range the lowest and the highest tile slot that a list of the block names, the block's own particles
    included (pass_a_body: extremes): (lo, hi) int64[blocks, 3], lo > hi = -1 for a range nobody names.  `counts`, `table`:
    the oracle's lists in original index space.  A neighbor in the same strip has a slot of the first range, one in the
    next strip a slot of the second, one in the previous strip a slot of the third -- the scan that found it decides."""
    rows, _, order = _sorted_cells(points, d)
    n = len(order)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    b = tile_bounds(points, d)
    tot = b[:, 1::2] - b[:, 0::2]
    first_slot = np.column_stack((np.zeros(len(b), np.int64), tot[:, 0], tot[:, 0] + tot[:, 1]))
    src = np.repeat(np.arange(n), counts)            # original indices
    dst = table[table >= 0]
    assert len(dst) == len(src)
    i, j = np.r_[pos[src], np.arange(n)], np.r_[pos[dst], np.arange(n)]  # sorted positions; every particle names itself
    dr = rows[j] - rows[i]
    assert np.all(np.abs(dr) <= 1)
    rng = np.where(dr == 0, 0, np.where(dr == 1, 1, 2))
    blk = i // TILE
    slot = first_slot[blk, rng] + (j - b[blk, 2 * rng])
    assert np.all((slot >= first_slot[blk, rng]) & (j < b[blk, 2 * rng + 1]))
    lo = np.full((len(b), 3), np.iinfo(np.int64).max)
    hi = np.full((len(b), 3), -1, dtype=np.int64)
    np.minimum.at(lo, (blk, rng), slot)
    np.maximum.at(hi, (blk, rng), slot)
    return lo, hi


def reach_total(lo, hi):
    """Entries of the ranges a block's lists reach (pass_a_body: reach)."""
    return np.where(hi >= lo, hi - lo + 1, 0).sum(axis=1)


def scan_ranges(points, d):
    """Per sorted particle the candidate counts of its four scans -- same strip after, next strip, same strip before,
    previous strip -- and the sorted position each scan starts at (pass A: e0 - (i + 1), e1 - b1, i - b0, em - bm):
    (counts int64[n, 4], first int64[n, 4])."""
    rows, cols, _ = _sorted_cells(points, d)
    key = _cell_keys(rows, cols)
    keys = key(rows, cols)
    i = np.arange(len(rows))

    def start(r, c):
        return np.searchsorted(keys, key(r, c), side="left")

    e0, b0 = start(rows, cols + 2), start(rows, cols - 1)
    b1, e1 = start(rows + 1, cols - 1), start(rows + 1, cols + 2)
    bm, em = start(rows - 1, cols - 1), start(rows - 1, cols + 2)
    return (np.column_stack((e0 - (i + 1), e1 - b1, i - b0, em - bm)),
            np.column_stack((i + 1, b1, i - 1, em - 1)))


def cluster_lists(pts, d):
    """Neighbor lists of a cluster whose particles are ALL within d of each other and in one strip: to the
    right in (x, index) order, then to the left descending, cut at 20 (collision_detector.py:85-93)."""
    n = len(pts)
    order = np.lexsort((np.arange(n), pts[:, 0]))
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    table = np.full((n, 20), -1, dtype=np.int64)
    for i in range(n):
        k = pos[i]
        seq = list(order[k + 1:k + 21]) + list(order[max(k - 20, 0):k][::-1])
        seq = seq[:20]
        table[i, :len(seq)] = seq
    return np.full(n, 20, dtype=np.int32), table


# ---------------------------------------------------------------- builders (cell units, scaled by d at the end)
def _finish(cells_xy, d, seed):
    pts = np.asarray(cells_xy, dtype=np.float64) * d
    return pts[np.random.RandomState(seed).permutation(len(pts))]


def _lone(n, col, row, up=False):
    """n particles with nobody near them: three cells apart, forty to a row, rows going down (or up) from `row`."""
    k = np.arange(n)
    return np.column_stack((col + 0.5 + 3.0 * (k % 40), row + 0.5 + 3.0 * (k // 40) * (1 if up else -1)))


def lone_bucket(n, d=D):
    """n particles in one cell, first in the sorted order, nothing within two cells of it: every full block inside has
    (n0, n1, n2) = (n, 0, 0).  Up to 4,097 the cell is filled and a sprinkle of particles lies some rows further on; the
    65 k buckets are a patch whose particles are all within d of each other and nothing else (cluster_lists applies)."""
    rs = np.random.RandomState(n)
    if n > 2 * ROW_SLOT_MAX:
        cells = np.column_stack((128 + 0.1 + rs.rand(n) * 0.3, 100 + 0.2 + rs.rand(n) * 0.3))
    else:
        bucket = np.column_stack((128 + 0.01 + rs.rand(n) * 0.98, 100 + 0.01 + rs.rand(n) * 0.98))
        rest = np.column_stack((60 + rs.rand(300) * 130, 104 + rs.rand(300) * 40))
        cells = np.vstack((bucket, rest))
    return _finish(cells, d, n)


def _banded_block(m1, m2, extras, seed, d, row=128, col=64, width=120):
    """A block of exactly TILE particles alone in `row`, block-aligned, two per cell, between a next row with m1 and a
    previous row with m2 particles from the first to the last one a list names -- the lowest and the highest x of either
    row sit directly beside the block's first and last particle -- and, with `extras`, that many particles more at each
    of the four ends, in the outermost cells of the ranges but beyond d of every block particle."""
    rs = np.random.RandomState(seed)
    x_first, x_last = col + 0.9, col + width + 0.1
    bx = np.linspace(x_first, x_last, TILE) + (rs.rand(TILE) - 0.5) * 0.1
    bx[0], bx[-1] = x_first, x_last
    block = np.column_stack((bx, row + 0.4 + rs.rand(TILE) * 0.2))
    parts = [block]
    for m, r, fy in ((m1, row + 1, 0.02), (m2, row - 1, 0.98)):
        inner = np.column_stack((x_first - 0.25 + rs.rand(m - 2) * (x_last - x_first + 0.5), r + 0.01 + rs.rand(m - 2) * 0.98))
        # thin the two ends, so that the first and the last block particle's lists have room for the row's end
        near_end = (inner[:, 0] < x_first + 1.0) | (inner[:, 0] > x_last - 1.0)
        inner[near_end, 1] = r + (0.95 if r > row else 0.05)
        ends = np.array([[x_first - 0.3, r + fy], [x_last + 0.3, r + fy]])
        parts += [inner, ends]
        if extras:
            parts.append(np.column_stack((col - 1 + 0.01 + rs.rand(extras) * 0.8, r + 0.01 + rs.rand(extras) * 0.98)))
            parts.append(np.column_stack((col + width + 1.2 + rs.rand(extras) * 0.79, r + 0.01 + rs.rand(extras) * 0.98)))
    before = m2 + 2 * extras  # sorted ahead of the block: the previous row; lone particles further down fill the block up
    pad = -before % TILE
    parts.append(_lone(pad, col, row - 6))
    parts.append(np.column_stack((col + rs.rand(200) * width, row + 5 + rs.rand(200) * 20)))  # and a sprinkle behind
    return _finish(np.vstack(parts), d, seed), (before + pad) // TILE


def three_ranges(t, d=D):
    """-> (points, block): the block's three ranges hold t entries in all, each of them some, and the lists of the block
    name the first and the last slot of every range -- slot t - 1 is the end of the previous rows' range."""
    m2 = (t - TILE) // 2
    return _banded_block(t - TILE - m2, m2, 0, t, d)


def reach_edge(r, d=D):
    """-> (points, block): the block's candidate ranges hold r + 1,600 entries, the lists reach exactly r of them."""
    m2 = (r - TILE) // 2
    return _banded_block(r - TILE - m2, m2, 400, 100000 + r, d)


def stacked(worlds, d=D, rows_apart=60):
    """Several (points, block) worlds in one: each moved `rows_apart` rows further up than the one before and filled up
    to a whole number of blocks -> (points, blocks)."""
    out, blocks, n = [], [], 0
    for k, (pts, block) in enumerate(worlds):
        pts = pts + np.array([0.0, k * rows_apart * d])
        pad = -len(pts) % TILE
        filler = _lone(pad, 20, 128 + 28 + k * rows_apart, up=True) * d
        out += [pts, filler]
        blocks.append(n // TILE + block)
        n += len(pts) + pad
    return np.vstack(out), blocks


# pile segments of scan_lengths(), in pile order: (particles, watched).  Tile slot of pile particle k: TILE + k, for the
# watchers of both rows.  With W = 1536 and 4608 (multiples of both half windows, nothing starting within 768 slots below):
#   slot 1536  the 261-scan starts on W: the window of either width is placed there ...
#   slot 2558  ... and the 129-scan ends two slots before the narrow window's end, 1536 + 1024,
#   slot 3069  the 128-scan three before the wide one's, 1536 + 1536;
#   slot 4608  the 256-scan starts on W; the 33-scan ends at 5631, one before 4608 + 1024, the 35-scan at 6142, two
#              before 4608 + 1536.
_PILE = ((256, True),) + ((256, False),) * 4 + \
        ((261, True), (31, True), (32, True), (33, True), (35, True), (127, True), (374, False), (129, True), (383, False),
         (128, True), (513, False), (513, False), (513, False),
         (256, True), (255, True), (257, True), (222, False), (33, True), (476, False), (35, True), (2, False))
SCAN_STARTS_ON_GRID = (1536, 4608)              # first slot of a next-strip scan
SCAN_ENDS = {"narrow": (2558, 5631), "wide": (3069, 6142)}  # end (excluded) of a next-strip scan; the window's end follows


def scan_lengths(d=D):
    """-> (points, watchers_below, watchers_above): a pile of 5,888 particles in one row, in groups of three cells with
    an empty cell between them; over the middle cell of a watched group a lone particle in the row below (its next-strip
    scan is the group) and one in the row above (its previous-strip scan is).  Each watcher is within d of exactly one
    particle of its group, the last but one of its scan.  watchers_*: (sorted position, candidates) per watcher."""
    rs = np.random.RandomState(7)
    row, col = 128, 40
    pile, below, above = [], [], []
    for g, (n, watched) in enumerate(_PILE):
        c = col + 4 * g + 1
        x = c - 0.6 + 2.2 * (np.arange(n) + 0.5) / n
        y = np.full(n, row + 0.5)
        if watched:
            y[n - 2] = row + 0.02   # the hit of the watcher below: last but one of its ascending scan
            y[1] = row + 0.98       # ... of the watcher above: last but one of its descending scan
            below.append((c + 0.9, row - 0.6, n))
            above.append((c + 0.1, row + 1.6, n))
        pile.append(np.column_stack((x, y)))
    pile = np.vstack(pile)
    assert len(pile) % TILE == 0
    end = col + 4 * len(_PILE) + 3
    parts = [pile]
    for w, r in ((below, row - 1), (above, row + 1)):
        rest = TILE - len(w)
        parts.append(np.array([(x, y) for x, y, _ in w]))
        parts.append(np.column_stack((end + rs.rand(rest) * 30, r + 0.01 + rs.rand(rest) * 0.98)))
    pts = np.vstack(parts)
    watchers_below = [(k, n) for k, (_, _, n) in enumerate(below)]
    watchers_above = [(TILE + len(pile) + k, n) for k, (_, _, n) in enumerate(above)]
    return _finish(pts, d, 7), watchers_below, watchers_above
