"""Worlds for the per-tick sort chain (k_scan_cells, k_scatter, k_sort_big, k_reorder = K4: csrc/sc_kernels.h) at every
size where it changes route -- tests/test_sort_cases_cpu.py proves each world has the property it is named for and holds a
plain model of the chain, tests/test_gpu_sort_cases.py runs them on both routes: the first tick that meets big buckets
(k_scatter<false>, K4 ranks everything by counting) and the ticks after it (k_scatter<true>, k_sort_big, K4 ranks sorted
chunks by position and binary search).

Every world is (points, velocities, ids) in the unit box of recovery_cases.BOX, every particle farther than 1.2 r from
every wall (no wall fix, no wall record) except in `wall_pile`.  ids are a permutation of 0 .. n - 1 and never the storage
index: the order is np.lexsort((ids, x, row)), and the tie-break by id is told from one by storage index.

  ladder            one bucket of every size in LADDER_SIZES, in three kinds of x (KINDS), one kind per grid row, the
                    buckets side by side; storage order shuffled.  130,116 particles.
  ends              13 and 25 first in the sorted order, 97 and 13 last, nlive % 64 neither 0 nor 63, and the run 97, 25,
                    1025 laid so that one 64-slot workgroup of K4 holds slots of all three.
  scan_neighbours   d = 0.011.  Pairs of big buckets in one scan thread's 8 cells, in the last lane of a wave and the first of the
                    next, and either side of a multiple of 2048 cells.
  table_collisions  d = 1/160.  Storage slots 0 .. 255 (one scatter workgroup) hold 256 distinct cells, 40 of them with
                    one hash value so close to the table's end that the probe chain wraps to slot 0; slots 256 .. 511 mix
                    those cells with a bucket of 300, which ends in a third workgroup.  Storage order is the layout.
  wall_pile         a bucket of 1,500 and one of 300 within 1.2 r of the left wall, 3,000 sparse particles, with
                    recovery_cases.PILE_COEF: the one world with a real time step, checked against the oracle's tick.
  overflow          d = 1/160.  16,300 buckets of 97 and 30 of 2,049: 16,390 tasks for a list of 16,384.

All worlds but wall_pile run with dt = 0 (`quiet_coef`): a tick changes neither positions nor velocities (proved on the
CPU), so a world can be ticked before it is tapped and the velocities K4 moved come back byte for byte.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import numpy as np

import recovery_cases as rc
from recovery_cases import cell_index, cells_of, grid, sort_tasks  # noqa: F401  (the grid, restated once: there)

RANK_WINDOW = 12        # sc_kernels.h: kRankWindow
BIG_BUCKET = 24         # kBigBucket
RANK_CHUNK = 256        # kRankChunk
REORDER_BLOCK = 64      # kReorderBlock
SORT_THRESHOLD = 96     # kSortThreshold
SORT_CHUNK = 1024       # kSortChunk
SORT_BLOCK = 512        # kSortBlock
SORT_BINS = 256         # kSortBins
SAMPLE_STRIDE = SORT_CHUNK // SORT_BINS  # 4: every fourth key of a chunk is a sample
RANK_SIDE = 4           # kRankSide
MAX_SORT_TASKS = 16384  # kMaxSortTasks
SCAN_PER_THREAD = 8     # kScanPerThread
SCAN_PER_BLOCK = 2048   # kScanPerBlock
CELL_TAB_SLOTS = 512    # kCellTabSlots
SCATTER_BLOCK = 256     # sc_device.h: kBlock -- storage slots per workgroup of k_scatter
CONSTANTS = dict(kRankWindow=RANK_WINDOW, kBigBucket=BIG_BUCKET, kRankChunk=RANK_CHUNK, kReorderBlock=REORDER_BLOCK,
                 kSortThreshold=SORT_THRESHOLD, kSortChunk=SORT_CHUNK, kSortBlock=SORT_BLOCK, kSortBins=SORT_BINS,
                 kRankSide=RANK_SIDE, kMaxSortTasks=MAX_SORT_TASKS, kScanPerThread=SCAN_PER_THREAD,
                 kCellTabSlots=CELL_TAB_SLOTS)
assert (SORT_THRESHOLD, SORT_CHUNK, SCAN_PER_BLOCK) == (rc.SORT_THRESHOLD, rc.SORT_CHUNK, rc.SCAN_PER_BLOCK)

D = rc.D            # 0.012: 93 x 93 cells, five workgroups in the scan
D_SCAN = 0.011      # 101 x 101 cells: a multiple of 2048 cells falls between two cells inside the box (at 0.012 none does)
D_FINE = 1.0 / 160  # 170 x 170 cells: enough of them to share a hash value forty times, and for 16,330 buckets

LADDER_SIZES = (1, 2, 12, 13, 23, 24, 25, 26, 63, 64, 65, 96, 97, 98, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1028,
                1029, 1535, 1536, 1537, 2047, 2048, 2049, 4096, 4097, 8192, 8193)
KINDS = ("distinct", "five", "one")  # x all distinct / five values (exact ties) / one value (ranked by id alone)
LADDER_ROWS = dict(distinct=10, five=20, one=30)
LADDER_COL0 = 4
FIVE = (0.1, 0.3, 0.5, 0.7, 0.9)


def quiet_coef(d, max_particles):
    """No time passes: v + 0 * (finite) = v and p + 0 * v = p, exactly."""
    return dict(rc.COEF, dt=0.0, particle_radius=d / 2, max_particles=max_particles)


def table_hash(cell):
    """cell_tab_insert's first slot: the top 9 bits of the 32-bit product."""
    return ((np.asarray(cell, dtype=np.int64) * 2654435761) % (1 << 32)) >> 23


def reference_order(p, ids, d):
    """Storage indices in sorted order: by (row, x, id).  (x alone suffices inside a row: cells are intervals of x.)"""
    return np.lexsort((ids, p[:, 0], np.floor(p[:, 1] / d).astype(np.int64)))


# ---------------------------------------------------------------- building blocks
def bucket(rs, row, col, n, kind, d, lo=0.05, hi=0.95):
    """n points inside cell (row, col), their x of the given kind; every y is drawn apart, so no two points coincide."""
    if kind == "distinct":
        fx = lo + (hi - lo) * (rs.permutation(n) + 0.5 * rs.rand(n)) / n
    elif kind == "five":
        fx = np.array(FIVE)[rs.permutation(n) % 5]
    else:
        fx = np.full(n, 0.5)
    fy = lo + (hi - lo) * rs.rand(n)
    return np.column_stack(((col + fx) * d, (row + fy) * d))


def finish(rs, parts, shuffle=True):
    """-> (p, v, ids): storage order shuffled, velocities random and nowhere zero, ids a permutation that is not arange."""
    p = np.concatenate(parts)
    if shuffle:
        p = p[rs.permutation(len(p))]
    v = (rs.rand(len(p), 2) - 0.5) * 0.2
    assert (v != 0).all()
    ids = rs.permutation(len(p)).astype(np.int64)
    return p, v, ids


def prime(d):
    """The state that raises the hint: one bucket of 97 and a few particles of their own."""
    rs = np.random.RandomState(60)
    parts = [bucket(rs, 5, 5, 97, "distinct", d)] + [bucket(rs, 8, 3 + 2 * k, 1, "one", d) for k in range(7)]
    return finish(rs, parts)


# ---------------------------------------------------------------- the worlds
def ladder(sizes=LADDER_SIZES):
    rs = np.random.RandomState(61)
    parts = [bucket(rs, LADDER_ROWS[kind], LADDER_COL0 + k, n, kind, D) for kind in KINDS for k, n in enumerate(sizes)]
    return finish(rs, parts)


ENDS_FIRST = ((2, 2, 13), (2, 3, 25))            # (row, col, size)
ENDS_RUN = ((40, 10, 97), (40, 11, 25), (40, 12, 1025))
ENDS_LAST = ((80, 79, 97), (80, 80, 13))
ENDS_FILL_BEFORE, ENDS_FILL_AFTER = 13, 5        # single particles in row 3 and in row 60


def ends():
    rs = np.random.RandomState(62)
    parts = [bucket(rs, r, c, n, "five" if n == 25 else "distinct", D) for r, c, n in ENDS_FIRST + ENDS_RUN + ENDS_LAST]
    parts += [bucket(rs, 3, 4 + 2 * k, 1, "one", D) for k in range(ENDS_FILL_BEFORE)]
    parts += [bucket(rs, 60, 4 + 2 * k, 1, "one", D) for k in range(ENDS_FILL_AFTER)]
    return finish(rs, parts)


def find_pair(pred, d=D_SCAN):
    """The first (row, col) with cells (row, col) and (row, col + 1) inside the box whose cell index i has pred(i)."""
    for row in range(4, 78):
        for col in range(2, 78):
            if pred(cell_index(row, col, d)):
                return row, col
    raise AssertionError("no such pair of cells")


def scan_pairs():
    """-> {name: ((row, col), sizes)}: two big buckets in cells i and i + 1."""
    same_thread = find_pair(lambda i: i % SCAN_PER_THREAD == 3)
    lanes = find_pair(lambda i: i % (64 * SCAN_PER_THREAD) == 64 * SCAN_PER_THREAD - 1 and i % SCAN_PER_BLOCK != SCAN_PER_BLOCK - 1)
    blocks = find_pair(lambda i: i % SCAN_PER_BLOCK == SCAN_PER_BLOCK - 1)
    return dict(same_thread=(same_thread, (97, 1025)), lanes=(lanes, (300, 98)), blocks=(blocks, (2049, 97)))


def scan_neighbours():
    rs = np.random.RandomState(63)
    parts = []
    for (row, col), (a, b) in scan_pairs().values():
        parts += [bucket(rs, row, col, a, "five", D_SCAN), bucket(rs, row, col + 1, b, "distinct", D_SCAN)]
    parts += [bucket(rs, 79, 3 + 2 * k, 1 + k % 3, "one", D_SCAN) for k in range(30)]
    return finish(rs, parts)


TABLE_SAME = 40    # cells of one hash value
TABLE_BUCKET = 300
TABLE_BUCKET_CELL = (100, 100)


def table_cells():
    """-> (the 40 cells that share a hash value, the other 216), as (row, col) arrays; the hash value is the largest one
    that forty cells inside the box share -- CELL_TAB_SLOTS - 40 < hash: the chain cannot end before the table does."""
    rows, cols = np.meshgrid(np.arange(3, 157), np.arange(3, 157), indexing="ij")
    rows, cols = rows.ravel(), cols.ravel()
    keep = ~((rows == TABLE_BUCKET_CELL[0]) & (cols == TABLE_BUCKET_CELL[1]))
    rows, cols = rows[keep], cols[keep]
    h = table_hash(cell_index(rows, cols, D_FINE))
    per = np.bincount(h, minlength=CELL_TAB_SLOTS)
    value = int(np.flatnonzero(per >= TABLE_SAME).max())
    same = np.flatnonzero(h == value)[:TABLE_SAME]
    rs = np.random.RandomState(64)
    rest = rs.permutation(np.flatnonzero(h != value))[:SCATTER_BLOCK - TABLE_SAME]
    return (rows[same], cols[same]), (rows[rest], cols[rest])


def table_collisions():
    rs = np.random.RandomState(65)
    (sr, sc), (orow, ocol) = table_cells()
    one = lambda r, c, kind: bucket(rs, int(r), int(c), 1, kind, D_FINE)  # noqa: E731
    first = [one(r, c, "five") for r, c in zip(sr, sc)] + [one(r, c, "five") for r, c in zip(orow, ocol)]
    first = [first[k] for k in rs.permutation(SCATTER_BLOCK)]
    pile = bucket(rs, *TABLE_BUCKET_CELL, TABLE_BUCKET, "five", D_FINE)
    second = [one(r, c, "five") for r, c in zip(sr, sc)] + [one(r, c, "five") for r, c in zip(orow[:60], ocol[:60])]
    second = np.concatenate(second + [pile[:SCATTER_BLOCK - TABLE_SAME - 60]])
    second = second[rs.permutation(SCATTER_BLOCK)]
    return finish(rs, first + [second, pile[SCATTER_BLOCK - TABLE_SAME - 60:]], shuffle=False)


WALL_PILE_CELLS = ((40, 0), (60, 0))  # column 0: x in [0, d), the left wall at x = 0
WALL_PILE_SIZES = (1500, 300)


def wall_pile():
    """x in 0.2 r .. 1.1 r: all within 1.2 r of the wall, most inside r, where the hard wall fix puts them on x = r."""
    rs = np.random.RandomState(66)
    parts = [bucket(rs, row, col, n, "distinct", D, lo=0.1, hi=0.55) for (row, col), n in zip(WALL_PILE_CELLS, WALL_PILE_SIZES)]
    parts.append(rc._sparse(rs, 3000, ()))
    p, v, ids = finish(rs, parts)
    near = p[:, 0] < D
    v[near] = 0.0  # (as recovery_cases.pile: the piles are at rest)
    return p, v, ids


OVERFLOW_SMALL, OVERFLOW_BIG = (16300, 97), (30, 2049)
OVERFLOW_TASKS = OVERFLOW_SMALL[0] + OVERFLOW_BIG[0] * 3


def overflow():
    rs = np.random.RandomState(67)
    (ns, small), (nb, big) = OVERFLOW_SMALL, OVERFLOW_BIG
    side = 154  # rows and columns 3 .. 156
    cells = rs.permutation(side * side)[:ns + nb]
    size = np.r_[np.full(ns, small), np.full(nb, big)][rs.permutation(ns + nb)]
    row, col = np.repeat(cells // side + 3, size), np.repeat(cells % side + 3, size)
    n = len(row)
    fx = np.where(rs.rand(n) < 0.5, np.array(FIVE)[rs.randint(0, 5, n)], 0.05 + 0.9 * rs.rand(n))  # half of them tie
    p = np.column_stack(((col + fx) * D_FINE, (row + 0.05 + 0.9 * rs.rand(n)) * D_FINE))
    return finish(rs, [p])


WORLDS = dict(ladder=(ladder, D), ends=(ends, D), scan_neighbours=(scan_neighbours, D_SCAN), table_collisions=(table_collisions, D_FINE),
              wall_pile=(wall_pile, D), overflow=(overflow, D_FINE))
_made = {}


def world(name):
    """-> ((p, v, ids), d), built once; nobody writes to the arrays."""
    if name not in _made:
        fn, d = WORLDS[name]
        state = fn()
        for a in state:
            a.setflags(write=False)
        _made[name] = (state, d)
    return _made[name]


def coef_of(name):
    (p, _, _), d = world(name)
    return rc.PILE_COEF if name == "wall_pile" else quiet_coef(d, len(p) + 1024)
