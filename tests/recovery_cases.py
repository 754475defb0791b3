"""Worlds for what a context is worth after a reported error (tests/test_gpu_recovery.py,
tests/test_recovery_cases_cpu.py): a tick abandoned behind its bucket scan (sc_set_scan_patience(-1)) and a particle
dropped as NaN, at the smallest sizes that still reach the paths -- and a NumPy model of the counters an abandoned tick
leaves behind, under the rule before the recovery was written and under the rule of `recover_flags`
(csrc/sandcrate_hip.hip).

All worlds: d = 0.012 in a fixed box, no motored body (the host would keep moving it through abandoned ticks, and a twin
that ran no abandoned tick would see other walls).

  quiet       6,000 particles, sparse and uniform, none within 1.2 r of a wall through its ticks: the wall fix of the
              abandoned tick's first kernel changes nothing, positions compare exactly.  93 x 93 cells: five workgroups in
              the scan (one could not give up), no bucket above kSortThreshold.
  walls       quiet plus a band inside r of the floor, APPENDED after the good ticks: the wall fix runs in the abandoned
              tick.  (It leaves nobody inside r, and no tick moves a particle there -- the crossing check stops it on the
              wall's pad, at r or an ulp beyond --, so only new particles can be found there.  The band's slots also
              have no pressure yet: what the abandoned tick leaves must say so.)
  pile        a cell of 1,500 particles (two chunks of kSortChunk), a cell of 300, 3,000 sparse ones, in random storage
              order; a short dt keeps the piles in their cells.
  pile_after  another state for the same context: 200 and 120 particles in those two cells, 1,100 and 250 in two others
              -- a task listed for `pile` runs past its bucket here.
  nan         quiet plus one particle exactly on the left wall, in the middle of the ids.
  dense       70,000 particles, uniform: more than the 65,536 ids up to which one small launch draws the noise of
              noise="host" (sc_rng.h: kSmallIds); still no bucket above kSortThreshold.  Twin runs only, no oracle.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import math

import numpy as np

from oracle.scene import OracleCrate
from oracle.world import World

D = 0.012
R = D / 2
DT = 0.002 * D / 0.01

SCAN_PER_BLOCK = 2048   # sc_kernels.h: kScanPerBlock -- cells per workgroup of k_scan_cells
SORT_THRESHOLD = 96     # sc_kernels.h: kSortThreshold -- buckets above it are listed for k_sort_big
SORT_CHUNK = 1024       # sc_kernels.h: kSortChunk -- slots per task of k_sort_big
ABANDONED = 2           # A: the abandoned ticks of every test
GOOD_BEFORE, GOOD_AFTER = 2, 3

COEF = dict(spring_overlap_balance=0.5, spring_amplifier=100.0,  # (scene files carry these two; no tick reads them)
            dt=DT, particle_radius=R, wall_collision_decay=0.3, pressure_amplifier=30.0, ignored_pressure=0.2,
            collider_noise_level=0.1, viscosity=4.0, surface_smoothing=80.0, target_pressure=-1.0, gravity=[0.0, 9.8],
            max_particles=100000)
PILE_COEF = dict(COEF, dt=DT / 20)  # a pile's pressures are in the tens: at the full dt it leaves its cell within a tick

BOX = {"fixed": {"name": "box", "segments": [[[0.0, 0.0], [1.0, 0.0]], [[1.0, 0.0], [1.0, 1.0]],
                                             [[1.0, 1.0], [0.0, 1.0]], [[0.0, 1.0], [0.0, 0.0]]]}}

PILE_CELLS = ((40, 30), (55, 60))        # (row, column) = (floor(y / d), floor(x / d)) of pile's two big buckets
PILE_AFTER_CELLS = ((20, 50), (70, 25))  # ... and of the two that only pile_after fills
PILE_SIZES = (1500, 300)
PILE_AFTER_SIZES = (200, 120)            # what pile_after keeps in PILE_CELLS
PILE_AFTER_OWN = (1100, 250)             # ... and puts into PILE_AFTER_CELLS


def oracle(coef=COEF):
    return OracleCrate(World([BOX], [], dict(coef)))


# ---------------------------------------------------------------- the cell grid, restated (sandcrate_hip.hip: build_world)
def grid(d=D):
    """-> (row0 = col0, nrows = ncols): the grid covers [-r, 1 + r]^2, three cells of margin and a ring of empty cells."""
    r = d / 2
    cmin = math.floor(-r / d) - 3
    cmax = math.floor((1 + r) / d) + 3
    return cmin - 1, cmax - cmin + 1 + 2


def cells_of(p, d=D):
    """The bucket of every particle: (floor(y / d) - row0) * ncols + floor(x / d) - col0 (collision_detector.py:126)."""
    c0, n = grid(d)
    row = np.floor(p[:, 1] / d).astype(np.int64) - c0
    col = np.floor(p[:, 0] / d).astype(np.int64) - c0
    assert ((row >= 1) & (row <= n - 2) & (col >= 1) & (col <= n - 2)).all()
    return row * n + col


def cell_index(row, col, d=D):
    c0, n = grid(d)
    return (row - c0) * n + (col - c0)


def cell_counts(p, d=D):
    _, n = grid(d)
    return np.bincount(cells_of(p, d), minlength=n * n)


def scan_workgroups(d=D):
    _, n = grid(d)
    return (n * n + 1 + SCAN_PER_BLOCK - 1) // SCAN_PER_BLOCK  # (the one-past-the-end entry is scanned too)


def wall_distance(p):
    """Distance to the nearest wall of the unit box, for points inside it."""
    return np.minimum(np.minimum(p[:, 0], 1 - p[:, 0]), np.minimum(p[:, 1], 1 - p[:, 1]))


def capacity(*counts):
    """Room for (A + 2) n particles: bucket starts of A abandoned ticks' counts under the next tick's stay inside arrays
    sized by the capacity even where nothing put them right."""
    return (ABANDONED + 2) * max(counts)


# ---------------------------------------------------------------- the worlds
def quiet(n=6000, seed=41):
    rs = np.random.RandomState(seed)
    p = 0.06 + 0.88 * rs.rand(n, 2)
    v = (rs.rand(n, 2) - 0.5) * 0.2
    return p, v


walls = quiet  # ... as uploaded


def band(n=160, seed=42):
    """walls' late arrivals: 0.15 r .. 0.9 r above the floor (y = 1: gravity points to +y), at rest."""
    rs = np.random.RandomState(seed)
    p = np.column_stack((0.1 + 0.8 * rs.rand(n), 1.0 - R * (0.15 + 0.75 * rs.rand(n))))
    return p, np.zeros_like(p)


def _in_cell(rs, row, col, n, ties=0):
    """n points well inside cell (row, col); the first `ties` share their x with another one (the id breaks the tie)."""
    f = 0.3 + 0.4 * rs.rand(n, 2)
    if ties:
        f[:ties, 0] = f[ties:2 * ties, 0]
    return np.column_stack(((col + f[:, 0]) * D, (row + f[:, 1]) * D))


def _sparse(rs, n, avoid):
    """n points on distinct cells away from the walls and from the cells in `avoid`, one per cell."""
    lo, hi = 6, 76
    taken = {tuple(c) for c in avoid}
    cells = [(r, c) for r in range(lo, hi) for c in range(lo, hi) if (r, c) not in taken]
    pick = rs.choice(len(cells), n, replace=False)
    rc = np.array(cells)[pick]
    f = 0.2 + 0.6 * rs.rand(n, 2)
    return np.column_stack(((rc[:, 1] + f[:, 0]) * D, (rc[:, 0] + f[:, 1]) * D))


def _piled(seed, groups, n_sparse):
    rs = np.random.RandomState(seed)
    parts = [_in_cell(rs, r, c, n, ties=min(n // 8, 64)) for (r, c), n in groups]
    parts.append(_sparse(rs, n_sparse, PILE_CELLS + PILE_AFTER_CELLS))
    p = np.concatenate(parts)
    v = np.zeros_like(p)
    v[-n_sparse:] = (rs.rand(n_sparse, 2) - 0.5) * 0.2
    order = rs.permutation(len(p))  # storage order says nothing about the cell
    return p[order], v[order]


def pile():
    return _piled(43, list(zip(PILE_CELLS, PILE_SIZES)), 3000)


def pile_after():
    return _piled(44, list(zip(PILE_CELLS + PILE_AFTER_CELLS, PILE_AFTER_SIZES + PILE_AFTER_OWN)), 2500)


def extra(n=7, seed=45):
    """A few particles to append after the recovery: in the big pile's cell and beside it."""
    rs = np.random.RandomState(seed)
    (row, col), _ = PILE_CELLS
    p = np.concatenate((_in_cell(rs, row, col, n - 3), _in_cell(rs, row, col + 1, 3)))
    return p, np.zeros_like(p)


def dense(n=70000, seed=46):
    return quiet(n, seed)


SMALL_IDS = 1 << 16  # sc_rng.h: kSmallIds
NAN_AT = 2987  # the id of the particle on the wall


def nan():
    p, v = quiet()
    return np.insert(p, NAN_AT, [0.0, 0.5], axis=0), np.insert(v, NAN_AT, [0.0, 0.0], axis=0)


# ---------------------------------------------------------------- the counters across ticks, as a model
def sort_tasks(counts):
    """k_scan_cells' list for one tick: (cell, chunk, length) for every chunk of every bucket above the threshold."""
    tasks = []
    for cell in np.flatnonzero(counts > SORT_THRESHOLD):
        e = int(counts[cell])
        for j in range((e + SORT_CHUNK - 1) // SORT_CHUNK):
            tasks.append((int(cell), j, min(SORT_CHUNK, e - j * SORT_CHUNK)))
    return tasks


class Counters:
    """What the kernels of a tick do to cellCount, C_NBIG / C_NTASKS (with the task list), C_NT and C_NS, tick by tick.

    A good tick: K1 adds the particles' cells, the scan lists the big buckets behind what C_NTASKS holds and writes the
    sum as C_NT, the scatter takes every count back, pass B zeroes C_NBIG / C_NTASKS and sets C_NS = C_NT.
    An abandoned tick (every workgroup of the scan but the first gives up at once): K1 and the scan as before -- but the
    last workgroup's sum is its own cells' only --, nothing else.
    rule "old":  K1 runs in every tick (the path of physics_tick: no look-ahead), a reader clears the flag
                 (sc_synchronize also zeroes cellCount).
    rule "new":  a tick that finds the flag up does not even run K1; the reader zeroes cellCount, C_NBIG, C_NTASKS and
                 puts C_NT back to the last finished tick's (`recover_flags`)."""

    def __init__(self, rule, d=D):
        assert rule in ("old", "new")
        self.rule = rule
        _, n = grid(d)
        self.ncells = n * n
        self.cell_count = np.zeros(self.ncells, dtype=np.int64)
        self.nbig = self.ntasks = 0
        self.tasks = []
        self.ran = []  # the tasks k_sort_big ran in the last finished tick
        self.ns = self.nt = self.nt_done = 0
        self.flag = False

    def upload(self, p):
        self.ns = len(p)
        self.nt_done = 0

    def append(self, k):
        self.ns += k  # (C_NT and C_NT_DONE stay: the new slots have no pressure)

    def _scan(self, abandoned):
        listed = sort_tasks(self.cell_count)
        self.tasks = self.tasks[:self.ntasks] + listed
        self.nbig += int((self.cell_count > SORT_THRESHOLD).sum())
        self.ntasks += len(listed)
        last = (self.ncells // SCAN_PER_BLOCK) * SCAN_PER_BLOCK  # the last workgroup's first cell
        self.nt = int(self.cell_count[last:].sum() if abandoned else self.cell_count.sum())
        return int(self.cell_count.sum())  # the one-past-the-end bucket start: where the next scatter's slots end

    def tick(self, p, abandon=False):
        """`p`: the positions after the wall fix.  -> the largest bucket start of the tick's scan."""
        own = np.zeros(self.ncells, dtype=np.int64)
        if not (self.rule == "new" and self.flag):
            own = np.bincount(cells_of(p), minlength=self.ncells)
            self.cell_count += own
        top = self._scan(abandon or self.flag)
        if abandon:
            self.flag = True
        if self.flag:
            return top
        self.cell_count -= own  # the scatter takes back what its particles counted, no more
        self.ran = list(self.tasks[:self.ntasks])
        self.nbig = self.ntasks = 0
        self.ns = self.nt_done = self.nt
        return top

    def read_by(self, reader):
        """The first reader of the flags: "synchronize" or "download"."""
        assert self.flag
        self.flag = False
        if self.rule == "new":
            self.cell_count[:] = 0
            self.nbig = self.ntasks = 0
            self.nt = self.nt_done
        elif reader == "synchronize":
            self.cell_count[:] = 0
