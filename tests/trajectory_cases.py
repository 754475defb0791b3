"""Worlds and windows for the trajectory log (tests/test_gpu_trajectory.py; their premises are proved from the spec alone
in tests/test_trajectory_cpu.py).

A case is a state in STORAGE order -- the order an upload or `load_state_tensors` stores it in, slot k = row k, before
any tick -- with its ids, and the windows to record it through.

  edge_state(n, id0, M)   n particles among whose ids are id0 - 1, id0, id0 + M - 1 and id0 + M (those that exist and fit
                          n): the window cuts ids off on both sides, and its first and last row are taken.  M runs over
                          ROWS: one below, at and one above a wave and a workgroup of k_traj_clear.
  top_state()             ids up to 2^31 - 2 with a window that ends at 2^31 - 1: id0 + M passes INT_MAX in 32 bits.
  wave_state()            130 particles with ids 0..129 in storage order -- two full waves of the scatter and a tail of
                          two lanes -- and WAVE_WINDOWS, through which a full wave holds 0, 1, 63 and all 64 outsiders.
  odd_values()            live particles with -0.0, infinities and NaN in y and the velocity, and stored ones whose x is
                          NaN or infinite: absent, as in the export.
Everything here is NumPy: no device, no reference."""
from __future__ import annotations

import numpy as np

import growth_cases as G
import track_cases as tk
import trajectory_spec as T

WAVE = 64                      # lanes of a wave: the scatter counts outsiders once per wave
BLOCK = 256                    # sc_kernels.h: kBlock -- rows per workgroup of k_traj_clear, slots of k_traj_scatter
ROWS = (1, 63, 64, 65, 255, 256, 257)
LIVE_COUNTS = (0, 1, 257)
EDGE_ID0 = 1000
WAVE_COUNT = 130
WAVE_WINDOWS = ((0, 64), (1, 65), (0, 130), (64, 128))
RUN_WINDOW = (3, 2500)         # the run's window: ids below it from the first tick, ids above it before the last
RUN_TICKS = 30
EVERYS = (1, 3)


def edge_ids(n: int, id0: int, rows: int) -> np.ndarray:
    """n distinct ids in no order: the four at the window's edges first (those that exist), then ids drawn from
    [id0 - 2 rows - n, id0 + 3 rows + n): inside and outside the window, on both sides."""
    edges = []
    for i in (id0, id0 + rows, id0 - 1, id0 + rows - 1):
        if 0 <= i <= T.MAX_ID and i not in edges:
            edges.append(i)
    rs = np.random.RandomState(7 * rows + n)
    lo, hi = max(0, id0 - 2 * rows - n), min(T.MAX_ID + 1, id0 + 3 * rows + n)
    pool = np.setdiff1d(np.arange(lo, hi, dtype=np.int64), np.array(edges, dtype=np.int64))
    ids = np.concatenate([np.array(edges, dtype=np.int64), rs.permutation(pool)])[:n]
    return rs.permutation(ids)


def edge_state(n: int, id0: int, rows: int):
    """-> (xy, vxy, ids) of n particles in storage order."""
    xy, vxy = tk.cloud(rows + 3 * n, n)
    return xy, vxy, edge_ids(n, id0, rows)


def top_state():
    """-> (xy, vxy, ids, window): 257 rows that end at 2^31 - 1; ids just below the window, at its two ends, and small."""
    rows = 257
    hi = T.MAX_ID + 1
    id0 = hi - rows
    ids = np.array([T.MAX_ID, id0, id0 - 1, 0, 5, id0 + 100, T.MAX_ID - 1, 2 ** 31 - 2 ** 20, 2 ** 30], dtype=np.int64)
    xy, vxy = tk.cloud(91, len(ids))
    return xy, vxy, ids, (id0, hi)


def wave_state():
    xy, vxy = tk.cloud(92, WAVE_COUNT)
    return xy, vxy, np.arange(WAVE_COUNT, dtype=np.int64)


def outsiders_per_wave(ids_in_storage_order, window) -> list:
    """How many lanes of each wave of the scatter (64 slots each, the last one partial) hold an id outside the window."""
    ids = np.asarray(ids_in_storage_order, dtype=np.int64)
    out = (ids < window[0]) | (ids >= window[1])
    return [int(out[k:k + WAVE].sum()) for k in range(0, len(ids), WAVE)]


def odd_values():
    """-> (xy, vxy, live): 12 stored particles (ids 0..11 by upload); `live` says which the export delivers."""
    nan, inf = np.nan, np.inf
    xy = np.array([[0.5, 0.5], [0.25, -0.0], [-0.0, 0.75], [0.3, inf], [0.4, -inf], [0.6, nan], [nan, 0.5], [0.7, 0.2],
                   [inf, 0.5], [-inf, 0.1], [0.8, 0.8], [nan, nan]])
    vxy = np.array([[0.0, 0.0], [-0.0, 1.0], [inf, -inf], [nan, 0.0], [0.0, nan], [nan, nan], [1.0, 2.0], [-0.0, -0.0],
                    [3.0, 4.0], [0.0, 0.0], [inf, inf], [0.0, 0.0]])
    return xy, vxy, np.isfinite(xy[:, 0])


def run_case():
    """growth_cases' emitting-and-leaving scene: the first source's particles leave within two ticks, so the live ids
    have gaps from the start."""
    return G.cases()["sources_two_growths"]


def run_on_oracle(ticks: int):
    """The run's live ids per tick on the oracle (ample capacity): -> [ids after tick 1, after tick 2, ...].  The case has
    16 ticks of its own; the flows stay as its last edit left them."""
    case = run_case()
    longer = G.GrowthCase(case.name, case.bodies, case.sources, case.coef, ticks, case.capacities, case.growths,
                          case.flow_steps)
    return [step["ids"] for step in G.run(longer, case.ample)]
