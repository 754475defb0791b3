"""The named inputs of the nearest-k tables' tests: name -> (points (n, 2) float64, radius, k, queries (q, 2) float64 or None).
tests/test_nearest_cpu.py proves that each has the property it is named for; tests/test_gpu_nearest.py runs each on the
device against tests/nearest_spec.py.  The search's own edges come from tests/pairs_cases.py, each with one k; the cases
made here are those where the selection can go wrong.  The width and the hashed table come from the implementation's
constants mirrored in `sand_crate_amd._native` (NEAREST_*, PAIRS_*)."""
import functools

import numpy as np

import pairs_cases as K
from sand_crate_amd import _native as N

KS = (1, 2, 16, 17, 32, 33, 64)     # each side of every change of the kernel (its places per row in LDS), and the ends
OUTSIDE = "query_outside_domain"    # the one case whose result is the domain error


def arrival(points, radius, row_point, self_index=None):
    """The order in which the device's walk meets the partners of a row at `row_point`: the nine cells in raster order, a
    cell's bucket by the exported hash, a bucket's members ascending in index (the binning sort is stable), a candidate
    accepted only in its own cell -> the list of j."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    buckets = N.pairs_buckets(len(pts))
    cells = K.cells_of(pts, radius)
    (cx0, cy0), = K.cells_of([row_point], radius)
    r2 = np.float64(radius) * np.float64(radius)
    out = []
    for c in range(9):
        cx, cy = cx0 + c % 3 - 1, cy0 + c // 3 - 1
        b = N.pairs_bucket(cx, cy, buckets)
        for j in range(len(pts)):                                                   # ascending in index
            if N.pairs_bucket(*cells[j], buckets) != b or cells[j] != (cx, cy) or j == self_index:
                continue
            dx, dy = np.float64(row_point[0]) - pts[j, 0], np.float64(row_point[1]) - pts[j, 1]
            if dx * dx + dy * dy <= r2:
                out.append(j)
    return out


def groups(k):
    """Groups of 1, k, k + 1 and k + 2 points, each inside a disk of 0.45 radii and 10 radii from the next, shuffled: every
    row of a group of g points has g - 1 partners -- 0, k - 1, k and k + 1."""
    rs = np.random.RandomState(300 + k)
    radius = 0.125
    pts = [np.array([10.0 * radius * g, 0.0]) + 0.45 * radius * disk(rs, size)
           for g, size in enumerate((1, k, k + 1, k + 2))]
    pts = np.concatenate(pts)
    return pts[rs.permutation(len(pts))], radius


def disk(rs, n):
    r, a = np.sqrt(rs.rand(n)), 2 * np.pi * rs.rand(n)
    return np.stack([r * np.cos(a), r * np.sin(a)], axis=1)


def pile(n=70):
    """n coincident points: every d2 is 0, row i gets the smallest j != i."""
    return np.tile([[0.3, -0.7]], (n, 1)), 0.1


def ordered_arrival(descending, counts=(10, 30, 10)):
    """Row 0's candidates lie on a line through three cells of its cell row -- left, own, right, which the walk visits in
    this order -- with indices such that they reach the row in strictly descending (or ascending) order of the key."""
    radius = 0.2
    h = float(K.cell_size(radius))
    cx, cy = 40, -3
    y = (cy + 0.5) * h
    at = 0.95 if descending else 0.05
    row = (cx + at) * h
    left, own, right = counts
    # distances in cells: the far side 0.951 .. 0.99 (inside the radius, h / (1 + 2^-20)), the own cell 0.15 .. 0.85, the
    # near side 0.06 .. 0.09
    far, mid, near = np.linspace(0.99, 0.951, left), np.linspace(0.85, 0.15, own), np.linspace(0.09, 0.06, right)
    if descending:
        xs = np.concatenate([row - far * h, row - mid * h, row + near * h])
    else:
        xs = np.concatenate([row - near[::-1] * h, row + mid[::-1] * h, row + far[::-1] * h])
    pts = np.stack([np.concatenate([[row], xs]), np.full(1 + len(xs), y)], axis=1)
    return pts, radius


def nine_cells():
    """Row 0 is fed by all nine cells, 12 partners in each (108 > 64), beside an ordinary cloud; the pattern of
    pairs_cases.long_rows, the indices behind row 0 shuffled."""
    rs = np.random.RandomState(61)
    radius = 0.05
    h = float(K.cell_size(radius))
    centre = np.array([[(100 + 0.5) * h, (100 + 0.5) * h]])
    ring = [centre + np.array([[0.6 * dx * h, 0.6 * dy * h]]) + 0.08 * h * (rs.rand(12, 2) - 0.5)
            for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    rest = np.concatenate(ring + [rs.rand(150, 2)])
    return np.concatenate([centre, rest[rs.permutation(len(rest))]]), radius


def width_sizes():
    """(n, k): n one below, at and one above the workgroup's width -- and twice the width, the second workgroup full --
    for a k of every kernel: 16, and the smallest k of the two larger ones, so that even the smallest n has rows with
    more than k partners."""
    ks = [N.NEAREST_SLOTS[0]] + [slots + 1 for slots in N.NEAREST_SLOTS[:-1]]
    return [(w + d, k) for k in ks for w in (N.nearest_width(k), 2 * N.nearest_width(k)) for d in (-1, 0, 1)]


def query_cases():
    out = {}
    pts, radius = K.cloud(71, 100)
    out["q_0"] = (pts, radius, 4, np.zeros((0, 2)))
    out["n_0_q_10"] = (np.zeros((0, 2)), 0.1, 3, np.random.RandomState(72).rand(10, 2))
    pts, radius = K.cloud(73, 700, partners=12.0)
    rs = np.random.RandomState(74)
    out["q_300"] = (pts, radius, 16, rs.rand(300, 2))
    queries = rs.rand(40, 2)
    queries[::4] = pts[rs.choice(700, 10, replace=False)]
    out["query_on_a_point"] = (pts, radius, 5, queries)
    queries = rs.rand(30, 2)
    queries[3] = (np.nan, 0.5)
    queries[7] = (0.5, np.inf)
    queries[11] = (-np.inf, np.nan)
    queries[29, 0] = np.nan
    out["query_not_finite"] = (pts, radius, 17, queries)
    out["query_in_empty_cells"] = (pts, radius, 2, np.array([[100.0, 100.0], [-50.0, 3.0], [0.5, 0.5], [0.5, -7.0 * radius],
                                                             [1.0 + 1.5 * radius, 0.5], [1e6, -1e6]]))
    pts, radius = K.cloud(41, 70)
    queries = rs.rand(9, 2)
    queries[4, 1] = -(2.0 ** 30)                                                      # radius 0.5: exactly 2^31 radii
    out[OUTSIDE] = (pts, 0.5, 8, queries)
    queries = queries.copy()
    queries[4, 1] = np.nextafter(queries[4, 1], 0)                                    # one ulp inside: fine
    out["query_one_ulp_inside"] = (pts, 0.5, 8, queries)
    pts, radius = K.domain_rim()
    top = 2.0 ** 31
    out["query_at_the_rim"] = (pts, radius, 3, np.array([[np.nextafter(top, 0), 0.25], [top - 1.0, 0.0], [-(top - 0.75), 0.0],
                                                         [0.25, -np.nextafter(top, 0)], [np.nextafter(top, 0), np.nextafter(top, 0)],
                                                         [-np.nextafter(top, 0), -np.nextafter(top, 0)]]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for at, (name, (pts, radius)) in enumerate(K.cases().items()):
        k = 8 if name == "three_passes" else KS[at % len(KS)]
        out[f"{name}_k_{k}"] = (pts, radius, k, None)
    for k in KS:
        out[f"groups_k_{k}"] = (*groups(k), k, None)
    for k in (2, 3):
        out[f"tie_at_the_cut_k_{k}"] = (*K.lattice(0.25), k, None)
    for k in (64, 5):
        out[f"pile_70_k_{k}"] = (*pile(), k, None)
    for k in (16, 33):
        out[f"descending_arrival_k_{k}"] = (*ordered_arrival(True), k, None)
        out[f"ascending_arrival_k_{k}"] = (*ordered_arrival(False), k, None)
    out["nine_cells_k_64"] = (*nine_cells(), 64, None)
    for n, k in width_sizes():
        out[f"width_n_{n}_k_{k}"] = (*K.cloud(500 + n, n, partners=1.4 * k), k, None)
    out.update(query_cases())
    for pts, _, _, queries in out.values():
        pts.setflags(write=False)
        if queries is not None:
            queries.setflags(write=False)
    return out
