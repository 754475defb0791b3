"""The named inputs of the pair search's tests: name -> (points (n, 2) float64, radius).  tests/test_pairs_cases_cpu.py
proves that each has the property it is named for; tests/test_gpu_pairs.py runs each on the device against
tests/pairs_spec.py.  The sizes and the hashed table come from the implementation's constants mirrored in
`sand_crate_amd._native` (PAIRS_*)."""
import functools

import numpy as np

from sand_crate_amd import _native as N


def cell_size(radius):
    return np.float64(radius) * np.float64(N.PAIRS_CELL_FACTOR)


def cells_of(points, radius):
    """The cells the device computes: floor(fl(c / h)) per coordinate, as Python ints (finite coordinates only)."""
    h = cell_size(radius)
    return [(int(np.floor(x / h)), int(np.floor(y / h))) for x, y in np.asarray(points, dtype=np.float64).reshape(-1, 2)]


def cloud(seed, n, partners=6.0):
    """n uniform points in the unit square and the radius at which a point has about `partners` partners."""
    rs = np.random.RandomState(seed)
    return rs.rand(n, 2), float(np.sqrt(partners / (np.pi * max(n, 1))))


def edge_sizes():
    """0, 1, 2, around a wave, and one below, at and above every width at which a launch gains a workgroup: a block of the
    row kernels, a tile of the binning sort, a block of the scans (of the 256 digit counts per tile, of the buckets, of
    the row lengths), and a size with three blocks of the 64-bit scan."""
    sizes = {0, 1, 2, 63, 64, 65}
    for w in (N.PAIRS_BLOCK, N.PAIRS_SORT_TILE, N.PAIRS_SCAN_BLOCK, 2 * N.PAIRS_SCAN_BLOCK):
        sizes |= {w - 1, w, w + 1}
    # the bucket table doubles where PAIRS_LOAD * n passes a power of two: 128 / 129 points, 1024 / 1025, ...
    sizes |= {N.PAIRS_MIN_BUCKETS // N.PAIRS_LOAD, N.PAIRS_MIN_BUCKETS // N.PAIRS_LOAD + 1, 1024, 1025}
    assert max(sizes) <= 5000
    return sorted(sizes)


def shared_bucket_cells(buckets):
    """-> (centre cell, two of its nine cells that share a bucket, a far cell in the centre cell's bucket), found by
    search with the exported hash."""
    for cx in range(3, 4000):
        cy = 7
        nine = [(cx + dx, cy + dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        seen = {}
        for cell in nine:
            b = N.pairs_bucket(*cell, buckets)
            if b in seen:
                own = N.pairs_bucket(cx, cy, buckets)
                far = next((fx, -50000) for fx in range(100000, 200000) if N.pairs_bucket(fx, -50000, buckets) == own)
                return (cx, cy), (seen[b], cell), far
            seen[b] = cell
    raise AssertionError("no cell with two neighbours in one bucket")


def bucket_sharing():
    """Radius 1.  A centre point in the middle of its cell with partners in all eight cells around -- two of the nine share
    a bucket -- and three points in a far cell that falls into the centre cell's bucket, partners of each other only."""
    n = 9 + 3
    buckets = N.pairs_buckets(n)
    (cx, cy), _, (fx, fy) = shared_bucket_cells(buckets)
    h = float(cell_size(1.0))
    pts = [((cx + 0.5 + 0.55 * dx) * h, (cy + 0.5 + 0.55 * dy) * h) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    pts += [((fx + 0.5) * h, (fy + 0.5) * h), ((fx + 0.25) * h, (fy + 0.5) * h), ((fx + 0.5) * h, (fy + 0.75) * h)]
    order = np.random.RandomState(4).permutation(n)
    return np.array(pts)[order], 1.0


def long_rows():
    """Piles of 65, 257 and 300 coincident points (longer than a wave, than a workgroup) beside an ordinary cloud, and a
    point whose row is fed by all nine cells: 12 partners in each, the indices of all points shuffled together."""
    rs = np.random.RandomState(21)
    radius = 0.05
    h = float(cell_size(radius))
    pts = [np.tile([[0.2, 0.2]], (65, 1)), np.tile([[0.8, 0.2]], (257, 1)), np.tile([[0.2, 0.8]], (300, 1)), rs.rand(200, 2)]
    centre = np.array([[(100 + 0.5) * h, (100 + 0.5) * h]])
    ring = [centre + np.array([[0.6 * dx * h, 0.6 * dy * h]]) + 0.08 * h * (rs.rand(12, 2) - 0.5)
            for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    pts = np.concatenate(pts + [centre] + ring)
    return pts[rs.permutation(len(pts))], radius


def non_finite():
    pts, radius = cloud(31, 300, partners=8.0)
    rs = np.random.RandomState(32)
    bad = rs.choice(300, 60, replace=False)
    values = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(bad):
        v = values[k % 3]
        if k % 4 == 0:
            pts[i] = (v, values[(k + 1) % 3])
        elif k % 4 in (1, 3):
            pts[i, 0] = v
        else:
            pts[i, 1] = v
    return pts, radius


def three_passes():
    """The smallest n whose table has 65536 buckets: the keys 0 .. 65536 then need 17 bits, and the binning sort a third
    pass of eight.  40 points with a coordinate that is not finite carry the key 65536, the only one with a non-zero third
    digit: that pass has to move them behind every live point (every smaller case has an even number of passes)."""
    n = 32768 // N.PAIRS_LOAD + 1
    pts, radius = cloud(51, n)
    values = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(np.random.RandomState(52).choice(n, 40, replace=False)):
        pts[i, k % 2] = values[k % 3]
    return pts, radius


def lattice(radius, reach=3):
    """Points on exact multiples of the radius, negative ones and -0.0 included (fl(k * radius), k = -reach .. reach)."""
    k = np.arange(-reach, reach + 1, dtype=np.float64)
    c = k * np.float64(radius)
    c[reach] = -0.0
    x, y = np.meshgrid(c, c)
    return np.stack([x.ravel(), y.ravel()], axis=1), radius


def eight_cells():
    """Radius 0.37.  A point in the middle of cell (0, 0) with one partner in each of the eight cells around it, and eight
    points two cells away, which are nobody's partners."""
    radius = 0.37
    h = float(cell_size(radius))
    c = 0.5 * h
    near = [(c + 0.6 * h * dx, c + 0.6 * h * dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    far = [(c + 2.0 * h * dx, c + 2.0 * h * dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    return np.array([(c, c)] + near + far), radius


def misplaced_floor():
    """Radius 0.01.  0.03 and 0.06: floor(fl(c / 0.01)) is not the cell the exact quotient lies in.  With their
    neighbours a radius away, on both axes."""
    c = np.array([0.0, 0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, np.nextafter(0.03, 0), np.nextafter(0.06, 1)])
    x, y = np.meshgrid(c, c)
    return np.stack([x.ravel(), y.ravel()], axis=1), 0.01


def large_cells():
    """Radius 0.01 near 1e3: cell indices near 1e5, where fl(c / h) has lost 17 bits behind the point."""
    k = np.arange(-4, 5, dtype=np.float64)
    c = np.concatenate([1e3 + k * 0.01, [np.nextafter(1e3, 0), 1e3 + 0.005]])
    x, y = np.meshgrid(c, -c)
    return np.stack([x.ravel(), y.ravel()], axis=1), 0.01


def domain_rim():
    """Radius 1, coordinates just inside |c| / radius < 2^31: the outermost cells there are."""
    top = 2.0 ** 31
    return np.array([[top - 1.5, 0.0], [top - 0.75, 0.0], [-(top - 0.5), 0.25], [-(top - 1.25), 0.0],
                     [np.nextafter(top, 0), 0.5], [0.0, -np.nextafter(top, 0)], [0.5, -(top - 0.5)]]), 1.0


def outside_domain():
    """Radius 0.5 and one coordinate at exactly 2^31 radii."""
    pts, _ = cloud(41, 70)
    pts[33, 1] = -(2.0 ** 30)
    return pts, 0.5


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in edge_sizes():
        out[f"n_{n}"] = cloud(100 + n, n)
    out["at_radius_3_4_5"] = (np.array([[0.0, 0.0], [3.0, 4.0]]), 5.0)
    out["beyond_radius_3_4_5"] = (np.array([[0.0, 0.0], [3.0, np.nextafter(4.0, 5.0)]]), 5.0)
    out["radius_0.1"] = (np.array([[0.0, 0.0], [0.1, 0.0], [0.06, 0.08], [0.0, -0.1], [0.1, 0.1], [-0.08, 0.06],
                                   [np.nextafter(0.1, 1), 0.0], [0.3, 0.4], [0.3, 0.5], [0.36, 0.48]]), 0.1)
    out["lattice_0.25"] = lattice(0.25)
    out["lattice_0.01"] = lattice(0.01)
    out["eight_cells"] = eight_cells()
    out["misplaced_floor"] = misplaced_floor()
    out["large_cells"] = large_cells()
    out["bucket_sharing"] = bucket_sharing()
    out["long_rows"] = long_rows()
    out["non_finite"] = non_finite()
    out["domain_rim"] = domain_rim()
    out["three_passes"] = three_passes()
    for pts, _ in out.values():
        pts.setflags(write=False)
    return out


BIG_PILE = 65536   # coincident points: E = 65536 * 65535 = 4,294,901,760: beyond 31 bits, and beyond 32 as a byte offset
