"""The named inputs of the per-cluster sums' tests.  tests/test_cluster_sums_cpu.py proves that each has the property it is
named for; tests/test_gpu_cluster_sums.py runs each on the device against tests/cluster_sums_spec.py, byte for byte.
The shapes are the smallest at which the reduction can go wrong: the sizes around one, two and 64 groups of 64, a cluster
that reaches the fourth level, clusters that interleave in index so that only the sort brings them together."""
import functools

import numpy as np

import cluster_cases as CK

RADIUS = 1.0
LADDER_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097)
CHAIN4 = 64 ** 3 + 1          # 262,145: 4,097 chunks, 65 partials, 2 partials, 1 -- four levels
CHAIN4_SINGLETONS = 3


def labels_of_groups(group):
    """Labels by construction: `group[i]` says which set point i belongs to (-1: none); the clusters are numbered in
    ascending order of their smallest member, as tests/cluster_spec.py numbers them."""
    group = np.asarray(group, dtype=np.int64)
    labels = np.full(len(group), -1, dtype=np.int64)
    alive = np.flatnonzero(group >= 0)
    if len(alive) == 0:
        return labels, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    _, first = np.unique(group[alive], return_index=True)       # the first (smallest) member of every set
    roots = np.sort(alive[first])
    number = np.empty(int(group.max()) + 1, dtype=np.int64)
    number[group[roots]] = np.arange(len(roots))
    labels[alive] = number[group[alive]]
    return labels, np.bincount(labels[alive], minlength=len(roots)).astype(np.int64), roots.astype(np.int64)


def chains(sizes, seed=None, spacing=0.5, rows_apart=3.0):
    """Chains of the given sizes, points `spacing` radii apart, the chains `rows_apart` radii above each other; with a seed
    the indices are a permutation of the whole.  -> (points, group of every point)."""
    pts, group = [], []
    for row, size in enumerate(sizes):
        k = np.arange(size, dtype=np.float64)
        pts.append(np.stack([spacing * RADIUS * k, np.full(size, rows_apart * RADIUS * row)], axis=1))
        group.append(np.full(size, row, dtype=np.int64))
    pts, group = np.concatenate(pts), np.concatenate(group)
    if seed is not None:
        order = np.random.RandomState(seed).permutation(len(pts))
        pts, group = pts[order], group[order]
    return pts, group


def order_channel(n):
    """(1e16, 1, -1e16, 1, ...): a sum of these shows the order it was taken in."""
    return np.tile(np.array([1e16, 1.0, -1e16, 1.0]), n // 4 + 1)[:n]


def table(seed, n, width=8):
    """Seeded normals times 1e-3, 1 or 1e3 per entry, and in column 3 (column 0 when there is only one) the order channel."""
    rs = np.random.RandomState(seed)
    v = rs.standard_normal((n, width)) * np.array([1e-3, 1.0, 1e3])[rs.randint(0, 3, size=(n, width))]
    v[:, 3 if width > 3 else 0] = order_channel(n)
    return v


def ladder():
    """-> (points, values (n, 8), labels, sizes, roots): the LADDER_SIZES chains, interleaved in index."""
    pts, group = chains(LADDER_SIZES, seed=91)
    return (pts, table(92, len(pts)), *labels_of_groups(group))


def chain4(length=CHAIN4, singletons=CHAIN4_SINGLETONS):
    """One chain of `length` points in path order, and behind it a few singletons far from it and from each other."""
    pts, group = chains((length,) + (1,) * singletons)
    return (pts, table(93, len(pts), 2), *labels_of_groups(group))


def isolated_dead():
    """`cluster_cases.isolated`'s 500 singletons with points that are not finite scattered through them in
    `cluster_cases.not_finite`'s pattern; every dead row's values are NaN."""
    pts, _ = CK.isolated()
    pts = pts.copy()
    bad = [np.nan, np.inf, -np.inf]
    dead = np.random.RandomState(94).choice(len(pts), 90, replace=False)
    for k, i in enumerate(dead):
        v = bad[k % 3]
        if k % 4 == 0:
            pts[i] = (v, bad[(k + 1) % 3])
        elif k % 4 in (1, 3):
            pts[i, 0] = v
        else:
            pts[i, 1] = v
    group = np.arange(len(pts))
    group[dead] = -1
    values = table(95, len(pts), 3)
    values[dead] = np.nan
    return (pts, values, *labels_of_groups(group))


def special():
    """Radius 1, four clusters far apart, two channels.  0: three points of -0.0 only (the rule gives +0.0).  1: five points,
    one value NaN.  2: four points with +inf and -inf among them (the sum is NaN, the extrema are the infinities).  3: a
    cluster of one.  The second channel is finite everywhere."""
    sizes = (3, 5, 4, 1)
    pts, group = chains(sizes)
    values = np.stack([np.array([-0.0, -0.0, -0.0, 1.0, 2.0, np.nan, 4.0, 5.0, 1.5, np.inf, -np.inf, 2.5, -7.25]),
                       np.arange(13.0) - 3.5], axis=1)
    return (pts, values, *labels_of_groups(group))


@functools.lru_cache(maxsize=None)
def cases():
    out = {"ladder": ladder(), "chain4": chain4(), "isolated_dead": isolated_dead(), "special": special()}
    for case in out.values():
        for a in case:
            a.setflags(write=False)
    return out
