"""Proves on the spec (tests/cluster_spec.py) that every named case of tests/cluster_cases.py has the property it is named
for, and that the spec's two ways to the clusters -- the plain search of `clusters` and the label propagation of
`components` -- agree on every small case.  No GPU."""
import functools

import numpy as np
import pytest

import cluster_cases as CK
import cluster_spec as CS
import pairs_cases as K
import pairs_spec as S
from sand_crate_amd import _native as N


@functools.lru_cache(maxsize=None)
def spec(name):
    points, radius = CK.cases()[name]
    return CS.clusters(points, radius)


def check_shape(points, labels, sizes, roots):
    """What holds for every result: the numbering by smallest member, sizes and labels that fit each other."""
    alive = np.isfinite(points).all(axis=1)
    assert labels.dtype == sizes.dtype == roots.dtype == np.int64 and labels.shape == (len(points),)
    assert (labels[~alive] == -1).all() and (labels[alive] >= 0).all()
    assert sizes.shape == roots.shape and sizes.sum() == alive.sum() and (np.diff(roots) > 0).all()
    assert np.array_equal(np.bincount(labels[alive], minlength=len(sizes)), sizes)
    assert np.array_equal(labels[roots], np.arange(len(roots)))
    first = np.full(len(sizes), len(points))
    np.minimum.at(first, labels[alive], np.flatnonzero(alive))
    assert np.array_equal(first, roots)


@pytest.mark.parametrize("name", list(CK.small_cases()))
def test_the_two_ways_agree(name):
    points, radius = CK.cases()[name]
    assert len(points) <= CK.SMALL
    want = spec(name)
    check_shape(points, *want)
    alive = np.isfinite(points).all(axis=1)
    for half in (False, True):                                                      # `half` does not change the clusters
        offsets, partners, _ = S.pairs(points, radius, half)
        got = CS.components(len(points), offsets, partners, alive=alive)
        for g, w in zip(got, want):
            assert g.dtype == np.int64 and np.array_equal(g, w)


def test_the_table_has_every_case():
    names = set(CK.cases())
    for n in K.edge_sizes():
        for partners in (2.0, 4.5, 8.0):
            assert f"n_{n}_partners_{partners}" in names
    assert {"exactly_radius", "bucket_sharing", "serpentine_along", "serpentine_reversed", "serpentine_bit_reversed",
            "serpentine_shuffled", "lattice", "two_combs", "late_root", "isolated", "piles", "not_finite", "wide"} <= names
    assert set(CK.cases()) - set(CK.small_cases()) == {"wide"}


def test_edge_sizes_span_the_regimes():
    n = max(K.edge_sizes())
    largest = [spec(f"n_{n}_partners_{p}")[1].max() / n for p in CK.PARTNERS]
    counts = [len(spec(f"n_{n}_partners_{p}")[1]) for p in CK.PARTNERS]
    assert largest[0] < 0.02 and counts[0] > n // 4                                 # many small clusters
    assert 0.02 < largest[1] < 0.9 and counts[1] > 100                              # near percolation: neither
    assert largest[2] > 0.9                                                         # one giant


def test_exactly_radius():
    points, radius = CK.cases()["exactly_radius"]
    r2 = np.float64(radius) * np.float64(radius)
    d2 = lambda a, b: (points[a, 0] - points[b, 0]) ** 2 + (points[a, 1] - points[b, 1]) ** 2  # noqa: E731
    assert d2(0, 1) == r2
    assert r2 < d2(2, 3) <= np.nextafter(np.nextafter(r2, np.inf), np.inf) and points[3, 1] == np.nextafter(points[1, 1], 1)
    cells = K.cells_of(points, radius)
    buckets = N.pairs_buckets(len(points))
    assert cells[0] == (0, 0) and cells[4] == cells[5] and abs(cells[4][0]) > 1000
    assert N.pairs_bucket(*cells[4], buckets) == N.pairs_bucket(*cells[0], buckets)
    labels, sizes, roots = spec("exactly_radius")
    assert labels.tolist() == [0, 0, 1, 2, 3, 3] and sizes.tolist() == [2, 1, 1, 2] and roots.tolist() == [0, 2, 3, 4]


def test_bucket_sharing():
    points, radius = CK.cases()["bucket_sharing"]
    cells = K.cells_of(points, radius)
    buckets = N.pairs_buckets(len(points))
    labels, sizes, roots = spec("bucket_sharing")
    assert sorted(sizes.tolist()) == [3, 9]
    far = int(np.argmin(sizes))
    near_buckets = {N.pairs_bucket(*cells[i], buckets) for i in np.flatnonzero(labels != far)}
    far_cells = {cells[i] for i in np.flatnonzero(labels == far)}
    assert len(far_cells) == 1 and N.pairs_bucket(*far_cells.pop(), buckets) in near_buckets
    assert len({cells[i] for i in np.flatnonzero(labels != far)}) == 9 and len(near_buckets) < 9


@pytest.mark.parametrize("order", list(CK.serpentine_orders()))
def test_serpentine(order):
    points, radius = CK.cases()[f"serpentine_{order}"]
    n = len(points)
    assert n == 4096
    index = CK.serpentine_orders()[order]
    assert np.array_equal(np.sort(index), np.arange(n))
    offsets, partners, _ = S.pairs(points, radius)
    rows = np.repeat(np.arange(n), np.diff(offsets))
    where = np.empty(n, dtype=np.int64)                                             # the place on the path of every index
    where[index] = np.arange(n)
    assert len(partners) == 2 * (n - 1) and (np.abs(where[rows] - where[partners]) == 1).all()   # path neighbours only
    labels, sizes, roots = spec(f"serpentine_{order}")
    assert not labels.any() and sizes.tolist() == [n] and roots.tolist() == [0]


def test_serpentine_orders_differ():
    orders = CK.serpentine_orders()
    assert np.array_equal(orders["along"], np.arange(4096)) and orders["reversed"][0] == 4095
    assert orders["bit_reversed"][:4].tolist() == [0, 2048, 1024, 3072]
    assert len({o.tobytes() for o in orders.values()}) == 4


def test_lattice():
    points, radius = CK.cases()["lattice"]
    assert len(points) == 64 * 64 and np.array_equal(points[65], [radius, radius])  # raster order
    offsets, _, d2 = S.pairs(points, radius)
    assert offsets[-1] == 4 * 64 * 63 and (d2 == radius * radius).all()             # the four neighbours, at the radius
    labels, sizes, roots = spec("lattice")
    assert not labels.any() and sizes.tolist() == [4096] and roots.tolist() == [0]


def test_two_combs():
    points, radius, comb = CK.two_combs_parts()
    assert np.array_equal(points, CK.cases()["two_combs"][0])
    labels, sizes, roots = spec("two_combs")
    first = int(comb[0])                                                            # the comb of index 0 is cluster 0
    assert np.array_equal(labels, np.where(comb == first, 0, 1))
    closed = CK.two_combs_sizes()
    assert closed == (41 + 5 * 11, 41 + 5 * 10) and sizes.tolist() == [closed[first], closed[1 - first]]
    # the closest the combs come: one ulp of the upper spine's height above the radius
    a, b = points[comb == 0], points[comb == 1]
    dx, dy = a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1]
    gap = np.sqrt((dx * dx + dy * dy).min())
    assert 1.0 < gap <= 1.0 + 2 * np.spacing(CK.COMB_TEETH + 1.0)


def test_late_root():
    points, radius = CK.cases()["late_root"]
    labels, sizes, roots = spec("late_root")
    assert roots.tolist() == [0, 1, 2, 3, 4, 20] and sizes.tolist() == [5, 4, 4, 4, 4, 3]
    assert labels.tolist() == [0, 1, 2, 3, 4] * 4 + [5, 5, 5, 0]
    assert points[20:23, 0].max() < points[:20, 0].min()                            # leftmost, numbered last


def test_isolated():
    points, radius = CK.cases()["isolated"]
    n = len(points)
    assert S.pairs(points, radius)[0][-1] == 0
    labels, sizes, roots = spec("isolated")
    assert np.array_equal(labels, np.arange(n)) and (sizes == 1).all() and np.array_equal(roots, np.arange(n))


def test_piles():
    points, radius = CK.cases()["piles"]
    labels, sizes, roots = spec("piles")
    seen = []
    for at, count in (((0.2, 0.2), 65), ((0.8, 0.2), 257), ((0.2, 0.8), 300)):
        members = np.flatnonzero((points == at).all(axis=1))
        assert len(members) == count and len(set(labels[members].tolist())) == 1
        assert sizes[labels[members[0]]] >= count
        seen.append(int(labels[members[0]]))
    assert len(set(seen)) == 3 and len(sizes) > 20                                  # three clusters, and a cloud beside


def test_not_finite():
    points, radius = CK.cases()["not_finite"]
    labels, sizes, roots = spec("not_finite")
    bad = ~np.isfinite(points).all(axis=1)
    kinds = {(str(x), str(y)) for x, y in np.where(np.isfinite(points), 0.0, points)[bad]}
    assert {("nan", "0.0"), ("inf", "0.0"), ("-inf", "0.0"), ("0.0", "nan"), ("0.0", "inf"), ("0.0", "-inf")} <= kinds
    assert any("0.0" not in k for k in kinds) and bad.sum() == 92
    assert (labels[bad] == -1).all() and (labels[~bad] >= 0).all() and sizes.sum() == len(points) - 92
    n = CK.NOT_FINITE_CLOUD
    left, between, right = labels[n:n + 3], labels[n + 3:n + 5], labels[n + 5:n + 8]
    assert len(set(left.tolist())) == 1 and len(set(right.tolist())) == 1 and left[0] != right[0]
    assert between.tolist() == [-1, -1] and sizes[left[0]] == sizes[right[0]] == 3
    # with the points between made finite, each of them alone joins the two triples
    for k, value in ((n + 3, (points[n + 3, 0], 5.0)), (n + 4, (points[n + 3, 0], 5.0))):
        mended = points.copy()
        mended[k] = value
        joined = CS.clusters(mended, radius)[0]
        assert joined[n] == joined[n + 5] == joined[k]


def test_wide_is_wide():
    points, radius = CK.cases()["wide"]
    n = len(points)
    assert n == 70001 > 1 << 16 and n > 2 * N.PAIRS_SCAN_BLOCK and -(-n // N.PAIRS_BLOCK) == 274
    assert np.isfinite(points).all()


def test_components_at_the_size_of_wide():
    """The propagation stays usable at about 10^5 nodes: a lattice of 316 x 316 in raster order, and a path."""
    side = 316
    n = side * side
    k = np.arange(n)
    right, down = k[(k % side) < side - 1], k[k < n - side]
    rows = np.concatenate([right, down])
    order = np.argsort(rows, kind="stable")
    i, j = rows[order], np.concatenate([right + 1, down + side])[order]
    offsets = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))])
    labels, sizes, roots = CS.components(n, offsets, j)
    assert not labels.any() and sizes.tolist() == [n] and roots.tolist() == [0]
    path = np.random.RandomState(5).permutation(n)                                  # a path through all nodes, any order
    lo, hi = np.minimum(path[:-1], path[1:]), np.maximum(path[:-1], path[1:])
    order = np.argsort(lo, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(lo, minlength=n))])
    labels, sizes, roots = CS.components(n, offsets, hi[order])
    assert not labels.any() and sizes.tolist() == [n] and roots.tolist() == [0]
