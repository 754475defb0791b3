"""Every named case of tests/pairs_cases.py has the property it is named for -- proven from the rule (tests/pairs_spec.py)
and from the implementation's constants mirrored in `sand_crate_amd._native`.  No GPU."""
from fractions import Fraction

import numpy as np

import pairs_cases as K
import pairs_spec as S
from sand_crate_amd import _native as N


def rows(points, radius, half=False):
    offsets, partners, d2 = S.pairs(points, radius, half)
    return [partners[offsets[i]:offsets[i + 1]].tolist() for i in range(len(offsets) - 1)], d2


def test_every_case_is_inside_the_domain_and_small():
    for name, (pts, radius) in K.cases().items():
        assert pts.dtype == np.float64 and pts.shape == (len(pts), 2), name
        assert len(pts) <= 5000 or name == "three_passes", name           # (the one case that needs its size)
        assert S.in_domain(pts, radius), name


def test_edge_sizes_sit_on_the_launch_widths():
    sizes = K.edge_sizes()
    assert {0, 1, 2} <= set(sizes)
    for w in (64, N.PAIRS_BLOCK, N.PAIRS_SORT_TILE, N.PAIRS_SCAN_BLOCK):
        assert {w - 1, w, w + 1} <= set(sizes)
    assert N.pairs_buckets(128) == 256 and N.pairs_buckets(129) == 512       # the table doubles between two of them
    assert N.pairs_buckets(1024) == 2048 and N.pairs_buckets(1025) == 4096
    assert N.pairs_buckets(0) == N.PAIRS_MIN_BUCKETS
    # a size with several blocks of the scan over the tiles' digit counts (256 per tile) and of the 64-bit scan
    assert -(-max(sizes) // N.PAIRS_SORT_TILE) * 256 > 2 * N.PAIRS_SCAN_BLOCK and max(sizes) > 2 * N.PAIRS_SCAN_BLOCK
    for n in (65, 2049):
        pts, radius = K.cases()[f"n_{n}"]
        lengths = np.diff(S.pairs(pts, radius)[0])
        assert 3 < lengths.mean() < 9                       # ordinary rows: a handful of partners each


def test_exactly_at_the_radius():
    pts, radius = K.cases()["at_radius_3_4_5"]
    got, d2 = rows(pts, radius)
    assert got == [[1], [0]] and d2.tolist() == [25.0, 25.0]
    pts, radius = K.cases()["beyond_radius_3_4_5"]
    assert rows(pts, radius)[0] == [[], []]
    assert pts[1, 1] > 4.0 and 9.0 + pts[1, 1] * pts[1, 1] > 25.0
    # a radius whose square rounds: fl(0.1 * 0.1) is above the exact square of fl(0.1) ...
    r = np.float64(0.1)
    assert Fraction(float(r * r)) != Fraction(0.1) ** 2
    pts, radius = K.cases()["radius_0.1"]
    got, _ = rows(pts, radius)
    assert 1 in got[0] and 3 in got[0]                      # (0.1, 0) and (0, -0.1): d2 = fl(0.1 * 0.1), equal to r2
    assert (2 in got[0]) == bool(np.float64(0.06) ** 2 + np.float64(0.08) ** 2 <= r * r)
    assert 4 not in got[0] and 6 not in got[0]              # the diagonal, and one ulp beyond the radius
    assert (8 in got[7]) == bool((np.float64(0.4) - np.float64(0.5)) ** 2 <= r * r)


def test_lattices_sit_on_multiples_of_the_radius():
    for name in ("lattice_0.25", "lattice_0.01"):
        pts, radius = K.cases()[name]
        assert len(pts) == 49 and (pts < 0).any()
        assert any(x == 0 and np.signbit(x) for x in pts.ravel())       # -0.0
        k = np.arange(-3, 4)
        assert set(pts[:, 0].tolist()) == set((k * np.float64(radius)).tolist())
        got, _ = rows(pts, radius)
        centre = next(i for i, p in enumerate(pts) if p[0] == 0 and p[1] == 0)
        assert len(got[centre]) == 4                                      # the four at one radius; the diagonal is beyond


def test_eight_cells_and_none_two_away():
    pts, radius = K.cases()["eight_cells"]
    cells = K.cells_of(pts, radius)
    assert cells[0] == (0, 0)
    assert sorted(cells[1:9]) == sorted((dx, dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1) if (dx, dy) != (0, 0))
    assert all(max(abs(cx), abs(cy)) == 2 for cx, cy in cells[9:])
    got, _ = rows(pts, radius)
    assert got[0] == list(range(1, 9))
    assert not any(j >= 9 for row in got[:9] for j in row) and all(
        all(j >= 9 for j in row) for row in got[9:])       # the far ones are not partners of the near ones


def test_misplaced_floor():
    pts, radius = K.cases()["misplaced_floor"]
    r = np.float64(radius)
    wrong = [c for c in (0.03, 0.06) if int(np.floor(np.float64(c) / r)) != Fraction(c) // Fraction(radius)]
    assert wrong == [0.03, 0.06]
    for c in wrong:
        assert c in pts[:, 0] and c in pts[:, 1]
    # ... and the pairs of the rule reach across such a coordinate's cell border: (0.02, 0.03), ...
    got, _ = rows(pts, radius)
    index = {tuple(p): i for i, p in enumerate(pts.tolist())}
    assert index[(0.02, 0.0)] in got[index[(0.03, 0.0)]] and index[(0.03, 0.01)] in got[index[(0.03, 0.0)]]
    assert index[(0.07, 0.0)] in got[index[(0.06, 0.0)]] or index[(0.05, 0.0)] in got[index[(0.06, 0.0)]]
    # every pair of the rule lies within one computed cell, as the search needs it
    assert_pairs_within_one_cell(pts, radius)


def assert_pairs_within_one_cell(pts, radius):
    cells = K.cells_of(pts, radius)
    got, _ = rows(pts, radius)
    for i, row in enumerate(got):
        for j in row:
            assert abs(cells[i][0] - cells[j][0]) <= 1 and abs(cells[i][1] - cells[j][1]) <= 1


def test_large_cell_indices():
    pts, radius = K.cases()["large_cells"]
    cells = K.cells_of(pts, radius)
    assert min(abs(c) for cell in cells for c in cell) > 90000
    got, _ = rows(pts, radius)
    assert sum(len(r) for r in got) > len(pts)
    assert_pairs_within_one_cell(pts, radius)
    # the computed floor(c / radius) is not the true cell for some of them
    r = np.float64(radius)
    assert any(int(np.floor(np.float64(x) / r)) != Fraction(float(x)) // Fraction(radius) for x in pts[:, 0])


def test_bucket_sharing():
    pts, radius = K.cases()["bucket_sharing"]
    buckets = N.pairs_buckets(len(pts))
    assert buckets == N.PAIRS_MIN_BUCKETS
    (cx, cy), (a, b), far = K.shared_bucket_cells(buckets)
    assert a != b and max(abs(a[0] - cx), abs(a[1] - cy), abs(b[0] - cx), abs(b[1] - cy)) <= 1
    assert N.pairs_bucket(*a, buckets) == N.pairs_bucket(*b, buckets)
    assert N.pairs_bucket(*far, buckets) == N.pairs_bucket(cx, cy, buckets) and abs(far[0] - cx) > 1000
    cells = K.cells_of(pts, radius)
    for cell in (a, b, far, (cx, cy)):
        assert cell in cells                                 # all of them occupied
    assert cells.count(far) == 3
    got, _ = rows(pts, radius)
    centre = cells.index((cx, cy))
    assert len(got[centre]) == 8                             # each of the eight once, though two share a bucket
    for i, cell in enumerate(cells):
        if cell == far:
            assert len(got[i]) == 2 and all(cells[j] == far for j in got[i])


def test_hash_mirror_is_32_bit():
    assert N.pairs_bucket(-1, 0, 1 << 20) == N.pairs_bucket(0xFFFFFFFF, 0, 1 << 20)
    assert 0 <= N.pairs_bucket(-2 ** 31, 2 ** 31 - 1, 256) < 256
    assert N.PAIRS_CELL_FACTOR == 1.0 + 2.0 ** -20


def test_long_rows():
    pts, radius = K.cases()["long_rows"]
    lengths = np.diff(S.pairs(pts, radius)[0])
    for pile in (65, 257, 300):
        assert (lengths >= pile - 1).sum() >= pile
    assert lengths.max() > N.PAIRS_BLOCK and (lengths < 10).sum() > 100   # long rows beside ordinary ones
    # the row fed by all nine cells, its partners' indices interleaved over the cells
    h = float(K.cell_size(radius))
    centre = int(np.argmin(np.abs(pts - 100.5 * h).sum(axis=1)))
    cells = K.cells_of(pts, radius)
    got, _ = rows(pts, radius)
    row = got[centre]
    by_cell = [cells[j] for j in row]
    assert len(set(by_cell)) == 9 and len(row) == 9 * 12
    changes = sum(1 for a, b in zip(by_cell, by_cell[1:]) if a != b)
    assert changes > 50                                      # not nine runs one after another: a real merge


def test_non_finite_points():
    pts, radius = K.cases()["non_finite"]
    bad = ~np.isfinite(pts).all(axis=1)
    assert bad.sum() == 60 and np.isnan(pts).any() and (pts == np.inf).any() and (pts == -np.inf).any()
    assert (~np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 1])).any() and (np.isfinite(pts[:, 0]) & ~np.isfinite(pts[:, 1])).any()
    assert (~np.isfinite(pts)).all(axis=1).any()
    offsets, partners, _ = S.pairs(pts, radius)
    lengths = np.diff(offsets)
    assert not lengths[bad].any() and not bad[partners].any() and lengths[~bad].sum() > 500


def test_three_passes_of_the_binning_sort():
    pts, radius = K.cases()["three_passes"]
    n = len(pts)
    assert n == 16385 and N.pairs_buckets(n) == 65536 and N.pairs_buckets(n - 1) == 32768   # the smallest such n
    assert (65536).bit_length() == 17                        # the keys 0 .. 65536: two digits of eight bits do not hold them
    dead = ~np.isfinite(pts).all(axis=1)
    assert dead.sum() == 40 and not dead[-40:].all()         # dead points, and not where the sort would put them anyway
    live = {N.pairs_bucket(cx, cy, 65536) for cx, cy in K.cells_of(pts[~dead], radius)}
    assert len(live) > 256 and max(live) < 65536             # distinct first AND second digits; only a dead key has a third


def test_domain_rim_and_outside():
    pts, radius = K.cases()["domain_rim"]
    assert S.in_domain(pts, radius)
    cells = [c for cell in K.cells_of(pts, radius) for c in cell]
    # (a cell is a little larger than the radius: the outermost cell index is 2^31 / PAIRS_CELL_FACTOR, 2048 below 2^31)
    assert 2 ** 31 - 4096 < max(cells) < 2 ** 31 - 1 and -2 ** 31 + 1 < min(cells) < -2 ** 31 + 4096
    got, _ = rows(pts, radius)
    assert got[0] == [1] and got[1] == [0, 4] and got[2] == [3]
    pts, radius = K.outside_domain()
    assert not S.in_domain(pts, radius)
    assert abs(pts[33, 1]) / radius == 2.0 ** 31
    ok = pts.copy()
    ok[33, 1] = np.nextafter(ok[33, 1], 0)
    assert S.in_domain(ok, radius)
    assert S.in_domain(np.array([[np.inf, np.nan], [1.0, -np.inf]]), 1.0)   # only finite coordinates count


def test_big_pile_closed_form():
    n = K.BIG_PILE
    offsets = S.coincident_offsets(n)
    assert offsets[n] == 4294901760 > 2 ** 31 and 2 * offsets[n] > 2 ** 32 and offsets[3] == 3 * 65535
    assert S.coincident_partners(n, 0, 65535).tolist() == list(range(1, 65536))
    assert S.coincident_partners(n, 65535, 3).tolist() == [0, 2, 3]
    # the closed forms are the rule's, at a size the rule can be run at
    pts = np.tile([[0.25, -1.5]], (37, 1))
    for half in (False, True):
        o, p, d2 = S.pairs(pts, 0.01, half)
        assert np.array_equal(o, S.coincident_offsets(37, half)) and not d2.any()
        assert np.array_equal(p, S.coincident_partners(37, 0, len(p), half))
