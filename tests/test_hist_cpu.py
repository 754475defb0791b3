"""CPU-side checks of the distance histograms: the rule of tests/hist_spec.py against np.histogram row by row on every
case of tests/hist_cases.py, every claim the cases make, the host-side check of the edges (`_native.hist_squared_edges`,
what `Engine.pairs_hist` runs before the library is touched), and `shell_edges` / `radial_distribution` on a square
lattice whose g(r) is known in closed form.  No GPU."""
import functools

import numpy as np
import pytest

import hist_cases as HK
import hist_spec as HS
import pairs_spec as S
from sand_crate_amd import _native as N


@functools.lru_cache(maxsize=None)
def spec(name, query_form=False):
    case = HK.cases()[name]
    return HS.histogram(case.points, case.edges, HK.queries_of(case) if query_form else case.queries)


def bin_of(case, r, j):
    """The bin of point j in row r, by the rule, from a world of that row and that point alone."""
    rows = case.points if case.queries is None else case.queries
    table, _ = HS.histogram(case.points[[j]], case.edges, rows[[r]])
    assert table.sum() in (0, 1)
    return int(np.nonzero(table[0])[0][0]) if table.sum() else None


# ---- the rule against np.histogram

@pytest.mark.parametrize("name", sorted(HK.cases()))
@pytest.mark.parametrize("query_form", [False, True])
def test_the_rule_is_np_histogram_row_by_row(name, query_form):
    case = HK.cases()[name]
    queries = HK.queries_of(case) if query_form else case.queries
    table, total = spec(name, query_form)
    e2 = HS.squared_edges(case.edges)
    assert table.dtype == np.int32 and total.dtype == np.int64
    rows = len(case.points) if queries is None else len(queries)
    assert table.shape == (rows, len(e2) - 1) and total.shape == (len(e2) - 1,)
    assert HS.in_domain(case.points, case.edges, queries)
    for lo in range(0, rows, HS.BLOCK):
        d2 = HS.squared_distances(case.points, queries, lo, min(rows, lo + HS.BLOCK))
        for r, row in enumerate(d2, lo):
            row = row[np.isfinite(row)]                              # (np.histogram refuses NaN; the self entry is NaN here)
            assert np.array_equal(np.histogram(row, bins=e2)[0], table[r]), r
    assert np.array_equal(total, table.astype(np.int64).sum(axis=0))


def test_the_cases_cover_what_they_are_named_for():
    cases = HK.cases()
    assert {len(cases[f"bins_{b}"].edges) - 1 for b in HK.BINS} == set(HK.BINS)
    for slots in N.HIST_SLOTS:                                        # one below, at and above every LDS size but the last
        assert {slots - 1, slots} <= set(HK.BINS) and (slots == N.HIST_MAX_BINS or slots + 1 in HK.BINS)
    assert {N.hist_slots(b) for b in HK.BINS} == set(N.HIST_SLOTS)
    for n in HK.ROWS:
        assert len(cases[f"rows_{n}"].points) == n and len(cases[f"queries_{n}"].queries) == n
    assert {N.HIST_BLOCK - 1, N.HIST_BLOCK, N.HIST_BLOCK + 1, 2 * N.HIST_BLOCK, 2 * N.HIST_BLOCK + 1} <= set(HK.ROWS)
    assert len(cases["rows_0"].points) == 0 and len(cases["queries_0"].queries) == 0
    assert HK.WIDE - 1 > 2 ** 8 and HK.WIDE - 1 > 2 ** 12
    assert spec("wide_counter")[0].max() == HK.WIDE - 1 > np.iinfo(np.uint8).max
    assert int(HK.coincident_total(HK.BEYOND_32_BITS)[0]) == 4_355_934_000 > 2 ** 32
    assert int(HK.coincident_total(70000)[0]) > 2 ** 32 > int(HK.coincident_total(65000)[0])
    outside = HK.outside()
    assert HS.in_domain(outside.points, outside.edges) and not HS.in_domain(outside.points, outside.edges, outside.queries)
    far = cases["far_cells"].points
    assert (far[:70, 0] < 0).all() and (far[70:, 1] < -9e5).all()


# ---- every claim

CLAIMED = [(name, kind) for name, case in sorted(HK.cases().items()) for kind in sorted(case.claims)]


@pytest.mark.parametrize("name,kind", CLAIMED)
def test_claim(name, kind):
    case = HK.cases()[name]
    claim = case.claims[kind]
    table, total = spec(name)
    e2 = HS.squared_edges(case.edges)
    if kind == "pair_bin":
        for (r, j), b in claim.items():
            assert bin_of(case, r, j) == b, (r, j)
    elif kind == "on_edge":
        d2 = HS.squared_distances(case.points, case.queries)
        for r, j, k in claim:
            assert d2[r, j] == e2[k], (r, j, k)
            want = min(k, len(e2) - 2)                               # at e2[b]: bin b, not b - 1; at e2[B]: the last bin
            assert bin_of(case, r, j) == want
    elif kind == "total":
        assert total.tolist() == list(claim)
    elif kind == "row":
        for r, want in claim.items():
            assert table[r].tolist() == want, r
    elif kind == "nothing_lost":
        offsets, _, _ = S.pairs(case.points, case.edges[-1])
        assert np.array_equal(table.sum(axis=1), np.diff(offsets)) and total.sum() == offsets[-1] > 0
    elif kind == "mean_partners":
        lo, hi = claim
        assert lo <= table.sum(axis=1).mean() <= hi
    elif kind == "zero_rows":
        assert len(claim) and not table[claim].any() and table.any() == (len(case.points) > 0)
    elif kind == "absent":
        keep = np.setdiff1d(np.arange(len(case.points)), claim)
        without, _ = HS.histogram(case.points[keep], case.edges, case.queries)
        assert np.array_equal(without, table[keep] if case.queries is None else table)
        assert not np.isfinite(case.points[claim]).all(axis=1).any()
    elif kind == "shared_bucket":
        h = np.float64(case.edges[-1]) * N.PAIRS_CELL_FACTOR
        cells = {(int(np.floor(x / h)), int(np.floor(y / h))) for x, y in case.points}
        buckets = N.pairs_buckets(len(case.points))
        assert len({N.pairs_bucket(cx, cy, buckets) for cx, cy in cells}) < len(cells)
        assert min(cx for cx, _ in cells) < 0 and min(cy for _, cy in cells) < -(2 ** 20)
    elif kind == "differs_from":
        assert not np.array_equal(table, spec(claim)[0])
    else:
        raise AssertionError(f"unknown claim {kind}")


def test_one_ulp_either_side_of_an_edge():
    """d2 = 2.25 exactly.  The edge 1.5 squares to 2.25: the partner is AT the edge and belongs to the bin above it.
    One ulp up the square is above 2.25 -- asserted, not assumed -- and the partner falls below the edge; one ulp down
    it is below and the partner stays above.  A search on d = 1.5 instead of d2, or an edge squared in other
    arithmetic, gives another answer in one of the three."""
    at, above, below = (HK.cases()[n] for n in ("ulp_at", "ulp_above", "ulp_below"))
    d2 = HS.squared_distances(at.points)[0, 1]
    assert d2 == 2.25
    e_at, e_above, e_below = (HS.squared_edges(c.edges)[1] for c in (at, above, below))
    assert e_below < e_at == d2 < e_above and len({e_at, e_above, e_below}) == 3
    assert [spec(n)[0].tolist() for n in ("ulp_at", "ulp_above", "ulp_below")] == [[[0, 1]] * 2, [[1, 0]] * 2, [[0, 1]] * 2]
    # on the distances themselves the three edges are three different numbers around d = 1.5: below, at and above
    assert below.edges[1] < 1.5 == at.edges[1] < above.edges[1]


def test_the_closed_form_of_coincident_points():
    table, total = spec("coincident_300")
    assert np.array_equal(total, HK.coincident_total(300)) and (table == 299).all()
    assert np.array_equal(spec("wide_counter")[1], HK.coincident_total(HK.WIDE))


# ---- the host-side check of the edges

def test_squared_edges_are_numpy_float64_squares():
    e = HK.cases()["bins_33"].edges
    e2 = N.hist_squared_edges(e)
    assert e2.dtype == np.float64 and np.array_equal(e2, e * e) and np.array_equal(e2, HS.squared_edges(e))
    assert np.array_equal(N.hist_squared_edges(list(e)), e2)          # a sequence serves
    assert np.array_equal(N.hist_squared_edges(e.astype(np.float32)), e.astype(np.float32).astype(np.float64) ** 2)
    assert len(N.hist_squared_edges(np.linspace(0, 1, 65))) == 65 and len(N.hist_squared_edges([0.0, 1.0])) == 2


@pytest.mark.parametrize("edges", [
    [0.0, 0.2, 0.1], [0.0, 0.1, 0.1],                                 # not ascending
    [1.0, 1.0, 2.0], [0.0, 0.0],                                      # equal
    [3e-200, 4e-200, 1.0],                                            # squares that collapse: both 0
    [1e200, 2e200],                                                   # ... or overflow
    [-0.1, 0.1], [-0.0 - 1e-300, 1.0],                                # negative
    [0.0, np.nan], [0.0, np.inf], [np.nan, 1.0],
    [0.5], [], np.linspace(0, 1, 66),                                 # B = 0, no edges, B = 65
    np.zeros((2, 2)), 1.0])
def test_bad_edges_are_refused(edges):
    with pytest.raises(ValueError):
        N.hist_squared_edges(edges)


def test_squares_that_collapse_one_ulp_apart():
    a = 1.0 + 2.0 ** -30
    b = np.nextafter(a, 2.0)
    lo, hi = np.float64(a) * np.float64(a), np.float64(b) * np.float64(b)
    if lo == hi:                                                      # (two neighbours may or may not square apart)
        with pytest.raises(ValueError):
            N.hist_squared_edges([0.0, a, b])
    small = [0.0, 1e-170, 2e-170]                                     # ascending distances, squares 0, 0, 0
    assert small[1] < small[2] and small[1] * small[1] == 0.0
    with pytest.raises(ValueError, match="squares"):
        N.hist_squared_edges(small)


def test_hist_slots():
    assert [N.hist_slots(b) for b in (1, 16, 17, 32, 33, 64)] == [16, 16, 32, 32, 64, 64]
    for bad in (0, 65, -1):
        with pytest.raises(ValueError):
            N.hist_slots(bad)


# ---- shell_edges and radial_distribution

def test_shell_edges():
    from sand_crate_amd import pairs
    e = pairs.shell_edges(0.5, 4)
    assert e.dtype == np.float64 and e.tolist() == [0.0, 0.125, 0.25, 0.375, 0.5]
    e = pairs.shell_edges(0.3, 7, inner=0.1)
    assert len(e) == 8 and e[0] == 0.1 and e[-1] == 0.3 and np.allclose(np.diff(e), 0.2 / 7, rtol=1e-12)
    assert len(N.hist_squared_edges(pairs.shell_edges(0.037, 64))) == 65
    for bad in (lambda: pairs.shell_edges(0.5, 0), lambda: pairs.shell_edges(0.5, 3, inner=0.5),
                lambda: pairs.shell_edges(0.5, 3, inner=-0.1), lambda: pairs.shell_edges(np.inf, 3)):
        with pytest.raises(ValueError):
            bad()


def test_radial_distribution_of_a_square_lattice():
    """A periodic square lattice of spacing a, n points on the area n a^2: every point has 4 partners at a, 4 at a sqrt 2,
    4 at 2a, 8 at a sqrt 5.  With edges halfway between those shells, total[b] = n m_b and so
    g[b] = m_b a^2 / (pi (e[b+1]^2 - e[b]^2)), in closed form -- and 0 in the empty first bin."""
    import torch
    from sand_crate_amd import pairs
    a, side = 0.125, 12
    n = side * side
    k = np.arange(side) * a
    pts = np.stack([np.tile(k, side), np.repeat(k, side)], axis=1)
    images = np.concatenate([pts + np.array([ox, oy]) * side * a for ox in (-1, 0, 1) for oy in (-1, 0, 1)])
    edges = a * np.array([0.0, 0.5, 1.2, 1.7, 2.1, 2.5])
    table, total = HS.histogram(images, edges, pts)                   # every point of the cell looks at the periodic images
    total = total - np.array([n, 0, 0, 0, 0])                         # ... of which one is the point itself, at d2 = 0
    shells = np.array([0, 4, 4, 4, 8])
    assert np.array_equal(total, n * shells)
    g = pairs.radial_distribution(torch.from_numpy(total), edges, n, n * a * a)
    want = shells * a * a / (np.pi * (edges[1:] ** 2 - edges[:-1] ** 2))
    assert g.dtype == torch.float64 and g.shape == (5,) and g[0] == 0
    assert np.allclose(g.numpy(), want, rtol=1e-14, atol=0)
    assert abs(float(g[1]) - 4 / (np.pi * (1.2 ** 2 - 0.5 ** 2))) < 1e-12
    with pytest.raises(ValueError):
        pairs.radial_distribution(torch.from_numpy(total), edges[:-1], n, 1.0)
    assert "ordered pairs" in pairs.radial_distribution.__doc__.lower().replace("\n", " ")
