"""The named inputs of the distance histograms' tests: name -> Case(points (n, 2), edges (B + 1,), queries (q, 2) or None,
claims).  Worlds of the smallest size at which the kernel can go wrong.  `claims` says what the world is there for, in
terms tests/test_hist_cpu.py proves from tests/hist_spec.py; tests/test_gpu_hist.py runs each on the device against the
spec, in the self form and -- with `queries_of` -- in the query form.  The kinds of claim:

    "pair_bin"      {(r, j): b or None}: point j falls into bin b of row r, None: into no bin
    "on_edge"       [(r, j, k)]: d2 of row r and point j is EXACTLY e2[k]
    "total"         the totals of the self form, worked out by hand
    "row"           {r: [counts]}: whole rows of the self form, worked out by hand
    "nothing_lost"  every pair of the pair list at radius edges[B] is in some bin
    "mean_partners" (lo, hi): the mean over the rows of a row's sum
    "zero_rows"     rows (of the self form, or of the queries when the case has them) that are all zero
    "absent"        points that are in nobody's row: without them the other rows are the same
    "shared_bucket" two distinct occupied cells of the count's grid lie in one bucket of its hashed table
    "differs_from"  another case whose table is not this one's
"""
import collections
import functools

import numpy as np

from sand_crate_amd import _native as N

Case = collections.namedtuple("Case", "points edges queries claims")

BINS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)                  # around every LDS size of the kernel (N.HIST_SLOTS)
ROWS = (1, 63, 64, 65, 128, 129)                               # around a workgroup's 64 rows (N.HIST_BLOCK)
OUTSIDE = "query_outside_domain"
WIDE = 5000                                                    # partners of one row in one bin: beyond 8 and 16 bits
BEYOND_32_BITS = 66000                                         # coincident points whose total in bin 0 passes 2^32
NAN, INF = float("nan"), float("inf")
assert max(N.HIST_SLOTS) == N.HIST_MAX_BINS == 64 and N.HIST_BLOCK == 64


def cloud(seed, n, partners=12.0, of=None):
    """n uniform points in the unit square and the radius at which one of `of` (default n) such points has about
    `partners` partners."""
    rs = np.random.RandomState(seed)
    return rs.rand(n, 2), float(np.sqrt(partners / (np.pi * max(of or n, 1))))


def lattice():
    """6 x 6 points of spacing 0.125 from (-0.25, -0.25): every coordinate, difference and d2 is a dyadic rational."""
    k = np.arange(6) * 0.125 - 0.25
    return np.stack([np.tile(k, 6), np.repeat(k, 6)], axis=1)      # point 6 iy + ix


def coincident(n, at=(0.25, 0.75)):
    return np.tile(np.array(at, dtype=np.float64), (n, 1))


def coincident_total(n):
    """The totals of n coincident points with edges [0, anything]: every row has the n - 1 others in bin 0."""
    return np.array([n * (n - 1)], dtype=np.int64)


def queries_of(case):
    """The queries of the query form: the case's own, or its points -- every one then lies on a point, at d2 = 0."""
    return case.points if case.queries is None else case.queries


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    # -- edges hit exactly
    pts = lattice()
    e = np.arange(5) * 0.125                                       # 0, .125, .25, .375, .5
    out["lattice_edges_hit"] = Case(pts, e, None, dict(
        on_edge=[(0, 1, 1), (0, 2, 2), (0, 3, 3), (0, 4, 4), (0, 24, 4)],
        pair_bin={(0, 1): 1, (0, 2): 2, (0, 3): 3, (0, 4): 3, (0, 24): 3, (0, 6): 1, (0, 7): 1, (0, 5): None},
        row={0: [0, 3, 5, 8]}))   # d2 / 0.125^2 of the others: 1 1 2 | 4 4 5 5 8 | 9 9 10 10 13 13 16 16; 17 .. are out
    inner = np.array([0.125, 0.25, 0.375])
    out["lattice_inner_edge"] = Case(pts, inner, None, dict(
        on_edge=[(0, 1, 0), (7, 8, 0)], pair_bin={(0, 1): 0, (0, 6): 0, (7, 8): 0, (7, 1): 0, (0, 3): 1, (0, 4): None},
        nothing_lost=True, row={0: [3, 7]}))                       # 1 1 2 | 4 4 5 5 8 9 9
    # -- one ulp either side: d2 = 2.25 exactly; the edge's square is 2.25, above it, below it
    two = np.array([[0.0, 0.0], [1.5, 0.0]])
    x = 1.5
    out["ulp_at"] = Case(two, np.array([0.0, x, 2.0]), None, dict(on_edge=[(0, 1, 1)], pair_bin={(0, 1): 1, (1, 0): 1}))
    out["ulp_above"] = Case(two, np.array([0.0, np.nextafter(x, 2.0), 2.0]), None,
                            dict(pair_bin={(0, 1): 0, (1, 0): 0}, differs_from="ulp_at"))
    out["ulp_below"] = Case(two, np.array([0.0, np.nextafter(x, 0.0), 2.0]), None,
                            dict(pair_bin={(0, 1): 1, (1, 0): 1}, differs_from="ulp_above"))
    # -- below the first edge, and coincident points
    four = np.array([[0.5, 0.5], [0.5, 0.5], [0.5, 0.5], [0.5, 0.8]])            # three at one place, one 0.3 away
    out["coincident_from_0"] = Case(four, np.array([0.0, 0.2, 0.4]), None, dict(
        pair_bin={(0, 1): 0, (0, 2): 0, (1, 0): 0, (0, 3): 1, (3, 0): 1}, total=[6, 6], row={0: [2, 1], 3: [0, 3]}))
    out["coincident_from_0.1"] = Case(four, np.array([0.1, 0.2, 0.4]), None, dict(
        pair_bin={(0, 1): None, (0, 2): None, (1, 0): None, (0, 3): 1, (3, 0): 1}, total=[0, 6], row={0: [0, 1], 3: [0, 3]}))
    # -- every bin count at which the kernel or its LDS changes
    pts, radius = cloud(11, 300)
    for bins in BINS:
        out[f"bins_{bins}"] = Case(pts, np.linspace(0.0, radius, bins + 1), None, dict(mean_partners=(9.0, 13.0)))
    # -- row counts at the workgroup's edge, for points and for queries
    rs = np.random.RandomState(12)
    base, _ = cloud(13, 200)
    for n in ROWS:
        pts, radius = cloud(100 + n, n, 9.0)
        out[f"rows_{n}"] = Case(pts, np.linspace(0.0, radius, 6), None, {})
        out[f"queries_{n}"] = Case(base, np.linspace(0.0, 0.12, 6), rs.rand(n, 2), {})
    out["rows_0"] = Case(np.zeros((0, 2)), np.array([0.0, 0.1, 0.2]), None, {})
    out["queries_0"] = Case(base, np.array([0.0, 0.1, 0.2]), np.zeros((0, 2)), {})
    out["queries_of_nothing"] = Case(np.zeros((0, 2)), np.array([0.0, 0.1, 0.2]), rs.rand(5, 2), dict(zero_rows=list(range(5))))
    # -- not finite: such rows are zero, such points in nobody's row
    pts, radius = cloud(14, 90, 14.0)
    pts = pts.copy()
    bad = {3: (NAN, 0.5), 17: (0.5, NAN), 29: (INF, 0.5), 41: (0.5, -INF), 53: (NAN, NAN), 64: (INF, -INF), 77: (-INF, NAN)}
    for r, p in bad.items():
        pts[r] = p
    e = np.linspace(0.0, radius, 8)
    out["non_finite_points"] = Case(pts, e, None, dict(zero_rows=sorted(bad), absent=sorted(bad)))
    good, _ = cloud(14, 90, 14.0)
    qs = np.concatenate([np.array(list(bad.values())), good[:9] + 0.01])
    out["non_finite_queries"] = Case(pts, e, qs, dict(zero_rows=list(range(len(bad))), absent=sorted(bad)))
    # -- negative coordinates and far cells: the signed cell conversion, distinct cells in one bucket
    rs = np.random.RandomState(15)
    far = np.concatenate([np.array([-3.7, 2.1]) + 0.12 * rs.randn(70, 2), np.array([1e6, -1e6]) + 0.12 * rs.randn(70, 2)])
    out["far_cells"] = Case(far, np.linspace(0.0, 0.05, 5), None, dict(shared_bucket=True, mean_partners=(1.0, 8.0)))
    out["far_cells_queries"] = Case(far, np.linspace(0.01, 0.05, 4), far[::3] + 0.004, {})
    # -- a wide counter
    out["wide_counter"] = Case(coincident(WIDE), np.array([0.0, 0.1]), None,
                               dict(total=coincident_total(WIDE).tolist(), row={0: [WIDE - 1], WIDE - 1: [WIDE - 1]}))
    # -- the closed form of coincident points, proved here where the spec still runs
    out["coincident_300"] = Case(coincident(300), np.array([0.0, 0.1]), None, dict(total=coincident_total(300).tolist()))
    return out


def outside():
    """One query at 1e300: the status is -1 and nothing is written."""
    pts, radius = cloud(16, 50)
    return Case(pts, np.linspace(0.0, radius, 4), np.array([[0.5, 0.5], [1e300, 0.5], [0.25, 0.25]]), {})
