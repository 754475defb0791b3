"""The rule of the device distance histograms (sc_pairs_hist_device, `Crate.distance_histogram`), in NumPy.

Inputs: `points`, an (n, 2) float64 array, `edges`, B + 1 float64 distances, B = 1 .. 64, with 0 <= edges[0] < edges[1] <
... < edges[B], and optionally `queries`, a (q, 2) float64 array.  The rows are the points themselves (the self form, row r
is point r) or the queries.  All arithmetic is float64, every operation rounded on its own -- that of tests/pairs_spec.py
for d2:

    e2[k] = edges[k]*edges[k]            computed once; the squares must still be strictly ascending (`squared_edges`)
    dx = qx - x[j];  dy = qy - y[j];  d2 = dx*dx + dy*dy
    j is a partner of row r  iff  d2 <= e2[B]      (self form: and j != r -- there is no include_self: a point's distance
                                                    to itself is not a distance)
    a partner is in bin b    iff  e2[b] <= d2 < e2[b+1]      for b < B - 1
                                  e2[B-1] <= d2 <= e2[B]     for the last bin: closed on top
    a partner with d2 < e2[0] is in no bin; coincident distinct points have d2 = 0 and are in bin 0 iff edges[0] == 0
    table[r, b] = the number of partners of row r in bin b                       (int32)
    total[b]    = sum over the rows of table[r, b]                               (int64; the self form counts ordered
                                                                                  pairs, each unordered pair twice)

No square root is taken anywhere: the squares are compared.  A point with a coordinate that is not finite is nobody's
partner, and a row whose own point or query is not finite is all zero (d2 is then NaN or +inf next to finite edges).  The
domain is that of the pair list at radius = edges[B], for the points and for the queries: `in_domain`.  This is what
np.histogram(d2, bins=e2) does with a row's d2; the rule below is written with the compares themselves, and
tests/test_hist_cpu.py holds the two against each other.  Brute force in row blocks: fine up to a few thousand rows.
"""
import numpy as np

import pairs_spec

MAX_BINS = 64
BLOCK = 512


def squared_edges(edges):
    """-> e2, float64 (B + 1,); asserts what the call demands of the edges."""
    e = np.array(edges, dtype=np.float64)
    assert e.ndim == 1 and 1 <= len(e) - 1 <= MAX_BINS
    assert np.isfinite(e).all() and e[0] >= 0 and (e[1:] > e[:-1]).all()
    e2 = e * e
    assert np.isfinite(e2).all() and (e2[1:] > e2[:-1]).all()
    return e2


def in_domain(points, edges, queries=None):
    radius = np.float64(np.asarray(edges, dtype=np.float64)[-1])
    return pairs_spec.in_domain(points, radius) and (queries is None or pairs_spec.in_domain(queries, radius))


def squared_distances(points, queries=None, lo=0, hi=None):
    """-> d2 of the rows lo .. hi against every point, (hi - lo, n); the self form's own entry is set to NaN (no bin)."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    self_form = queries is None
    q = p if self_form else np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    hi = len(q) if hi is None else hi
    with np.errstate(all="ignore"):
        dx = q[lo:hi, 0, None] - p[None, :, 0]
        dy = q[lo:hi, 1, None] - p[None, :, 1]
        d2 = dx * dx + dy * dy
    if self_form:
        r = np.arange(lo, hi)
        d2[r - lo, r] = np.nan
    return d2


def histogram(points, edges, queries=None):
    """-> (table int32 (R, B), total int64 (B,))."""
    e2 = squared_edges(edges)
    bins = len(e2) - 1
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    rows = len(p) if queries is None else len(np.asarray(queries, dtype=np.float64).reshape(-1, 2))
    table = np.zeros((rows, bins), dtype=np.int32)
    for lo in range(0, rows, BLOCK):
        hi = min(rows, lo + BLOCK)
        d2 = squared_distances(p, queries, lo, hi)
        with np.errstate(invalid="ignore"):
            for b in range(bins):
                below = d2 <= e2[b + 1] if b == bins - 1 else d2 < e2[b + 1]
                table[lo:hi, b] = ((e2[b] <= d2) & below).sum(axis=1)          # (NaN compares false)
    return table, table.astype(np.int64).sum(axis=0)
