"""The rule of the device nearest-k tables (sc_pairs_nearest_device, `Crate.neighbor_tensors`), in NumPy.

Inputs: `points`, an (n, 2) float64 array, `radius`, finite and > 0, `k` >= 1 and optionally `queries`, a (q, 2) float64
array.  The rows are the points themselves (the self form, row r is point r) or the queries.  All arithmetic is float64,
every operation rounded on its own -- exactly that of tests/pairs_spec.py:

    dx = qx - x[j];  dy = qy - y[j];  d2 = dx*dx + dy*dy
    j is a partner of row r  iff  d2 <= radius*radius  (and, in the self form only, j != r)

`partners[r]` is the number of partners, without any cap: in the self form the row length of the full pair list.
`neighbors[r, 0 .. min(k, partners[r]))` are the partners in ascending order of the key (d2, j): d2 compared as the float64
that was computed, bit-equal d2 ordered by the smaller j; `d2[r, s]` is the very number that was compared.  The places
behind hold -1 and +inf.  A point with a coordinate that is not finite is nobody's partner, and a row whose own point or
query is not finite is empty (d2 is then NaN or +inf next to a finite radius*radius).  A query that coincides with a point
has it as a partner at d2 = 0.  The domain: every FINITE coordinate c of the points and of the queries satisfies
|c| / radius < 2^31 (the rounded float64 quotient); `in_domain` says whether.  Brute force in row blocks: fine up to a few
thousand rows.
"""
import numpy as np

import pairs_spec

BLOCK = 512


def in_domain(points, radius, queries=None):
    return pairs_spec.in_domain(points, radius) and (queries is None or pairs_spec.in_domain(queries, radius))


def nearest(points, radius, k, queries=None):
    """-> (neighbors int64 (R, k), d2 float64 (R, k), partners int64 (R,))"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    self_form = queries is None
    q = p if self_form else np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    k = int(k)
    assert k >= 1
    radius = np.float64(radius)
    assert np.isfinite(radius) and radius > 0
    r2 = radius * radius
    n, rows = len(p), len(q)
    x, y = p[:, 0], p[:, 1]
    neighbors = np.full((rows, k), -1, dtype=np.int64)
    d2_out = np.full((rows, k), np.inf, dtype=np.float64)
    partners = np.zeros(rows, dtype=np.int64)
    index = np.arange(n)
    with np.errstate(all="ignore"):
        for lo in range(0, rows, BLOCK):
            hi = min(rows, lo + BLOCK)
            dx = q[lo:hi, 0, None] - x[None, :]
            dy = q[lo:hi, 1, None] - y[None, :]
            d2 = dx * dx + dy * dy
            ok = d2 <= r2                                   # (NaN compares false)
            if self_form:
                ok &= np.arange(lo, hi)[:, None] != index[None, :]
            partners[lo:hi] = ok.sum(axis=1)
            for r in range(lo, hi):
                js = np.nonzero(ok[r - lo])[0]
                ds = d2[r - lo, js]
                order = np.lexsort((js, ds))[:k]            # by d2, then by j
                neighbors[r, :len(order)] = js[order]
                d2_out[r, :len(order)] = ds[order]
    return neighbors, d2_out, partners
