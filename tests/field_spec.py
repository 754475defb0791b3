"""The rule of the device weighted sums (sc_pairs_sum_device, `Crate.field_tensors`), in NumPy.

Inputs: `points`, an (n, 2) float64 array, `radius`, finite and > 0, `values`, an (n, C) float64 array or None, `power` in
{0, 1, 2, 3}, `include_self`, and optionally `queries`, a (q, 2) float64 array.  The rows are the points themselves (the
self form, row r is point r) or the queries.  All arithmetic is float64, every operation rounded on its own -- that of
tests/pairs_spec.py and tests/nearest_spec.py for d2:

    dx = qx - x[j];  dy = qy - y[j];  d2 = dx*dx + dy*dy;  r2 = radius*radius
    j is a partner of row r  iff  d2 <= r2
        (self form with include_self false: and j != r; include_self true: point r is its own partner at d2 = 0, in its
         place in index order; with queries include_self has no meaning)
    t = 1 - d2 / r2                      (one division, one subtraction; 0 <= t <= 1 for a partner)
    w = 1 | t | t*t | (t*t)*t            for power 0 | 1 | 2 | 3   (power 0 computes no division)
    wsum[r]   = ((0.0 + w_j1) + w_j2) + ...                 the partners in ASCENDING j, left to right, from +0.0
    out[r, c] = ((0.0 + w_j1*v[j1,c]) + w_j2*v[j2,c]) + ... the same order; each product rounded, then each sum

A point with a coordinate that is not finite is nobody's partner, and a row whose own point or query is not finite has
out = 0 and wsum = 0 (d2 is then NaN or +inf next to a finite r2).  The values are taken as they are: a NaN or an infinity
propagates by IEEE rules, and 0 * inf at d2 == r2 is NaN.  The domain is that of the pair list, for the points and for the
queries: `in_domain`.  The sums are sequential -- np.cumsum adds left to right; np.sum and np.add.reduce add pairwise and
are not the rule.  Brute force in row blocks: fine up to a few thousand rows.
"""
import numpy as np

import pairs_spec

BLOCK = 512


def in_domain(points, radius, queries=None):
    return pairs_spec.in_domain(points, radius) and (queries is None or pairs_spec.in_domain(queries, radius))


def weights(d2, r2, power):
    """w of the squared distances `d2` (an array of partners' d2), each operation rounded on its own."""
    d2 = np.asarray(d2, dtype=np.float64)
    if power == 0:
        return np.ones_like(d2)
    t = np.float64(1.0) - d2 / r2
    if power == 1:
        return t
    tt = t * t
    return tt if power == 2 else tt * t


def sequential(terms):
    """((0.0 + terms[0]) + terms[1]) + ... along axis 0 -> the last partial sum; +0.0 for no terms."""
    terms = np.asarray(terms, dtype=np.float64)
    zero = np.zeros((1,) + terms.shape[1:], dtype=np.float64)
    return np.cumsum(np.concatenate([zero, terms], axis=0), axis=0)[-1]      # (cumsum adds left to right)


def partners_of(points, radius, include_self=True, queries=None):
    """-> per row (js ascending, d2 of each): the partners the sums run over."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    self_form = queries is None
    q = p if self_form else np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    radius = np.float64(radius)
    assert np.isfinite(radius) and radius > 0
    r2 = radius * radius
    x, y = p[:, 0], p[:, 1]
    index = np.arange(len(p))
    out = []
    with np.errstate(all="ignore"):
        for lo in range(0, len(q), BLOCK):
            hi = min(len(q), lo + BLOCK)
            dx = q[lo:hi, 0, None] - x[None, :]
            dy = q[lo:hi, 1, None] - y[None, :]
            d2 = dx * dx + dy * dy
            ok = d2 <= r2                                   # (NaN compares false)
            if self_form and not include_self:
                ok &= np.arange(lo, hi)[:, None] != index[None, :]
            for r in range(hi - lo):
                js = np.nonzero(ok[r])[0]                   # ascending
                out.append((js, d2[r, js]))
    return out


def field(points, radius, values=None, power=3, include_self=True, queries=None):
    """-> (out float64 (R, C), wsum float64 (R,)); C = 0 without values."""
    assert power in (0, 1, 2, 3)
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    v = np.zeros((len(p), 0)) if values is None else np.ascontiguousarray(values, dtype=np.float64)
    v = v[:, None] if v.ndim == 1 else v
    assert v.ndim == 2 and len(v) == len(p)
    radius = np.float64(radius)
    r2 = radius * radius
    rows = partners_of(p, radius, include_self, queries)
    out = np.zeros((len(rows), v.shape[1]), dtype=np.float64)
    wsum = np.zeros(len(rows), dtype=np.float64)
    with np.errstate(all="ignore"):
        for r, (js, d2) in enumerate(rows):
            w = weights(d2, r2, power)
            wsum[r] = sequential(w)
            out[r] = sequential(w[:, None] * v[js])
    return out, wsum
