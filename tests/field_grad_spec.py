"""The rule of the gradients of the device weighted sums (`Crate.field_function`, sc_pairs_sum_grad_device), in NumPy.

The forward is `field_spec.field`: sums[r, c] = sum_j w_rj v[j, c], wsum[r] = sum_j w_rj, w = t^power, t = 1 - d2 / r2.
Given the upstream gradients `G` (rows x C, of sums) and `gw` (rows, of wsum), either of which may be None:

The gradient with respect to the VALUES is `field_spec.field` itself, rows and partners swapped -- w depends on d2 only,
and d2 = fl(fl(dx dx) + fl(dy dy)) has the same bits from either end: `values_grad`.  gw does not enter.

The gradient with respect to POSITIONS is `position_grad`, all float64, every operation rounded on its own:

    j is a partner of row r  iff  d2 <= r2   (dx = qx - x[j], dy = qy - y[j], d2 = dx*dx + dy*dy, r2 = radius*radius: the
                                              arithmetic of pairs_spec), and in the self form j != r ALWAYS
                                              (d(d2_rr)/dx is identically 0; include_self plays no part)
    t = 1 - d2 / r2;   m = 1 | t | t*t   for power 1 | 2 | 3     (t^(power-1); power 0: the result is +0.0, nothing runs)
    s = (((0.0 + row_s[r]) + part_s[j]) + row_a[r,0]*part_b[j,0]) + row_a[r,1]*part_b[j,1] + ...
                                              left to right, each product and each sum rounded; an absent row_s or
                                              part_s adds nothing (not even a zero)
    ax = ((0.0 + (s*m)*dx_j1) + (s*m)*dx_j2) + ...    ay likewise;    partners in ASCENDING j
    out[r] = (k*ax, k*ay),  k = -(2*power) / r2       (one multiplication per component, at the end)

A row whose own point is not finite has no partners, so ax = ay = +0.0 and out[r] = (k*0.0, k*0.0): a zero (with the sign
of k, as for any row without partners).  A point that is not finite is nobody's partner.  row_a, part_b, row_s and part_s
are taken as they are: NaN and infinity propagate by IEEE rules.

The three uses of the one rule, V the values (`self_points_grad`, `query_queries_grad`, `query_points_grad`):

    self form, w.r.t. points      rows = points,  grid over points   row_a = [G | V]  part_b = [V | G]  row_s = part_s = gw
    query form, w.r.t. queries    rows = queries, grid over points   row_a = G        part_b = V        row_s = gw
    query form, w.r.t. points     rows = points,  grid over queries  row_a = V        part_b = G        part_s = gw

More than 8 channels go in groups of 8, one launch each, the scalars with the first group, and the (R, 2) results are
added in ascending group order: `position_grad_chunked`.  Brute force: fine up to a few thousand rows.
"""
import numpy as np

import field_spec
import pairs_spec  # noqa: F401  (the arithmetic of d2 and the domain are its)

GROUP = 8


def _two_dimensional(a, rows):
    if a is None:
        return np.zeros((rows, 0))
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a[:, None] if a.ndim == 1 else a


def position_grad(rows_xy, points, radius, power, row_a=None, part_b=None, row_s=None, part_s=None, self_form=False):
    """-> float64 (R, 2).  `self_form`: the rows ARE the points (rows_xy is ignored) and j != r."""
    assert power in (0, 1, 2, 3)
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    q = p if self_form else np.ascontiguousarray(rows_xy, dtype=np.float64).reshape(-1, 2)
    out = np.zeros((len(q), 2), dtype=np.float64)
    if power == 0:
        return out
    a, b = _two_dimensional(row_a, len(q)), _two_dimensional(part_b, len(p))
    assert a.shape[1] == b.shape[1] and len(a) >= len(q) and len(b) >= len(p)
    radius = np.float64(radius)
    r2 = radius * radius
    k = -np.float64(2 * power) / r2
    partners = field_spec.partners_of(p, radius, False, None if self_form else q)
    with np.errstate(all="ignore"):
        for r, (js, d2) in enumerate(partners):
            dx, dy = q[r, 0] - p[js, 0], q[r, 1] - p[js, 1]
            s = np.zeros(len(js), dtype=np.float64)
            if row_s is not None:
                s = s + np.float64(row_s[r])
            if part_s is not None:
                s = s + np.asarray(part_s, dtype=np.float64)[js]
            for c in range(a.shape[1]):
                s = s + a[r, c] * b[js, c]
            if power > 1:
                t = np.float64(1.0) - d2 / r2
                s = s * (t if power == 2 else t * t)
            out[r, 0] = k * field_spec.sequential(s * dx)
            out[r, 1] = k * field_spec.sequential(s * dy)
    return out


def position_grad_chunked(rows_xy, points, radius, power, row_a=None, part_b=None, row_s=None, part_s=None, self_form=False,
                          group=GROUP):
    """`position_grad` as the wrapper launches it: `group` channels per launch, the scalars with the first, the results
    added in ascending group order."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    rows = len(p) if self_form else len(np.asarray(rows_xy).reshape(-1, 2))
    a, b = _two_dimensional(row_a, rows), _two_dimensional(part_b, len(p))
    total = None
    for at in range(0, max(a.shape[1], 1), group):
        part = position_grad(rows_xy, p, radius, power, a[:, at:at + group], b[:, at:at + group],
                             row_s if at == 0 else None, part_s if at == 0 else None, self_form)
        with np.errstate(all="ignore"):
            total = part if total is None else total + part
    return total


def values_grad(points, radius, G, power, include_self=True, queries=None):
    """-> float64 (n, C): the gradient of sum(G * sums) with respect to the values -- `field` with the roles swapped; in
    the query form one row per point, summed over the queries in ascending query index."""
    if queries is None:
        return field_spec.field(points, radius, G, power, include_self)[0]
    return field_spec.field(queries, radius, G, power, True, points)[0]


def _pair(left, right):
    """[left | right] -- or nothing, when either is absent (then s has no dot product)."""
    if left is None or right is None:
        return None
    return np.concatenate([_two_dimensional(left, len(left)), _two_dimensional(right, len(right))], axis=1)


def self_points_grad(points, radius, values, power, G=None, gw=None):
    """The self form with respect to the points: s = gw[r] + gw[j] + G_r . V_j + V_r . G_j."""
    n = len(np.asarray(points).reshape(-1, 2))
    values = None if values is None else _two_dimensional(values, n)[:n]
    return position_grad_chunked(None, points, radius, power, _pair(G, values), _pair(values, G), gw, gw, True)


def query_queries_grad(points, radius, values, power, queries, G=None, gw=None):
    """The query form with respect to the queries: s = gw[r] + G_r . V_j."""
    if G is None or values is None:
        G = values = None
    return position_grad_chunked(queries, points, radius, power, G, values, gw, None)


def query_points_grad(points, radius, values, power, queries, G=None, gw=None):
    """The query form with respect to the points: the rows are the points, the partners the queries; s = gw[j] + V_r . G_j."""
    if G is None or values is None:
        G = values = None
    return position_grad_chunked(points, queries, radius, power, values, G, None, gw)
