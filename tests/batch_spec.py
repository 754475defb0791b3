"""The rule of the batched neighbourhood calls (`batch=` / `query_batch=`; sc_pairs_set_batch_device), in NumPy.

There is no new arithmetic.  `ptr` holds B + 1 ascending offsets, cloud b is ``points[ptr[b]:ptr[b + 1]]``; with queries
`query_ptr` cuts them the same way, and query cloud b sees the points of cloud b only.  Every result is the result of the
existing rule (pairs_spec, nearest_spec, field_spec, field_grad_spec) cloud by cloud, concatenated in cloud order, with
the partner indices shifted by ptr[b] -- the padding of a nearest-k table, -1, stays -1.  Values and upstream gradients
are global arrays, cut like the rows they belong to.
"""
import numpy as np

import field_grad_spec
import field_spec
import nearest_spec
import pairs_spec


def _points(points):
    return np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)


def _ptr(ptr, n):
    ptr = np.asarray(ptr, dtype=np.int64)
    assert ptr.ndim == 1 and len(ptr) >= 2 and ptr[0] == 0 and ptr[-1] == n and (np.diff(ptr) >= 0).all()
    return ptr


def _cut(a, ptr, b):
    return None if a is None else np.asarray(a)[ptr[b]:ptr[b + 1]]


def _columns(a):
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(len(a), 1) if a.ndim == 1 else a


def clouds(ptr):
    return len(ptr) - 1


def cloud_of(ptr, n):
    """The cloud of every row: int64 (n,)."""
    ptr = _ptr(ptr, n)
    return np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr))


def pairs(points, radius, ptr, half=False):
    """-> (offsets int64 (n + 1,), partners int64 (E,), d2 float64 (E,)), partners global."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    offsets, partners, d2, total = [np.zeros(1, dtype=np.int64)], [], [], 0
    for b in range(clouds(ptr)):
        o, j, d = pairs_spec.pairs(p[ptr[b]:ptr[b + 1]], radius, half)
        offsets.append(o[1:] + total)
        total += int(o[-1])
        partners.append(j + ptr[b])
        d2.append(d)
    return (np.concatenate(offsets).astype(np.int64), np.concatenate(partners + [np.zeros(0, dtype=np.int64)]).astype(np.int64),
            np.concatenate(d2 + [np.zeros(0)]).astype(np.float64))


def nearest(points, radius, k, ptr, queries=None, query_ptr=None):
    """-> (neighbors int64 (R, k), d2 float64 (R, k), partners int64 (R,)), neighbours global, the padding -1."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    q = None if queries is None else _points(queries)
    qptr = None if q is None else _ptr(query_ptr, len(q))
    assert qptr is None or len(qptr) == len(ptr)
    nb, d2, count = [np.zeros((0, k), dtype=np.int64)], [np.zeros((0, k))], [np.zeros(0, dtype=np.int64)]
    for b in range(clouds(ptr)):
        j, d, c = nearest_spec.nearest(p[ptr[b]:ptr[b + 1]], radius, k, None if q is None else q[qptr[b]:qptr[b + 1]])
        nb.append(np.where(j >= 0, j + ptr[b], j).reshape(-1, k))
        d2.append(np.asarray(d).reshape(-1, k))
        count.append(c)
    return np.concatenate(nb).astype(np.int64), np.concatenate(d2).astype(np.float64), np.concatenate(count).astype(np.int64)


def field(points, radius, ptr, values=None, power=3, include_self=True, queries=None, query_ptr=None):
    """-> (out float64 (R, C), wsum float64 (R,)); C = 0 without values."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    q = None if queries is None else _points(queries)
    qptr = None if q is None else _ptr(query_ptr, len(q))
    assert qptr is None or len(qptr) == len(ptr)
    v = None if values is None else _columns(values)
    width = 0 if v is None else v.shape[1]
    out, wsum = [np.zeros((0, width))], [np.zeros(0)]
    for b in range(clouds(ptr)):
        o, w = field_spec.field(p[ptr[b]:ptr[b + 1]], radius, _cut(v, ptr, b), power, include_self,
                                None if q is None else q[qptr[b]:qptr[b + 1]])
        out.append(np.asarray(o, dtype=np.float64).reshape(len(w), width))
        wsum.append(w)
    return np.concatenate(out), np.concatenate(wsum)


def values_grad(points, radius, ptr, G, power, include_self=True, queries=None, query_ptr=None):
    """field_grad_spec.values_grad per cloud -> float64 (n, C); G belongs to the rows (the points, or the queries)."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    q = None if queries is None else _points(queries)
    qptr = ptr if q is None else _ptr(query_ptr, len(q))
    G = _columns(G)
    out = [np.zeros((0, G.shape[1]))]
    for b in range(clouds(ptr)):
        g = field_grad_spec.values_grad(p[ptr[b]:ptr[b + 1]], radius, G[qptr[b]:qptr[b + 1]], power, include_self,
                                        None if q is None else q[qptr[b]:qptr[b + 1]])
        out.append(np.asarray(g, dtype=np.float64).reshape(ptr[b + 1] - ptr[b], G.shape[1]))
    return np.concatenate(out)


def self_points_grad(points, radius, ptr, values, power, G=None, gw=None):
    """field_grad_spec.self_points_grad per cloud -> float64 (n, 2)."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    return np.concatenate([np.zeros((0, 2))] + [
        np.asarray(field_grad_spec.self_points_grad(p[ptr[b]:ptr[b + 1]], radius, _cut(values, ptr, b), power, _cut(G, ptr, b),
                                                    _cut(gw, ptr, b))).reshape(-1, 2) for b in range(clouds(ptr))])


def query_queries_grad(points, radius, ptr, values, power, queries, query_ptr, G=None, gw=None):
    """field_grad_spec.query_queries_grad per cloud -> float64 (q, 2); G and gw belong to the queries."""
    p, q = _points(points), _points(queries)
    ptr, qptr = _ptr(ptr, len(p)), _ptr(query_ptr, len(q))
    return np.concatenate([np.zeros((0, 2))] + [
        np.asarray(field_grad_spec.query_queries_grad(p[ptr[b]:ptr[b + 1]], radius, _cut(values, ptr, b), power,
                                                      q[qptr[b]:qptr[b + 1]], _cut(G, qptr, b), _cut(gw, qptr, b))).reshape(-1, 2)
        for b in range(clouds(ptr))])


def query_points_grad(points, radius, ptr, values, power, queries, query_ptr, G=None, gw=None):
    """field_grad_spec.query_points_grad per cloud -> float64 (n, 2); G and gw belong to the queries."""
    p, q = _points(points), _points(queries)
    ptr, qptr = _ptr(ptr, len(p)), _ptr(query_ptr, len(q))
    return np.concatenate([np.zeros((0, 2))] + [
        np.asarray(field_grad_spec.query_points_grad(p[ptr[b]:ptr[b + 1]], radius, _cut(values, ptr, b), power,
                                                     q[qptr[b]:qptr[b + 1]], _cut(G, qptr, b), _cut(gw, qptr, b))).reshape(-1, 2)
        for b in range(clouds(ptr))])
