"""The rule of the batched clusters, cluster sums, histograms, rays and ray paths (sc_pairs_label_batch_device,
sc_pairs_hist_batch_device, sc_pairs_rays_batch_device, sc_pairs_ray_paths_batch_device), in NumPy.

As in tests/batch_spec.py there is no new arithmetic.  `ptr` holds B + 1 ascending offsets, cloud b is
``points[ptr[b]:ptr[b + 1]]``; `query_ptr` / `ray_ptr` cuts the queries or the rays the same way, and query or ray cloud b
sees the points of cloud b only.  Every result is the existing rule (cluster_spec, cluster_sums_spec, hist_spec, ray_spec,
ray_path_spec) cloud by cloud, concatenated in cloud order:

  clusters   labels shifted by the running cluster count (-1 stays -1), roots by ptr[b]; `cluster_ptr`, int64 (B + 1,), is
             that running count -- cloud b's clusters are cluster_ptr[b] .. cluster_ptr[b + 1];
  sums       cluster_sums_spec.cluster_sums over those global labels;
  histogram  the tables concatenated, the totals stacked: int64 (B, bins);
  rays       the walls are shared by all clouds, a hit >= 0 is shifted by ptr[b];
  paths      the same per leg.
"""
import numpy as np

import cluster_spec
import cluster_sums_spec
import hist_spec
import ray_path_spec
import ray_spec
from batch_spec import _points, _ptr, clouds


def clusters(points, radius, ptr):
    """-> (labels int64 (n,), sizes int64 (C,), roots int64 (C,), cluster_ptr int64 (B + 1,))."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    labels, sizes, roots, cptr = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [0]
    for b in range(clouds(ptr)):
        lab, siz, roo = cluster_spec.clusters(p[ptr[b]:ptr[b + 1]], radius)
        labels.append(np.where(lab >= 0, lab + cptr[-1], lab))
        sizes.append(siz)
        roots.append(roo + ptr[b])
        cptr.append(cptr[-1] + len(siz))
    return (np.concatenate(labels).astype(np.int64), np.concatenate(sizes).astype(np.int64),
            np.concatenate(roots).astype(np.int64), np.array(cptr, dtype=np.int64))


def cluster_sums(points, radius, ptr, values, extrema=True):
    """-> (labels, sizes, roots, sums[, mins, maxs], cluster_ptr)."""
    labels, sizes, roots, cptr = clusters(points, radius, ptr)
    tables = cluster_sums_spec.cluster_sums(labels, values, len(sizes), extrema)
    return (labels, sizes, roots, *tables, cptr)


def histogram(points, edges, ptr, queries=None, query_ptr=None):
    """-> (table int32 (R, bins), total int64 (B, bins))."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    q = None if queries is None else _points(queries)
    qptr = None if q is None else _ptr(query_ptr, len(q))
    assert qptr is None or len(qptr) == len(ptr)
    bins = len(edges) - 1
    tables, totals = [np.zeros((0, bins), dtype=np.int32)], [np.zeros((0, bins), dtype=np.int64)]
    for b in range(clouds(ptr)):
        table, total = hist_spec.histogram(p[ptr[b]:ptr[b + 1]], edges, None if q is None else q[qptr[b]:qptr[b + 1]])
        tables.append(np.asarray(table, dtype=np.int32).reshape(-1, bins))
        totals.append(np.asarray(total, dtype=np.int64).reshape(1, bins))
    return np.concatenate(tables).astype(np.int32), np.concatenate(totals).astype(np.int64)


def _rays(origins, directions, ray_ptr, ptr):
    o, d = _points(origins), _points(directions)
    assert len(o) == len(d)
    rptr = _ptr(ray_ptr, len(o))
    assert len(rptr) == len(ptr)
    return o, d, rptr


def rays(points, walls, origins, directions, rho, max_t, ptr, ray_ptr):
    """-> (t float64 (R,), hit int64 (R,)), a hit >= 0 global."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    o, d, rptr = _rays(origins, directions, ray_ptr, ptr)
    ts, hits = [np.zeros(0)], [np.zeros(0, dtype=np.int64)]
    for b in range(clouds(ptr)):
        t, hit = ray_spec.rays(p[ptr[b]:ptr[b + 1]], walls, o[rptr[b]:rptr[b + 1]], d[rptr[b]:rptr[b + 1]], rho, max_t)
        ts.append(t)
        hits.append(np.where(hit >= 0, hit + ptr[b], hit))
    return np.concatenate(ts).astype(np.float64), np.concatenate(hits).astype(np.int64)


def paths(points, walls, origins, directions, rho, max_t, bounces, ptr, ray_ptr, *, wrong=None):
    """-> (t (R, L), hit (R, L), P (R, L, 2), n (R, L, 2), end (R,)), a hit >= 0 global.  `wrong` is ray_path_spec's."""
    p = _points(points)
    ptr = _ptr(ptr, len(p))
    o, d, rptr = _rays(origins, directions, ray_ptr, ptr)
    legs = bounces + 1
    out = [[np.zeros((0, legs))], [np.zeros((0, legs), dtype=np.int64)], [np.zeros((0, legs, 2))], [np.zeros((0, legs, 2))],
           [np.zeros(0, dtype=np.int64)]]
    for b in range(clouds(ptr)):
        got = ray_path_spec.paths(p[ptr[b]:ptr[b + 1]], walls, o[rptr[b]:rptr[b + 1]], d[rptr[b]:rptr[b + 1]], rho, max_t,
                                  bounces, wrong=wrong)
        got = (got[0], np.where(got[1] >= 0, got[1] + ptr[b], got[1]), *got[2:])
        for k, a in enumerate(got):
            out[k].append(np.asarray(a).reshape((-1,) + out[k][0].shape[1:]))
    kinds = (np.float64, np.int64, np.float64, np.float64, np.int64)
    return tuple(np.concatenate(parts).astype(kind) for parts, kind in zip(out, kinds))
