"""The rule of the device cluster labelling (sc_pairs_label_device, `Crate.cluster_tensors`), in NumPy.

The graph is exactly that of tests/pairs_spec.py: for `points`, an (n, 2) float64 array, and a `radius`, i ~ j iff (i, j)
is a pair there (i != j and fl(fl(dx dx) + fl(dy dy)) <= fl(radius radius)).  A cluster is a connected component of that
graph over the points whose coordinates are all finite; a point with a coordinate that is not finite is in no cluster (and
has no partners, so it bridges none).  Clusters are numbered 0 .. C-1 in ascending order of their smallest member index:
`roots[c]` is that member, `sizes[c]` the member count, `labels[i]` the cluster of point i, or -1 for a point in none.  The
result is a pure function of the points: `half` lists and full lists give the same clusters.
"""
import numpy as np

import pairs_spec


def components(n, offsets, partners, alive=None):
    """-> (labels, sizes, roots), all int64, of the graph on n nodes given as a CSR list (half or full: an edge counts in
    both directions): what `clusters` gives, by another way.  `alive` (bool (n,), default all): the nodes that are in a
    cluster at all; the others get -1 and must have no edges.  Min-label propagation with pointer jumping, vectorised:
    usable at some 10^5 nodes."""
    n = int(n)
    offsets = np.asarray(offsets, dtype=np.int64)
    j = np.asarray(partners, dtype=np.int64)
    assert offsets.shape == (n + 1,) and offsets[0] == 0 and offsets[n] == len(j)
    i = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    i, j = np.concatenate([i, j]), np.concatenate([j, i])
    alive = np.ones(n, dtype=bool) if alive is None else np.asarray(alive, dtype=bool)
    assert alive.shape == (n,) and alive[i].all()
    low = np.arange(n, dtype=np.int64)           # low[x] <= x, a member of x's component, low[low[x]] == low[x]
    while True:
        nxt = low.copy()
        np.minimum.at(nxt, low[i], low[j])       # the label's own node hears of the smaller label next door ...
        np.minimum.at(nxt, i, low[j])            # ... and so does the node
        while True:                              # pointer jumping, to the fixed point
            up = nxt[nxt]
            if np.array_equal(up, nxt):
                break
            nxt = up
        if np.array_equal(nxt, low):
            break                                # every edge joins equal labels: each is its component's smallest member
        low = nxt
    roots = np.unique(low[alive])
    labels = np.where(alive, np.searchsorted(roots, low), -1).astype(np.int64)
    sizes = np.bincount(labels[alive], minlength=len(roots)).astype(np.int64)
    return labels, sizes, roots.astype(np.int64)


def clusters(points, radius):
    """-> (labels int64 (n,), sizes int64 (C,), roots int64 (C,)): a plain graph search over the full pair list, one node
    at a time (a few thousand points)."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    offsets, partners, _ = pairs_spec.pairs(p, radius)
    alive = np.isfinite(p).all(axis=1)
    labels = np.full(len(p), -1, dtype=np.int64)
    sizes, roots = [], []
    for s in range(len(p)):                      # ascending: a cluster is met first at its smallest member
        if not alive[s] or labels[s] >= 0:
            continue
        c = len(roots)
        labels[s] = c
        stack, count = [s], 0
        while stack:
            x = stack.pop()
            count += 1
            for y in partners[offsets[x]:offsets[x + 1]]:
                if labels[y] < 0:
                    labels[y] = c
                    stack.append(int(y))
        roots.append(s)
        sizes.append(count)
    return labels, np.array(sizes, dtype=np.int64), np.array(roots, dtype=np.int64)
