"""The rule of the per-cluster sums and extents (sc_pairs_cluster_sums_device, `Crate.cluster_sums`), in NumPy.  Nothing
here imports the product; tests/test_gpu_cluster_sums.py holds the GPU to it byte for byte.

`labels` and C are those of tests/cluster_spec.py.  The members of cluster c are the rows i with ``labels[i] == c``, in
ascending i.  A row with label -1 belongs to no cluster: its values are never read into any result, even if they are NaN.

The sum of a channel over a cluster is `tree(v)`, v the members' values in ascending index: pairwise summation in groups
of 64, and groups of groups, every add rounded on its own.  The padding is +0.0 and a single member still goes through
one group, so a cluster whose terms are all -0.0 sums to +0.0: that is this rule's result, not that of the terms alone
(-0.0 + -0.0 is -0.0).  Nothing here is compared with ``np.sum``: its bits differ from the rule's at most sizes.

Minima and maxima are NumPy's (``np.minimum`` / ``np.maximum``): a NaN on either side is the result; they do not depend
on order.  The member count is the label's `sizes`.

A cluster's result is a pure function of its own members' values.

Which NaN.  A sum that is NaN is any NaN: the sign and payload of a NaN that an addition makes (inf + -inf) are the
processor's -- x86 sets the sign bit, the GPU does not -- and no rule of arithmetic fixes them.  `same` therefore compares
the bytes of every entry that is not a NaN, and asks of a NaN only that it is one on both sides."""
import math

import numpy as np

GROUP = 64


def tree(a):
    """a: float64, len >= 1."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    assert len(a) >= 1
    with np.errstate(all="ignore"):
        while True:
            a = np.concatenate([a, np.zeros((-len(a)) % GROUP)]).reshape(-1, GROUP)
            for _ in range(6):
                a = a[:, 0::2] + a[:, 1::2]          # neighbours, each add rounded on its own
            a = a.reshape(-1)
            if len(a) == 1:
                return a[0]


def levels(n):
    """How many groups-of-groups `tree` takes for n terms."""
    k = 1
    while GROUP ** k < n:
        k += 1
    return k


def bound(v):
    """|tree(v) - fsum(v)| <= (ceil(log2 n) + 6) * 2^-53 * fsum(|v|): every term passes through at most that many adds."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    depth = math.ceil(math.log2(len(v))) if len(v) > 1 else 0
    return (depth + 6) * 2.0 ** -53 * math.fsum(np.abs(v).tolist())


def cluster_sums(labels, values, clusters=None, extrema=True):
    """-> (sums, mins, maxs), each float64 (C, F), of `values` (n, F) or (n,) over the clusters of `labels` (n,)."""
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    values = np.asarray(values, dtype=np.float64)
    values = values.reshape(len(values), 1) if values.ndim == 1 else values
    assert len(values) >= len(labels)
    total = (int(labels.max()) + 1 if len(labels) else 0) if clusters is None else int(clusters)
    width = values.shape[1]
    sums, mins, maxs = (np.empty((total, width)) for _ in range(3))
    order = np.argsort(labels, kind="stable")         # members together, ascending in index
    order = order[labels[order] >= 0]
    ends = np.cumsum(np.bincount(labels[order], minlength=total))
    with np.errstate(all="ignore"):
        for c in range(total):
            rows = values[order[(ends[c - 1] if c else 0):ends[c]]]
            assert len(rows) >= 1
            for f in range(width):
                sums[c, f] = tree(rows[:, f])
            if extrema:
                mins[c] = np.minimum.reduce(rows, axis=0)
                maxs[c] = np.maximum.reduce(rows, axis=0)
    return (sums, mins, maxs) if extrema else (sums,)


def same(got, want):
    """Byte for byte, except that a NaN equals any NaN (the module's docstring says why)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype != np.float64:
        return got.tobytes() == want.tobytes()
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.where(nan, 0.0, got).tobytes() == np.where(nan, 0.0, want).tobytes()


CHANNELS = ("x", "y", "vx", "vy", "ke", "p", "speed2", "pressed")
FIELDS = ("n", "sum_x", "sum_y", "sum_vx", "sum_vy", "sum_ke", "sum_p", "min_x", "max_x", "min_y", "max_y", "max_speed2",
          "max_p", "n_pressed")


def channels(xy, vxy, pressure):
    """The (n, 8) table `Crate.cluster_observables` reduces: every operation rounded on its own, the squared speed once."""
    xy, vxy = np.asarray(xy, dtype=np.float64).reshape(-1, 2), np.asarray(vxy, dtype=np.float64).reshape(-1, 2)
    p = np.asarray(pressure, dtype=np.float64).reshape(-1)
    with np.errstate(all="ignore"):
        speed2 = vxy[:, 0] * vxy[:, 0] + vxy[:, 1] * vxy[:, 1]
        return np.stack([xy[:, 0], xy[:, 1], vxy[:, 0], vxy[:, 1], 0.5 * speed2, p, speed2, (p > 0).astype(np.float64)], axis=1)


def observables(labels, sizes, xy, vxy, pressure):
    """-> the float64 (C, 14) table of FIELDS."""
    sums, mins, maxs = cluster_sums(labels, channels(xy, vxy, pressure), clusters=len(sizes))
    table = np.empty((len(sizes), len(FIELDS)))
    table[:, 0] = sizes
    table[:, 1:7] = sums[:, 0:6]
    table[:, 7], table[:, 8], table[:, 9], table[:, 10] = mins[:, 0], maxs[:, 0], mins[:, 1], maxs[:, 1]
    table[:, 11], table[:, 12], table[:, 13] = maxs[:, 6], maxs[:, 5], sums[:, 7]
    return table
