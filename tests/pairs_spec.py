"""The rule of the device pair search (sc_pairs_count_device / sc_pairs_fill_device, `Crate.pair_tensors`), in NumPy.

Inputs: `points`, an (n, 2) float64 array, and `radius`, finite and > 0.  All arithmetic is float64, every operation
rounded on its own (the library is built with -ffp-contract=off):

    dx = x[i] - x[j];  dy = y[i] - y[j];  d2 = dx*dx + dy*dy
    (i, j) is a pair  iff  i != j  and  d2 <= radius*radius

A point with a coordinate that is not finite has no partners and is nobody's partner (d2 is then NaN or +inf next to a
finite radius*radius); coincident points are pairs of each other.  `partners` (int64) holds all j of row 0 ascending, then
row 1, ...; `offsets` (int64, n + 1) is the exclusive scan of the row lengths, offsets[n] = E; `half` keeps j > i only;
`d2` is the number that was compared, per pair.  The domain: every FINITE coordinate c satisfies |c| / radius < 2^31 (the
rounded float64 quotient); `in_domain` says whether.  Brute force in row blocks: fine up to a few thousand points.
"""
import numpy as np

BLOCK = 512


def in_domain(points, radius):
    p = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    c = np.abs(p[np.isfinite(p)])
    return bool((c / np.float64(radius) < 2.0 ** 31).all())


def pairs(points, radius, half=False):
    """-> (offsets int64 (n + 1,), partners int64 (E,), d2 float64 (E,))"""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    n = len(p)
    radius = np.float64(radius)
    assert np.isfinite(radius) and radius > 0
    r2 = radius * radius
    x, y = p[:, 0], p[:, 1]
    lengths = np.zeros(n, dtype=np.int64)
    js, ds = [], []
    index = np.arange(n)
    with np.errstate(all="ignore"):
        for lo in range(0, n, BLOCK):
            hi = min(n, lo + BLOCK)
            dx = x[lo:hi, None] - x[None, :]
            dy = y[lo:hi, None] - y[None, :]
            d2 = dx * dx + dy * dy
            ok = d2 <= r2                                   # (NaN compares false)
            ok &= index[lo:hi, None] != index[None, :]
            if half:
                ok &= index[None, :] > index[lo:hi, None]
            lengths[lo:hi] = ok.sum(axis=1)
            rows, cols = np.nonzero(ok)                     # row-major: rows ascending, then columns ascending
            js.append(cols.astype(np.int64))
            ds.append(d2[rows, cols])
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lengths, out=offsets[1:])
    partners = np.concatenate(js) if js else np.zeros(0, dtype=np.int64)
    d2 = np.concatenate(ds) if ds else np.zeros(0, dtype=np.float64)
    return offsets, partners, d2


def coincident_offsets(n, half=False):
    """The offsets of n coincident points, in closed form: every row has the n - 1 others (half: the n - 1 - i behind)."""
    k = np.arange(n + 1, dtype=np.int64)
    return k * (n - 1) - k * (k - 1) // 2 if half else k * (n - 1)


def coincident_partners(n, first, count, half=False):
    """Entries first .. first + count of the partners of n coincident points: row i is 0 .. n - 1 without i (half: i + 1 ..
    n - 1); d2 is 0 for every one."""
    e = np.arange(first, first + count, dtype=np.int64)
    if not half:
        row, t = e // (n - 1), e % (n - 1)
        return t + (t >= row)
    offsets = coincident_offsets(n, True)
    row = np.searchsorted(offsets, e, side="right") - 1
    return row + 1 + (e - offsets[row])
