"""The named inputs of the cluster labelling's tests: name -> (points (n, 2) float64, radius).
tests/test_cluster_cases_cpu.py proves that each has the property it is named for; tests/test_gpu_clusters.py runs each on
the device against tests/cluster_spec.py.  Cases the pair search already has come from tests/pairs_cases.py.  Every case
has at most SMALL points, except `wide`."""
import functools

import numpy as np

import pairs_cases as K
from sand_crate_amd import _native as N

SMALL = 5000
PARTNERS = (2.0, 4.5, 8.0)          # many small clusters, near percolation (about 4.51 in the plane), one giant


def exactly_radius():
    """Radius 5s, s = 1/8 (every number below is exact).  (0, 0) and (3s, 4s): d2 == r2, joined.  The same pair 64s to the
    right with the second point one ulp further up: split.  A third pair, joined, in a far cell that falls into the bucket
    of the cell of (0, 0)."""
    s = 0.125
    radius = 5 * s
    h = float(K.cell_size(radius))
    buckets = N.pairs_buckets(6)
    own = N.pairs_bucket(0, 0, buckets)
    fx, fy = next((fx, 30000) for fx in range(-90000, -80000) if N.pairs_bucket(fx, 30000, buckets) == own)
    far = ((fx + 0.25) * h, (fy + 0.25) * h)
    pts = [(0.0, 0.0), (3 * s, 4 * s), (64 * s, 0.0), (67 * s, np.nextafter(4 * s, 1.0)), far, (far[0] + 0.3 * h, far[1] + 0.4 * h)]
    return np.array(pts), radius


SERPENTINE_ROWS, SERPENTINE_RUN = 64, 63


def serpentine_path():
    """4,096 points along a boustrophedon path, radius 1: rows of 63 points 0.9 apart, 1.5 above each other, and after each
    row one point half way up to the next, 0.75 from both row ends: only neighbours on the path are within the radius."""
    pts = []
    for row in range(SERPENTINE_ROWS):
        cols = range(SERPENTINE_RUN) if row % 2 == 0 else range(SERPENTINE_RUN - 1, -1, -1)
        pts += [(0.9 * c, 1.5 * row) for c in cols]
        pts.append((pts[-1][0], 1.5 * row + 0.75))
    return np.array(pts)


def serpentine_orders():
    """name -> where each point of the path goes: index[k] is the index of the k-th point along the path."""
    n = SERPENTINE_ROWS * (SERPENTINE_RUN + 1)
    bits = n.bit_length() - 1
    assert n == 1 << bits
    k = np.arange(n)
    return {"along": k, "reversed": k[::-1].copy(), "bit_reversed": np.array([int(format(v, f"0{bits}b")[::-1], 2) for v in k]),
            "shuffled": np.random.RandomState(61).permutation(n)}


def serpentine(order):
    path = serpentine_path()
    pts = np.empty_like(path)
    pts[serpentine_orders()[order]] = path
    return pts, 1.0


def lattice(side=64, spacing=0.25):
    """side x side points `spacing` apart in raster order, radius = spacing: every point hangs on its four neighbours at
    exactly the radius, and the parent chains of a union by smallest index are as deep as they get."""
    c = np.arange(side, dtype=np.float64) * spacing
    x, y = np.meshgrid(c, c)
    return np.stack([x.ravel(), y.ravel()], axis=1), spacing


COMB_WIDTH, COMB_TEETH = 41, 5


def two_combs_parts():
    """-> (points, radius 1, comb of every point: 0 / 1).  Comb 0: a spine of COMB_WIDTH points on y = 0, one apart, and on
    every fourth (x = 0, 4, ...) a tooth of COMB_TEETH points upwards, one apart.  Comb 1: the same upside down from a spine
    on y = top, the float above COMB_TEETH + 1, its teeth on x = 2, 6, ...  A tooth's tip is top - COMB_TEETH = 1 + ulp(top)
    from the other comb's spine: the squared distance is above 1, so the combs never join.  All differences are exact.
    Shuffled together."""
    top = np.nextafter(COMB_TEETH + 1.0, np.inf)
    pts, comb = [], []
    for x in range(COMB_WIDTH):
        pts += [(float(x), 0.0), (float(x), top)]
        comb += [0, 1]
        if x % 4 == 0:
            pts += [(float(x), float(t)) for t in range(1, COMB_TEETH + 1)]
            comb += [0] * COMB_TEETH
        if x % 4 == 2:
            pts += [(float(x), top - t) for t in range(1, COMB_TEETH + 1)]
            comb += [1] * COMB_TEETH
    order = np.random.RandomState(62).permutation(len(pts))
    return np.array(pts)[order], 1.0, np.array(comb)[order]


def two_combs_sizes():
    teeth0, teeth1 = (COMB_WIDTH + 3) // 4, (COMB_WIDTH + 1) // 4
    return COMB_WIDTH + COMB_TEETH * teeth0, COMB_WIDTH + COMB_TEETH * teeth1


LATE_CLUSTERS, LATE_EACH = 5, 4


def late_root():
    """Radius 1.  Indices 0 .. 19: five clusters far from each other, point i in cluster i % 5.  Indices 20 .. 22: a cluster
    of its own whose smallest member is 20 -- and which lies LEFT of all the others, so neither position nor largest
    member gives its number.  Index 23 belongs to the cluster of index 0."""
    pts = [(10.0 * (i % LATE_CLUSTERS) + 0.3 * (i // LATE_CLUSTERS), 0.0) for i in range(LATE_CLUSTERS * LATE_EACH)]
    pts += [(-50.0, 0.0), (-50.5, 0.0), (-50.0, 0.5), (0.0, 0.6)]
    return np.array(pts), 1.0


def isolated(n=500):
    """A shuffled grid 1.5 radii apart: nobody has a partner."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.random.RandomState(63).permutation(side * side)[:n]
    return np.stack([1.5 * (k % side), 1.5 * (k // side)], axis=1).astype(np.float64), 1.0


NOT_FINITE_CLOUD = 400


def not_finite():
    """A cloud at 8 partners with NaN, +inf and -inf in x, in y and in both scattered through it (pairs_cases.non_finite's
    pattern), and behind it two triples 1.6 radii apart with two points in the middle between them, one with y NaN and one
    with x -inf: were they finite, either would join the triples."""
    pts, radius = K.cloud(71, NOT_FINITE_CLOUD, partners=8.0)
    values = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(np.random.RandomState(72).choice(NOT_FINITE_CLOUD, 90, replace=False)):
        v = values[k % 3]
        if k % 4 == 0:
            pts[i] = (v, values[(k + 1) % 3])
        elif k % 4 in (1, 3):
            pts[i, 0] = v
        else:
            pts[i, 1] = v
    r = radius
    left = [(5.0, 5.0), (5.0 - 0.5 * r, 5.0), (5.0, 5.0 + 0.5 * r)]
    right = [(5.0 + 1.6 * r, 5.0), (5.0 + 2.1 * r, 5.0), (5.0 + 1.6 * r, 5.0 - 0.5 * r)]
    between = [(5.0 + 0.8 * r, np.nan), (-np.inf, 5.0)]
    return np.concatenate([pts, np.array(left + between + right)]), radius


def wide():
    """70,001 points near percolation: more than 2^16 rows, several blocks of the scan, 274 workgroups."""
    return K.cloud(81, 70001, partners=4.5)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in K.edge_sizes():
        for partners in PARTNERS:
            out[f"n_{n}_partners_{partners}"] = K.cloud(200 + n, n, partners)
    out["exactly_radius"] = exactly_radius()
    out["bucket_sharing"] = K.bucket_sharing()
    for order in serpentine_orders():
        out[f"serpentine_{order}"] = serpentine(order)
    out["lattice"] = lattice()
    out["two_combs"] = two_combs_parts()[:2]
    out["late_root"] = late_root()
    out["isolated"] = isolated()
    out["piles"] = K.long_rows()
    out["not_finite"] = not_finite()
    out["wide"] = wide()
    for pts, _ in out.values():
        pts.setflags(write=False)
    return out


def small_cases():
    return {name: case for name, case in cases().items() if len(case[0]) <= SMALL}
