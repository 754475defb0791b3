"""The named inputs of the weighted sums' tests: name -> Case(points (n, 2), radius, values (n, C), (n,) or None, power,
include_self, queries (q, 2) or None).  tests/test_field_cpu.py proves that each has the property it is named for;
tests/test_gpu_fields.py runs each on the device against tests/field_spec.py.  The search's own edges come from
tests/pairs_cases.py and the queries from tests/nearest_cases.py; the cases made here are those where the SUM can go wrong:
its order, its weights at the ends of 0 <= t <= 1, the channels of each kernel and the chunks of the wrapper."""
import collections
import functools

import numpy as np

import nearest_cases as NK
import pairs_cases as K
from sand_crate_amd import _native as N

Case = collections.namedtuple("Case", "points radius values power include_self queries")

OUTSIDE = ("point_outside_domain", "query_outside_domain")     # the cases whose result is the domain error
ORDER = "order_matters"
# the search's own edges (tests/pairs_cases.py), each with one power, width and include_self
SEARCH = ("n_0", "n_1", "n_2", "at_radius_3_4_5", "beyond_radius_3_4_5", "radius_0.1", "lattice_0.25", "lattice_0.01",
          "eight_cells", "misplaced_floor", "large_cells", "bucket_sharing", "long_rows", "non_finite", "domain_rim")
ROWS = (63, 64, 65, N.FIELDS_BLOCK - 1, N.FIELDS_BLOCK, N.FIELDS_BLOCK + 1)   # a wave's and a workgroup's edges
WIDTHS = tuple(range(1, N.FIELDS_MAX_CHANNELS + 1)) + (9, 17)                 # every kernel, guarded or not; two chunkings


def make_values(seed, n, channels=None):
    """randn * 10^randint(-8, 9) per point: magnitudes 17 decades apart in one row's sum, so its order shows.
    `channels` None: one-dimensional."""
    rs = np.random.RandomState(seed)
    scale = 10.0 ** rs.randint(-8, 9, size=n)
    v = rs.randn(n, channels or 1) * scale[:, None]
    return v if channels else v[:, 0]


def order_matters():
    """nearest_cases.nine_cells: row 0 has 108 partners from all nine cells with shuffled indices."""
    pts, radius = NK.nine_cells()
    return Case(pts, radius, make_values(5, len(pts), 3), 3, False, None)


def isolated():
    """Point 0 is 40 radii from a cloud: alone in its row with include_self, nothing without."""
    pts, radius = K.cloud(81, 50)
    return np.concatenate([[[1.0 + 40.0 * radius, 0.5]], pts]), radius


def at_the_radius(value):
    """(0, 0) and (3, 4) at radius 5: d2 == r2 exactly, t = 0 -- a partner with w = 0 for power >= 1."""
    return np.array([[0.0, 0.0], [3.0, 4.0]]), 5.0, np.array([[value, 1.0], [value, -2.0]])


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for at, name in enumerate(SEARCH):
        pts, radius = K.cases()[name]
        out[f"{name}_p{at % 4}"] = Case(pts, radius, make_values(200 + at, len(pts), 1 + at % 8), at % 4, at % 3 != 0, None)
    pts, radius = K.outside_domain()
    out[OUTSIDE[0]] = Case(pts, radius, make_values(230, len(pts), 2), 3, True, None)
    out[ORDER] = order_matters()
    out[ORDER + "_with_self"] = order_matters()._replace(include_self=True, power=1)
    for power in range(4):
        pts, radius = NK.pile()
        out[f"pile_70_p{power}"] = Case(pts, radius, make_values(240 + power, len(pts), 2), power, power % 2 == 0, None)
    for power in range(4):
        out[f"at_the_radius_p{power}"] = Case(*at_the_radius(3.5), power, False, None)
        out[f"at_the_radius_inf_p{power}"] = Case(*at_the_radius(np.inf), power, False, None)
    for include_self in (True, False):
        out[f"isolated_self_{int(include_self)}"] = Case(*isolated(), make_values(250, 51, 1), 2, include_self, None)
    for n in ROWS:
        out[f"rows_{n}"] = Case(*K.cloud(600 + n, n, partners=9.0), make_values(600 + n, n, 2), 3, True, None)
    pts, radius = K.cloud(91, 300, partners=10.0)
    for width in WIDTHS:
        out[f"channels_{width}"] = Case(pts, radius, make_values(700 + width, 300, width), 3, True, None)
    out["one_dimensional"] = Case(pts, radius, make_values(720, 300), 3, True, None)
    out["density"] = Case(pts, radius, None, 3, True, None)
    out["partner_count"] = Case(pts, radius, None, 0, False, None)
    for power in range(4):
        out[f"power_{power}"] = Case(pts, radius, make_values(730, 300, 4), power, True, None)
    bad = make_values(740, 300, 3)
    bad[::17, 0], bad[5::23, 1], bad[7::29, 2] = np.nan, np.inf, -np.inf
    out["values_not_finite"] = Case(pts, radius, bad, 3, True, None)
    for at, (name, (qpts, qradius, _, queries)) in enumerate(NK.query_cases().items()):
        case = Case(qpts, qradius, make_values(800 + at, len(qpts), 1 + (3 * at) % 8), at % 4, at % 2 == 0, queries)
        out[OUTSIDE[1] if name == NK.OUTSIDE else name] = case
    q_pts, q_radius = K.cloud(73, 700, partners=12.0)
    for n in ROWS:
        out[f"queries_{n}"] = Case(q_pts, q_radius, make_values(900 + n, 700, 2), 3, True, np.random.RandomState(900 + n).rand(n, 2))
    out["query_density"] = Case(q_pts, q_radius, None, 3, True, np.random.RandomState(77).rand(100, 2))
    for case in out.values():
        for a in (case.points, case.values, case.queries):
            if a is not None:
                a.setflags(write=False)
    return out
