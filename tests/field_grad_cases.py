"""The named inputs of the tests of the weighted sums' gradients: name -> Case(points, radius, values (n, C) or None, power,
include_self, queries or None, G (rows, C) or None, gw (rows,) or None) -- a case of tests/field_cases.py (which takes
the search's edges from tests/pairs_cases.py and the queries from tests/nearest_cases.py) with the upstream gradients of
`sums` and `wsum` beside it.  G and gw come from a seeded RandomState with magnitudes decades apart, as
`field_cases.make_values` makes the values, so that the order of a sum shows.  tests/test_field_grad_cpu.py proves that
each has the property it is named for; tests/test_gpu_field_grad.py runs each on the device against
tests/field_grad_spec.py.  The cases are the places where the gradient kernel can go wrong: the order of its sums, the
weights at the ends of 0 <= t <= 1 -- power 1 has m = 1 at d2 == r2 --, dx = dy = 0, rows without partners, the edges of
a wave and a workgroup, the channels of each kernel (twice the values' in the self form) and the groups of the wrapper,
the scalars alone and the dot product alone."""
import collections
import functools
import zlib

import numpy as np

import field_cases as FK
import field_grad_spec as GS
import pairs_cases as K

Case = collections.namedtuple("Case", "points radius values power include_self queries G gw")

OUTSIDE = FK.OUTSIDE
ORDER = FK.ORDER
PILE = tuple(f"pile_70_p{power}" for power in range(4))
AT_THE_RADIUS = tuple(f"at_the_radius_p{power}" for power in range(4))
SMALL = ("n_0_p0", "n_1_p1", "n_2_p2")
ROWS = tuple(f"rows_{n}" for n in FK.ROWS) + tuple(f"queries_{n}" for n in FK.ROWS)
WIDTHS = tuple(f"channels_{width}" for width in FK.WIDTHS)
QUERIES = ("q_0", "n_0_q_10", "q_300", "query_on_a_point", "query_not_finite", "query_in_empty_cells", "query_at_the_rim")
# taken from tests/field_cases.py as they are
TAKEN = ((ORDER, ORDER + "_with_self") + PILE + AT_THE_RADIUS + ("at_the_radius_inf_p1", "at_the_radius_inf_p3")
         + ("isolated_self_0", "isolated_self_1") + SMALL + ("non_finite_p1", "domain_rim_p2", "values_not_finite")
         + ROWS + WIDTHS + ("one_dimensional", "density", "partner_count", "query_density")
         + tuple(f"power_{power}" for power in range(4)) + QUERIES + OUTSIDE)
ONLY_GW = ("density", "query_density", "partner_count")          # no values: the gradient of the density
NO_GW = ("no_gw", "no_gw_queries")
COINCIDENT = "coincident"


def upstream(name, case):
    """G like the values' shape over the rows, gw over the rows: randn * 10^randint(-8, 9) per row."""
    rows = len(case.points) if case.queries is None else len(case.queries)
    seed = zlib.crc32(name.encode()) % (2 ** 31)
    width = None if case.values is None else (1 if case.values.ndim == 1 else case.values.shape[1])
    G = None if width is None else FK.make_values(seed, rows, width)
    return G, FK.make_values(seed + 1, rows)


def coincident():
    """A cloud in which every fifth point is a copy of its predecessor: partners at dx = dy = 0 among others."""
    pts, radius = K.cloud(95, 200, partners=8.0)
    pts = pts.copy()
    pts[4::5] = pts[3::5]
    return pts, radius


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for name in TAKEN:
        case = FK.cases()[name]
        out[name] = Case(*case, *upstream(name, case))
    for name in ("query_not_finite", "query_at_the_rim"):           # (power 0 in tests/field_cases.py: no gradient there)
        out[name + "_p3"] = out[name]._replace(power=3)
    pts, radius = coincident()
    for power in (1, 2, 3):
        case = FK.Case(pts, radius, FK.make_values(960 + power, len(pts), 3), power, power != 2, None)
        out[f"{COINCIDENT}_p{power}"] = Case(*case, *upstream(f"{COINCIDENT}_p{power}", case))
    for name in ("long_rows", "non_finite", "eight_cells", "bucket_sharing"):   # the search's edges at the full power
        pts, radius = K.cases()[name]
        case = FK.Case(pts, radius, FK.make_values(970, len(pts), 2), 3, True, None)
        out[name] = Case(*case, *upstream(name, case))
    out[NO_GW[0]] = out["channels_3"]._replace(gw=None)
    out[NO_GW[1]] = out["queries_65"]._replace(gw=None)
    out["no_G"] = out["channels_5"]._replace(G=None)                # values, but nobody used the sums
    out["no_G_queries"] = out["queries_63"]._replace(G=None)
    for case in out.values():
        for a in (case.G, case.gw):
            if a is not None:
                a.setflags(write=False)
    return out


def two_dimensional(a):
    return None if a is None else (a[:, None] if a.ndim == 1 else a)


def rows_of(case):
    return len(case.points) if case.queries is None else len(case.queries)


def values_of(case):
    return None if case.values is None else two_dimensional(case.values)[:len(case.points)]


def uses(case):
    """The launches of the rule's three-row table for this case: "points" or "queries" -> the arguments of
    `field_grad_spec.position_grad` (rows_xy, points, row_a, part_b, row_s, part_s, self_form), the channels not yet
    grouped."""
    V, G, gw = values_of(case), two_dimensional(case.G), case.gw
    dot = V is not None and G is not None
    if case.queries is None:
        a = np.concatenate([G, V], axis=1) if dot else None
        b = np.concatenate([V, G], axis=1) if dot else None
        return {"points": (None, case.points, a, b, gw, gw, True)}
    return {"queries": (case.queries, case.points, G if dot else None, V if dot else None, gw, None, False),
            "points": (case.points, case.queries, V if dot else None, G if dot else None, None, gw, False)}


def grads_of(case):
    """The rule's gradients of a case: {"values": (n, C), "points": (n, 2), "queries": (q, 2)} -- "values" only with values
    and G, "queries" only in the query form."""
    V, G, gw = values_of(case), two_dimensional(case.G), case.gw
    out = {}
    with np.errstate(all="ignore"):
        if V is not None and G is not None:
            out["values"] = GS.values_grad(case.points, case.radius, G, case.power, case.include_self, case.queries)
        if case.queries is None:
            out["points"] = GS.self_points_grad(case.points, case.radius, V, case.power, G, gw)
        else:
            out["queries"] = GS.query_queries_grad(case.points, case.radius, V, case.power, case.queries, G, gw)
            out["points"] = GS.query_points_grad(case.points, case.radius, V, case.power, case.queries, G, gw)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def spec(name):
    """`grads_of` a named case, computed once and shared."""
    return grads_of(cases()[name])
