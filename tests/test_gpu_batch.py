"""GPU tests of the batched neighbourhood calls (`batch=` / `query_batch=` of `Crate.pair_tensors`, `neighbor_tensors`,
`field_tensors` and `field_function`; sc_pairs_set_batch_device, sc_pairs_set_query_batch_device): every result against
the rule of tests/batch_spec.py -- the existing rules cloud by cloud -- bit for bit, floats compared as their 64 bits, on
the cases of tests/batch_cases.py.  And, unbatched, the readers in a row after one whose own flag went up: they share that
flag, and no call's verdict may reach the next."""
import functools

import numpy as np
import pytest

import batch_cases as BK
import batch_spec as BS
import gpu_support as U
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

ALL_CASES = BK.SELF_CASES + BK.QUERY_CASES
BATCH_ORDER = "batch offsets must start at 0, not descend and end at the number of points"


def tensor(a, tail=None, requires_grad=False):
    """Not U.tensor: this one keeps the array's own dtype, for the batch offsets are int64."""
    import torch
    if a is None:
        return None
    a = np.array(a)                                                                 # (a copy: the cases are read-only)
    t = torch.from_numpy(a if tail is None else a.reshape(-1, tail)).cuda()
    torch.cuda.synchronize()
    return t.requires_grad_() if requires_grad else t


def same_all(got, want):
    return len(got) == len(want) and all(U.same_bits_on_device(g, w) for g, w in zip(got, want))


def forms(name):
    return (False, True) if name in BK.QUERY_CASES else (False,)


def inputs(name, query_form=False):
    """-> the keyword arguments points=, batch= (and queries=, query_batch=) of a case, as CUDA tensors."""
    case = BK.cases()[name]
    kw = dict(points=tensor(case.points, 2), batch=tensor(case.ptr))
    if query_form:
        kw.update(queries=tensor(case.queries, 2), query_batch=tensor(case.query_ptr))
    return kw


def spec_args(name, query_form):
    case = BK.cases()[name]
    return dict(queries=case.queries, query_ptr=case.query_ptr) if query_form else {}


@functools.lru_cache(maxsize=None)
def values_of(name, width):
    v = np.random.RandomState(31 + width).rand(len(BK.cases()[name].points), width) - 0.5
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def pairs_spec_of(name, half):
    case = BK.cases()[name]
    return BS.pairs(case.points, case.radius, case.ptr, half)


@functools.lru_cache(maxsize=None)
def nearest_spec_of(name, k, query_form):
    case = BK.cases()[name]
    return BS.nearest(case.points, case.radius, k, case.ptr, **spec_args(name, query_form))


@functools.lru_cache(maxsize=None)
def field_spec_of(name, width, power, include_self, query_form):
    case = BK.cases()[name]
    return BS.field(case.points, case.radius, case.ptr, values_of(name, width), power, include_self,
                    **spec_args(name, query_form))


# ---- 1. the four functions against the rule

@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", ALL_CASES)
def test_pair_tensors_is_the_per_cloud_rule(crate, name, half):
    got = crate.pair_tensors(BK.RADIUS, half=half, squared_distances=True, **inputs(name))
    assert same_all(got, pairs_spec_of(name, half))


@pytest.mark.parametrize("k", [1, 16, 64])
@pytest.mark.parametrize("name", ALL_CASES)
def test_neighbor_tensors_is_the_per_cloud_rule(crate, name, k):
    for query_form in forms(name):
        got = crate.neighbor_tensors(k, BK.RADIUS, squared_distances=True, partner_counts=True, **inputs(name, query_form))
        assert same_all(got, nearest_spec_of(name, k, query_form)), query_form


FIELD_GRID = [(name, 3, 3, True) for name in ALL_CASES] + [
    (name, width, power, include_self) for name in ("boundaries", "queries") for width in (3, 11) for power in (0, 1, 2, 3)
    for include_self in (True, False) if (width, power, include_self) != (3, 3, True)]


@pytest.mark.parametrize("name,width,power,include_self", FIELD_GRID)
def test_field_tensors_is_the_per_cloud_rule(crate, name, width, power, include_self):
    """3 channels run the kernel of 4 with the loads guarded, 11 are a group of eight and one of three."""
    for query_form in forms(name):
        got = crate.field_tensors(tensor(values_of(name, width)), BK.RADIUS, power=power, include_self=include_self,
                                  weight_sums=True, **inputs(name, query_form))
        assert same_all(got, field_spec_of(name, width, power, include_self, query_form)), query_form
    if width == 3:                                                                  # ... and the density alone
        got = crate.field_tensors(None, BK.RADIUS, power=power, include_self=include_self, **inputs(name))
        assert same_all(got, field_spec_of(name, width, power, include_self, False)[1:])


@pytest.mark.parametrize("name", ALL_CASES)
def test_field_function_without_gradients_is_field_tensors(crate, name):
    for query_form in forms(name):
        got = crate.field_function(tensor(values_of(name, 3)), BK.RADIUS, weight_sums=True, **inputs(name, query_form))
        assert same_all(got, field_spec_of(name, 3, 3, True, query_form))


# ---- 2. gradients

def gradients(crate, name, width, power, query_form, needs):
    import torch
    case = BK.cases()[name]
    kw = inputs(name, query_form)
    values = tensor(values_of(name, width), requires_grad="values" in needs)
    kw["points"].requires_grad_("points" in needs)
    if query_form:
        kw["queries"].requires_grad_("queries" in needs)
    rows = len(case.queries if query_form else case.points)
    rs = np.random.RandomState(77)
    G, gw = rs.rand(rows, width) - 0.5, rs.rand(rows) - 0.5
    sums, wsum = crate.field_function(values, BK.RADIUS, power=power, weight_sums=True, **kw)
    wanted = [t for t, key in ((values, "values"), (kw["points"], "points"), (kw.get("queries"), "queries")) if key in needs]
    got = torch.autograd.grad((sums, wsum), wanted, (tensor(G), tensor(gw)))
    return dict(zip([key for key in ("values", "points", "queries") if key in needs], got)), G, gw


@pytest.mark.parametrize("name,width,power", [("triplets", 3, 3), ("collisions", 5, 2), ("empties", 3, 3), ("all_empty", 3, 3),
                                              ("boundaries", 3, 1), ("nonfinite", 3, 3), ("queries", 3, 2)])
def test_self_form_gradients_are_the_per_cloud_rule(crate, name, width, power):
    """5 channels make [G | V] ten wide: two launches of the position kernel, added up as the rule adds them."""
    case = BK.cases()[name]
    got, G, gw = gradients(crate, name, width, power, False, ("values", "points"))
    assert U.same_bits_on_device(got["values"], BS.values_grad(case.points, case.radius, case.ptr, G, power))
    assert U.same_bits_on_device(got["points"], BS.self_points_grad(case.points, case.radius, case.ptr, values_of(name, width),
                                                                    power, G, gw))


@pytest.mark.parametrize("width,power", [(3, 3), (5, 2)])
def test_query_form_gradients_are_the_per_cloud_rule(crate, width, power):
    name = "queries"
    case = BK.cases()[name]
    got, G, gw = gradients(crate, name, width, power, True, ("values", "points", "queries"))
    args = (case.points, case.radius, case.ptr, values_of(name, width), power, case.queries, case.query_ptr)
    assert U.same_bits_on_device(got["values"], BS.values_grad(case.points, case.radius, case.ptr, G, power, True, case.queries,
                                                               case.query_ptr))
    assert U.same_bits_on_device(got["queries"], BS.query_queries_grad(*args, G=G, gw=gw))
    assert U.same_bits_on_device(got["points"], BS.query_points_grad(*args, G=G, gw=gw))


# ---- 3. one cloud, the setter's life, the forms that do not synchronise

def test_one_cloud_equals_the_unbatched_call(crate):
    kw = inputs("single")
    points, values = kw["points"], tensor(values_of("single", 3))
    for half in (False, True):
        a = crate.pair_tensors(BK.RADIUS, half=half, squared_distances=True, **kw)
        b = crate.pair_tensors(BK.RADIUS, half=half, squared_distances=True, points=points)
        assert same_all(a, [t.cpu().numpy() for t in b])
    a = crate.neighbor_tensors(16, BK.RADIUS, squared_distances=True, partner_counts=True, **kw)
    b = crate.neighbor_tensors(16, BK.RADIUS, squared_distances=True, partner_counts=True, points=points)
    assert same_all(a, [t.cpu().numpy() for t in b])
    a = crate.field_tensors(values, BK.RADIUS, weight_sums=True, **kw)
    b = crate.field_tensors(values, BK.RADIUS, weight_sums=True, points=points)
    assert same_all(a, [t.cpu().numpy() for t in b])
    a = crate.field_function(values, BK.RADIUS, weight_sums=True, **kw)
    assert same_all(a, [t.cpu().numpy() for t in b])


def test_a_batch_is_consumed_by_its_call(crate):
    """The unbatched call after a batched one is what it was before; and the clusters and the histograms, which count for
    themselves, give their unbatched results right after a batched call."""
    from sand_crate_amd import pairs
    kw = inputs("triplets")
    points = kw["points"]
    edges = pairs.shell_edges(BK.RADIUS, 8)
    before = [crate.pair_tensors(BK.RADIUS, points=points, squared_distances=True),
              crate.neighbor_tensors(4, BK.RADIUS, points=points, squared_distances=True),
              crate.field_tensors(None, BK.RADIUS, points=points),
              crate.cluster_tensors(BK.RADIUS, points=points),
              crate.distance_histogram(edges, points=points, per_row=True)]
    batched = crate.pair_tensors(BK.RADIUS, squared_distances=True, **kw)
    assert int(batched[0][-1]) < int(before[0][0][-1])                              # (the twins are gone)
    after = [crate.pair_tensors(BK.RADIUS, points=points, squared_distances=True)]
    crate.pair_tensors(BK.RADIUS, **kw)
    after.append(crate.neighbor_tensors(4, BK.RADIUS, points=points, squared_distances=True))
    crate.neighbor_tensors(4, BK.RADIUS, **kw)
    after.append(crate.field_tensors(None, BK.RADIUS, points=points))
    crate.field_tensors(None, BK.RADIUS, **kw)
    after.append(crate.cluster_tensors(BK.RADIUS, points=points))
    crate.neighbor_tensors(4, BK.RADIUS, **kw)
    after.append(crate.distance_histogram(edges, points=points, per_row=True))
    for a, b in zip(after, before):
        assert same_all(a, [t.cpu().numpy() for t in b])
    # set by hand and cleared by hand: the count after it is unbatched
    eng = crate.engine
    eng.pairs_set_batch(kw["batch"])
    eng.pairs_set_batch(None)
    assert same_all(crate.pair_tensors(BK.RADIUS, points=points, squared_distances=True), [t.cpu().numpy() for t in before[0]])


@pytest.mark.parametrize("name", ["boundaries", "queries"])
def test_the_forms_that_do_not_synchronise_equal_the_default(crate, name):
    case = BK.cases()[name]
    n = len(case.points)
    want = pairs_spec_of(name, False)
    total = int(want[0][-1])
    offsets, partners, d2, counts = crate.pair_tensors(BK.RADIUS, squared_distances=True, max_pairs=total + 7, **inputs(name))
    crate.synchronize()
    assert counts.tolist() == [n, total]
    assert same_all((offsets[:n + 1], partners[:total], d2[:total]), want)
    values = tensor(values_of(name, 3))
    for query_form in forms(name):
        rows = len(case.queries if query_form else case.points)
        *got, counts = crate.neighbor_tensors(16, BK.RADIUS, squared_distances=True, partner_counts=True, sync=False,
                                              **inputs(name, query_form))
        crate.synchronize()
        assert int(counts[0]) == rows and int(counts[1]) >= 0
        assert same_all([t[:rows] for t in got], nearest_spec_of(name, 16, query_form))
        *got, counts = crate.field_tensors(values, BK.RADIUS, weight_sums=True, sync=False, **inputs(name, query_form))
        crate.synchronize()
        assert counts.tolist() == [rows, 0]
        assert same_all([t[:rows] for t in got], field_spec_of(name, 3, 3, True, query_form))


# ---- 4. the readers that are not batched yet

def test_label_and_histogram_refuse_a_batched_grid(crate):
    import torch
    from sand_crate_amd import _native as N
    eng = crate.engine
    kw = inputs("triplets")
    n = len(BK.cases()["triplets"].points)
    offsets, counts = U.full(n + 1, "cuda"), U.full(2, "cuda")
    eng.pairs_count(kw["points"], radius=BK.RADIUS, offsets=offsets, counts=counts, batch=kw["batch"])
    labels, sizes, roots, label_counts = U.full(n, "cuda"), U.full(n, "cuda"), U.full(n, "cuda"), U.full(2, "cuda")
    assert U.code_of(eng.pairs_label, labels, sizes, roots, counts=label_counts) == N.ERR_ARG
    table, total, hist_counts = U.full((n, 4), "cuda").to(torch.int32), U.full(4, "cuda"), U.full(2, "cuda")
    assert U.code_of(eng.pairs_hist, table, total, edges=[0.0, 0.01, 0.02, 0.03, 0.04], counts=hist_counts) == N.ERR_ARG
    assert U.code_of(eng.pairs_hist, table, total, edges=[0.0, 0.01, 0.02, 0.03, 0.04], queries=kw["points"],
                     counts=hist_counts) == N.ERR_ARG
    eng.synchronize()
    assert U.untouched(labels, sizes, roots, label_counts, table, total, hist_counts)
    assert counts.tolist() == [n, int(pairs_spec_of("triplets", False)[0][-1])]     # (the count itself went through)
    # the grid is still there for the readers that are batched
    partners = U.full(int(counts[1]), "cuda")
    eng.pairs_fill(partners)
    eng.synchronize()
    assert U.same_bits_on_device(partners, pairs_spec_of("triplets", False)[1])


# ---- 5. offsets out of order

def bad_cases():
    case = BK.cases()["queries"]
    return [("batch", key) for key in BK.bad_offsets(case.ptr, len(case.points))] + [
        ("query_batch", key) for key in BK.bad_offsets(case.query_ptr, len(case.queries))]


@pytest.mark.parametrize("which,key", bad_cases())
def test_offsets_out_of_order_write_nothing_and_raise(crate, which, key):
    """Through the engine: the status -3 in the counts and every output as it was.  Through the crate: ValueError."""
    import torch
    from sand_crate_amd import _native as N
    case = BK.cases()["queries"]
    n, q = len(case.points), len(case.queries)
    kw = inputs("queries", True)
    query_form = which == "query_batch"
    kw[which] = tensor(BK.bad_offsets(case.ptr, n)[key] if which == "batch" else BK.bad_offsets(case.query_ptr, q)[key])
    if not query_form:
        del kw["queries"], kw["query_batch"]
    eng = crate.engine
    values = tensor(values_of("queries", 3))
    rows = q if query_form else n
    offsets, counts = U.full(n + 1, "cuda"), U.full(2, "cuda")
    eng.pairs_count(kw["points"], radius=BK.RADIUS, offsets=offsets, counts=counts, half=True, batch=kw["batch"])
    partners, d2 = U.full(64, "cuda"), U.full(64, "cuda", U.SENTINEL_F)
    eng.pairs_fill(partners, d2)
    reader = dict(queries=kw.get("queries"), query_batch=kw.get("query_batch"))
    neighbors, nd2 = U.full((rows, 4), "cuda"), U.full((rows, 4), "cuda", U.SENTINEL_F)
    ncount, nearest_counts = U.full(rows, "cuda"), U.full(2, "cuda")
    if query_form:                                                                  # (pairs_nearest has no such keyword)
        eng.pairs_set_query_batch(kw["query_batch"])
    eng.pairs_nearest(neighbors, nd2, ncount, k=4, counts=nearest_counts, queries=reader["queries"])
    sums, wsum, sum_counts = U.full((rows, 3), "cuda", U.SENTINEL_F), U.full(rows, "cuda", U.SENTINEL_F), U.full(2, "cuda")
    eng.pairs_sum(values, sums, wsum, counts=sum_counts, **reader)
    grad, grad_counts = U.full((rows, 2), "cuda", U.SENTINEL_F), U.full(2, "cuda")
    row_a = tensor(np.ones((rows, 3)))
    eng.pairs_sum_grad(grad, row_a, values, counts=grad_counts, **reader)
    eng.synchronize()
    if query_form:                                                                  # (the count and the fill were in order)
        assert counts.tolist()[0] == n and counts.tolist()[1] >= 0 and not U.untouched(offsets)
    else:
        assert counts.tolist() == [n, N.PAIRS_BATCH] and U.untouched(offsets, partners, d2)
    assert int(nearest_counts[1]) == int(sum_counts[1]) == int(grad_counts[1]) == N.PAIRS_BATCH == -3
    assert U.untouched(neighbors, nd2, ncount, sums, wsum, grad)
    calls = [lambda: crate.neighbor_tensors(4, BK.RADIUS, **kw),
             lambda: crate.field_tensors(values, BK.RADIUS, **kw),
             lambda: crate.field_function(values, BK.RADIUS, **kw),
             lambda: crate.field_function(values.clone().requires_grad_(), BK.RADIUS, **kw)]
    if not query_form:
        calls.append(lambda: crate.pair_tensors(BK.RADIUS, points=kw["points"], batch=kw["batch"]))
    for call in calls:
        with pytest.raises(ValueError, match=BATCH_ORDER):
            call()
    # and the next call in order is served as ever
    assert same_all(crate.pair_tensors(BK.RADIUS, squared_distances=True, **inputs("queries")), pairs_spec_of("queries", False))
    assert torch.cuda.is_available()


# ---- 6. the argument errors

def test_the_setters_argument_errors(sc, crate):
    import torch
    from sand_crate_amd import _native as N
    eng = crate.engine
    kw = inputs("queries", True)
    n, q = kw["points"].shape[0], kw["queries"].shape[0]
    offsets, counts = U.full(max(n, eng.capacity) + 1, "cuda"), U.full(2, "cuda")
    lib, ctx = eng._lib, eng._ctx
    assert lib.sc_pairs_set_batch_device(ctx, N._P(kw["batch"].data_ptr()), -1) == N.ERR_ARG
    assert lib.sc_pairs_set_batch_device(None, N._P(kw["batch"].data_ptr()), 2) == N.ERR_ARG
    assert lib.sc_pairs_set_query_batch_device(None, N._P(kw["query_batch"].data_ptr())) == N.ERR_ARG
    # a pending batch and the state form: refused, and consumed -- the next state-form count goes through
    # (the raw call: `Engine.pairs_count` sets or clears the batch itself)
    state_count = lambda: lib.sc_pairs_count_device(ctx, None, 0, BK.RADIUS, 0, N._P(offsets.data_ptr()),  # noqa: E731
                                                    offsets.shape[0] - 1, N._P(counts.data_ptr()))
    eng.pairs_set_batch(kw["batch"])
    assert state_count() == N.ERR_ARG
    assert state_count() == 0
    eng.pairs_count(None, radius=BK.RADIUS, offsets=offsets, counts=counts)
    # query offsets on an unbatched grid
    assert U.code_of(eng.pairs_set_query_batch, kw["query_batch"]) == N.ERR_ARG
    eng.pairs_count(kw["points"], radius=BK.RADIUS, offsets=offsets, counts=counts)
    assert U.code_of(eng.pairs_set_query_batch, kw["query_batch"]) == N.ERR_ARG
    # a query-form reader of a batched grid without them -- each of the three -- and with them; they are consumed
    eng.pairs_count(kw["points"], radius=BK.RADIUS, offsets=offsets, counts=counts, batch=kw["batch"])
    neighbors, wsum = U.full((q, 2), "cuda"), U.full(q, "cuda", U.SENTINEL_F)
    grad, reader_counts = U.full((q, 2), "cuda", U.SENTINEL_F), U.full(2, "cuda")
    assert U.code_of(eng.pairs_nearest, neighbors, k=2, queries=kw["queries"], counts=reader_counts) == N.ERR_ARG
    assert U.code_of(eng.pairs_sum, None, None, wsum, queries=kw["queries"], counts=reader_counts) == N.ERR_ARG
    assert U.code_of(eng.pairs_sum_grad, grad, queries=kw["queries"], counts=reader_counts) == N.ERR_ARG
    eng.pairs_set_query_batch(kw["query_batch"])
    eng.pairs_nearest(neighbors, k=2, queries=kw["queries"], counts=reader_counts)
    assert U.code_of(eng.pairs_nearest, neighbors, k=2, queries=kw["queries"], counts=reader_counts) == N.ERR_ARG
    eng.synchronize()
    assert U.same_bits_on_device(neighbors, nearest_spec_of("queries", 2, True)[0]) and U.untouched(wsum, grad)
    # the wrappers' own checks, before anything is enqueued
    good, points, queries = kw["batch"], kw["points"], kw["queries"]
    wrong = [dict(points=points, batch=good.to(torch.int32)), dict(points=points, batch=good.cpu()),
             dict(points=points, batch=good.reshape(1, -1)), dict(points=points, batch=good[:1]),
             dict(points=None, batch=good),
             dict(points=points, batch=good, query_batch=kw["query_batch"]),
             dict(points=points, batch=good, queries=queries),
             dict(points=points, queries=queries, query_batch=kw["query_batch"]),
             dict(points=points, batch=good, queries=queries, query_batch=kw["query_batch"][:-1].contiguous()),
             dict(points=points, batch=good, queries=queries, query_batch=kw["query_batch"].to(torch.float64))]
    for bad in wrong:
        for call in (lambda **a: crate.neighbor_tensors(2, BK.RADIUS, **a), lambda **a: crate.field_tensors(None, BK.RADIUS, **a),
                     lambda **a: crate.field_function(None, BK.RADIUS, **a)):
            with pytest.raises(ValueError):
                call(**bad)
    for bad in wrong[:5]:
        with pytest.raises(ValueError):
            crate.pair_tensors(BK.RADIUS, **bad)
    with pytest.raises(TypeError):                                                  # (not batched yet: no such argument)
        crate.cluster_tensors(BK.RADIUS, points=points, batch=good)
    with pytest.raises(TypeError):
        crate.distance_histogram([0.0, BK.RADIUS], points=points, batch=good)


# ---- 7. the readers share one flag: no call's verdict reaches the next

def test_a_raised_reader_flag_does_not_reach_the_next_reader(crate):
    """One count of 70 points -- more than one 64-row workgroup of the nearest and of the histogram -- and 3 queries: a
    nearest call with a query outside the domain reports -1; the sum, the gradient, the histogram and a clean nearest call
    after it each report 0 and equal their NumPy rules bit for bit."""
    import torch
    import field_grad_spec
    import field_spec
    import hist_spec
    import nearest_spec
    rs = np.random.RandomState(70)
    radius, k, power = 0.1, 16, 3                                                   # (no row has 16 partners: the cut count is 0)
    points = rs.rand(70, 2) * 0.5
    queries = points[[3, 40, 69]] + 0.01
    outside = queries.copy()
    outside[1, 0] = 2.0 ** 32 * radius
    values, row_a, row_s, part_s = rs.rand(70, 3) - 0.5, rs.rand(3, 3) - 0.5, rs.rand(3) - 0.5, rs.rand(70) - 0.5
    edges = np.linspace(0.0, radius, 6)
    eng = crate.engine
    p, q, far = tensor(points), tensor(queries), tensor(outside)
    v, a, s, ps = tensor(values), tensor(row_a), tensor(row_s), tensor(part_s)
    offsets, counts = U.full(eng.capacity + 1, "cuda"), U.full(2, "cuda")
    status = [U.full(2, "cuda") for _ in range(5)]
    first, neighbors = U.full((3, k), "cuda"), U.full((3, k), "cuda")
    d2, partners = U.full((3, k), "cuda", U.SENTINEL_F), U.full(3, "cuda")
    sums, wsum, grad = U.full((3, 3), "cuda", U.SENTINEL_F), U.full(3, "cuda", U.SENTINEL_F), U.full((3, 2), "cuda", U.SENTINEL_F)
    table, total = torch.full((3, 5), U.SENTINEL, dtype=torch.int32, device="cuda"), U.full(5, "cuda")
    eng.pairs_count(p, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(first, k=k, queries=far, counts=status[0])
    eng.pairs_sum(v, sums, wsum, power=power, queries=q, counts=status[1])
    eng.pairs_sum_grad(grad, a, v, s, ps, power=power, queries=q, counts=status[2])
    eng.pairs_hist(table, total, edges=edges, queries=q, counts=status[3])
    eng.pairs_nearest(neighbors, d2, partners, k=k, queries=q, counts=status[4])
    eng.synchronize()
    assert counts.cpu().tolist()[0] == 70 and int(counts[1]) > 0
    assert status[0].cpu().tolist() == [U.SENTINEL, -1] and U.untouched(first)
    want_nearest = nearest_spec.nearest(points, radius, k, queries)
    assert [t.cpu().tolist() for t in status[1:]] == [[3, 0]] * 4 and int(want_nearest[2].max()) <= k
    assert same_all((sums, wsum), field_spec.field(points, radius, values, power, True, queries))
    assert U.same_bits_on_device(grad, field_grad_spec.position_grad(queries, points, radius, power, row_a, values, row_s,
                                                                     part_s))
    assert same_all((table, total), hist_spec.histogram(points, edges, queries))
    assert same_all((neighbors, d2, partners), want_nearest) and int(want_nearest[2].sum()) > 0
