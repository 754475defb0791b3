"""GPU tests of the batched clusters, cluster sums, histograms, rays and ray paths (`Crate.cluster_tensors_batch`,
`cluster_sums_batch`, `distance_histogram_batch`, `ray_tensors(batch=, ray_batch=)`, `ray_paths(batch=, ray_batch=)`;
sc_pairs_label_batch_device, sc_pairs_hist_batch_device, sc_pairs_rays_batch_device, sc_pairs_ray_paths_batch_device):
every result against the rule of tests/batch_readers_spec.py -- the existing rules cloud by cloud -- bit for bit or as
exact integers, on the cases of tests/batch_readers_cases.py, whose own promises tests/test_batch_readers_cpu.py proves."""
import functools

import numpy as np
import pytest

import batch_cases as BK
import batch_readers_cases as RK
import batch_readers_spec as RS
import gpu_support as U
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

BATCH_ORDER = "batch offsets must start at 0, not descend and end at the number of points"
ALL_RAY_CASES = RK.RAY_CASES + RK.POINT_CASES


def tensor(a, tail=None):
    """A CUDA copy of `a` in its own dtype (the offsets are int64), synchronised; None gives None."""
    import torch
    if a is None:
        return None
    a = np.array(a)                                                                 # (a copy: the cases are read-only)
    t = torch.from_numpy(a if tail is None else a.reshape(-1, tail)).cuda()
    torch.cuda.synchronize()
    return t


def same_all(got, want):
    return len(got) == len(want) and all(U.same_bits_on_device(g, w) for g, w in zip(got, want))


def same_paths(got, want):
    """t, hit, points, normals, end: where the rule has a NaN any NaN will do, everything else bit for bit."""
    return len(got) == len(want) == 5 and all(
        U.same_bits_or_nan(g, w) if w.dtype == np.float64 else U.same_bits_on_device(g, w) for g, w in zip(got, want))


def host(tensors):
    return [t.cpu().numpy() for t in tensors]


def inputs(name, query_form=False):
    case = RK.cases()[name]
    kw = dict(points=tensor(case.points, 2), batch=tensor(case.ptr))
    if query_form:
        kw.update(queries=tensor(case.queries, 2), query_batch=tensor(case.query_ptr))
    return kw


def ray_case(name):
    return RK.ray_cases()[name] if name in RK.RAY_CASES else RK.rays_of(name)


def ray_inputs(name):
    """-> (origins, directions, max_t), the keyword arguments of `ray_tensors` / `ray_paths` for a case."""
    case = ray_case(name)
    return (tensor(case.origins, 2), tensor(case.directions, 2), case.max_t), dict(
        disc_radius=case.rho, walls=case.walls, points=tensor(case.points, 2), batch=tensor(case.ptr), ray_batch=tensor(case.ray_ptr))


@functools.lru_cache(maxsize=None)
def values_of(name, width=3):
    v = np.random.RandomState(57 + width).rand(len(RK.cases()[name].points), width) - 0.5
    v.setflags(write=False)
    return v


def edges_of(bins):
    return np.linspace(0.0, RK.RADIUS, bins + 1)


@functools.lru_cache(maxsize=None)
def sums_spec_of(name):
    case = RK.cases()[name]
    return RS.cluster_sums(case.points, case.radius, case.ptr, values_of(name), extrema=True)


def clusters_spec_of(name):
    labels, sizes, roots, *_, cptr = sums_spec_of(name)
    return labels, sizes, roots, cptr


@functools.lru_cache(maxsize=None)
def hist_spec_of(name, bins, query_form):
    case = RK.cases()[name]
    return RS.histogram(case.points, edges_of(bins), case.ptr, *((case.queries, case.query_ptr) if query_form else ()))


@functools.lru_cache(maxsize=None)
def rays_spec_of(name):
    c = ray_case(name)
    return RS.rays(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.ptr, c.ray_ptr)


@functools.lru_cache(maxsize=None)
def paths_spec_of(name, bounces):
    c = ray_case(name)
    return RS.paths(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, bounces, c.ptr, c.ray_ptr)


# ---- 1. the five calls against the rule

@pytest.mark.parametrize("name", RK.POINT_CASES)
def test_cluster_tensors_batch_is_the_per_cloud_rule(crate, name):
    got = crate.cluster_tensors_batch(RK.RADIUS, **inputs(name))
    assert same_all(got, clusters_spec_of(name))


@pytest.mark.parametrize("name", RK.POINT_CASES)
def test_cluster_sums_is_the_per_cloud_rule(crate, name):
    import cluster_sums_spec
    got = crate.cluster_sums_batch(tensor(values_of(name)), RK.RADIUS, extrema=True, **inputs(name))
    want = sums_spec_of(name)
    assert len(got) == len(want) == 7
    assert all(cluster_sums_spec.same(g, w) for g, w in zip(host(got), want))
    got = crate.cluster_sums_batch(tensor(values_of(name)), RK.RADIUS, **inputs(name))    # ... and the sums alone
    assert all(cluster_sums_spec.same(g, w) for g, w in zip(host(got), want[:4] + want[6:])) and len(got) == 5


@pytest.mark.parametrize("bins", RK.HIST_BINS)
@pytest.mark.parametrize("name", RK.POINT_CASES)
def test_distance_histogram_batch_is_the_per_cloud_rule(crate, name, bins):
    for query_form in ((False, True) if name in RK.QUERY_CASES else (False,)):
        table, total = hist_spec_of(name, bins, query_form)
        kw = inputs(name, query_form)
        assert same_all(crate.distance_histogram_batch(edges_of(bins), per_row=True, **kw), (table, total)), query_form
        assert same_all(crate.distance_histogram_batch(edges_of(bins), **kw), (total,)), query_form
        assert same_all(crate.distance_histogram_batch(edges_of(bins), per_row=True, totals=False, **kw), (table,)), query_form


@pytest.mark.parametrize("name", ALL_RAY_CASES)
def test_ray_tensors_is_the_per_cloud_rule(crate, name):
    args, kw = ray_inputs(name)
    got = crate.ray_tensors(*args, **kw)
    want = rays_spec_of(name)
    assert U.same_values_signs(got[0], want[0]) and U.same_bits_on_device(got[1], want[1])


@pytest.mark.parametrize("bounces", RK.BOUNCES)
@pytest.mark.parametrize("name", ALL_RAY_CASES)
def test_ray_paths_is_the_per_cloud_rule(crate, name, bounces):
    args, kw = ray_inputs(name)
    assert same_paths(crate.ray_paths(*args, bounces, **kw), paths_spec_of(name, bounces))


# ---- 2. one cloud, the forms that do not synchronise, twice and for two capacities

def test_one_cloud_equals_the_unbatched_call(crate):
    import torch
    case = BK.cases()["single"]
    points, one = tensor(case.points, 2), tensor(case.ptr)
    values = tensor(np.random.RandomState(5).rand(len(case.points), 3) - 0.5)
    a = crate.cluster_tensors_batch(BK.RADIUS, points=points, batch=one)
    b = crate.cluster_tensors(BK.RADIUS, points=points)
    assert same_all(a[:3], host(b)) and a[3].tolist() == [0, len(b[1])]
    a = crate.cluster_sums_batch(values, BK.RADIUS, extrema=True, points=points, batch=one)
    b = crate.cluster_sums(values, BK.RADIUS, extrema=True, points=points)
    assert same_all(a[:6], host(b)) and a[6].tolist() == [0, len(b[1])]
    a = crate.distance_histogram_batch(edges_of(17), per_row=True, points=points, batch=one)
    b = crate.distance_histogram(edges_of(17), per_row=True, points=points)
    assert same_all((a[0], a[1][0]), host(b)) and a[1].shape == (1, 17)
    rays = RK.rays_of("collisions")
    o, d = tensor(rays.origins, 2), tensor(rays.directions, 2)
    lone = torch.tensor([0, len(rays.origins)], dtype=torch.int64, device="cuda")
    kw = dict(disc_radius=BK.RADIUS / 2, walls=rays.walls, points=points)
    a = crate.ray_tensors(o, d, rays.max_t, batch=one, ray_batch=lone, **kw)
    assert same_all(a, host(crate.ray_tensors(o, d, rays.max_t, **kw)))
    a = crate.ray_paths(o, d, rays.max_t, 3, batch=one, ray_batch=lone, **kw)
    assert same_all(a, host(crate.ray_paths(o, d, rays.max_t, 3, **kw)))


def test_the_forms_that_do_not_synchronise_equal_the_default(crate):
    import cluster_sums_spec
    name = "hist_blocks"
    case = RK.cases()[name]
    n, q = len(case.points), len(case.queries)
    labels, sizes, roots, sums, mins, maxs, cptr = sums_spec_of(name)
    C = len(sizes)
    for K in (C + 5, C - 3):                                                        # room to spare, and clipped
        *got, counts = crate.cluster_tensors_batch(RK.RADIUS, max_clusters=K, **inputs(name))
        crate.synchronize()
        k = min(K, C)
        assert counts.tolist() == [n, C] and len(got) == 4 and got[1].shape[0] == K
        assert same_all((got[0], got[1][:k], got[2][:k], got[3]), (labels, sizes[:k], roots[:k], cptr))   # cluster_ptr is whole
        *got, counts = crate.cluster_sums_batch(tensor(values_of(name)), RK.RADIUS, extrema=True, max_clusters=K, **inputs(name))
        crate.synchronize()
        assert counts.tolist() == [n, C] and len(got) == 7
        cut = [got[0]] + [t[:k] for t in got[1:6]] + [got[6]]
        assert all(cluster_sums_spec.same(g, w) for g, w in zip(host(cut), (labels, sizes[:k], roots[:k], sums[:k], mins[:k], maxs[:k], cptr)))
    for query_form in (False, True):
        rows = q if query_form else n
        table, total, counts = crate.distance_histogram_batch(edges_of(16), per_row=True, sync=False, **inputs(name, query_form))
        crate.synchronize()
        assert counts.tolist() == [rows, 0] and same_all((table[:rows], total), hist_spec_of(name, 16, query_form))
    args, kw = ray_inputs(name)
    rays = len(ray_case(name).origins)
    t, hit, counts = crate.ray_tensors(*args, sync=False, **kw)
    crate.synchronize()
    assert counts.tolist() == [rays, 0] and U.same_values_signs(t, rays_spec_of(name)[0]) and U.same_bits_on_device(hit, rays_spec_of(name)[1])
    *got, counts = crate.ray_paths(*args, 3, sync=False, **kw)
    crate.synchronize()
    assert counts.tolist() == [rays, 0] and same_paths(got, paths_spec_of(name, 3))


def test_the_same_result_twice_and_for_two_capacities(sc, crate):
    other = sc.Crate(U.scene(sc), noise="none", capacity=4096)
    name = "collisions"
    args, kw = ray_inputs(name)
    runs = [[c.cluster_sums_batch(tensor(values_of(name)), RK.RADIUS, extrema=True, **inputs(name)),
             c.distance_histogram_batch(edges_of(17), per_row=True, **inputs(name)),
             c.ray_tensors(*args, **kw), tuple(c.ray_paths(*args, 3, **kw))] for c in (crate, crate, other)]
    for later in runs[1:]:
        for a, b in zip(runs[0], later):
            assert len(a) == len(b) and all(U.same_bits_or_nan(x, y.cpu().numpy()) for x, y in zip(a, b))
    other.engine.close()


# ---- 3. the batch is consumed; the label feeds the sums

def test_a_batch_is_consumed_by_its_call(crate):
    name = "neighbours_in_index"
    case = RK.cases()[name]
    kw = inputs(name)
    points, values = kw["points"], tensor(values_of(name))
    rays = RK.rays_of(name)
    o, d = tensor(rays.origins, 2), tensor(rays.directions, 2)
    ray_kw = dict(disc_radius=rays.rho, walls=rays.walls, points=points)
    plain = [lambda: crate.cluster_tensors(RK.RADIUS, points=points),
             lambda: crate.cluster_sums(values, RK.RADIUS, extrema=True, points=points),
             lambda: crate.distance_histogram(edges_of(16), per_row=True, points=points),
             lambda: crate.ray_tensors(o, d, rays.max_t, **ray_kw),
             lambda: tuple(crate.ray_paths(o, d, rays.max_t, 1, **ray_kw))]
    batched = [lambda: crate.cluster_tensors_batch(RK.RADIUS, **kw),
               lambda: crate.cluster_sums_batch(values, RK.RADIUS, extrema=True, **kw),
               lambda: crate.distance_histogram_batch(edges_of(16), per_row=True, **kw),
               lambda: crate.ray_tensors(o, d, rays.max_t, batch=kw["batch"], ray_batch=tensor(rays.ray_ptr), **ray_kw),
               lambda: crate.ray_paths(o, d, rays.max_t, 1, batch=kw["batch"], ray_batch=tensor(rays.ray_ptr), **ray_kw)]
    before = [host(call()) for call in plain]
    assert len(before[0][1]) < len(clusters_spec_of(name)[1])                       # (unbatched, the clouds hang together)
    for with_batch in batched:
        with_batch()
        for call, want in zip(plain, before):
            assert all(U.same_bits_or_nan(g, w) for g, w in zip(call(), want))


def test_a_batched_label_feeds_the_cluster_sums(crate):
    import cluster_sums_spec
    from sand_crate_amd import _native as N
    name = "long_chain"
    case = RK.cases()[name]
    n = len(case.points)
    eng = crate.engine
    kw = inputs(name)
    values = tensor(values_of(name))
    labels, sizes, roots, sums, mins, maxs, cptr = sums_spec_of(name)
    offsets, counts = U.full(n + 1, "cuda"), U.full(2, "cuda")
    got = [U.full((len(sizes), 3), "cuda", U.SENTINEL_F) for _ in range(3)]
    sum_counts = U.full(2, "cuda")
    eng.pairs_count(kw["points"], radius=RK.RADIUS, offsets=offsets, counts=counts, batch=kw["batch"])
    assert U.code_of(eng.pairs_cluster_sums, values, *got, counts=sum_counts) == N.ERR_STATE    # a batched count, no label yet
    out = [U.full(n, "cuda"), U.full(len(sizes), "cuda"), U.full(len(sizes), "cuda")]
    ptr_out, label_counts = U.full(len(case.ptr), "cuda"), U.full(2, "cuda")
    eng.pairs_label_batch(*out, cluster_ptr=ptr_out, counts=label_counts)
    eng.pairs_cluster_sums(values, *got, counts=sum_counts)
    eng.synchronize()
    assert label_counts.tolist() == sum_counts.tolist() == [n, len(sizes)]
    assert same_all(out + [ptr_out], (labels, sizes, roots, cptr))
    assert all(cluster_sums_spec.same(g, w) for g, w in zip(host(got), (sums, mins, maxs)))


# ---- 4. the entry points on the wrong grid

def test_the_new_entry_points_refuse_an_unbatched_grid(crate):
    import torch
    from sand_crate_amd import _native as N
    name = "neighbours_in_index"
    case = RK.cases()[name]
    n, B = len(case.points), len(case.ptr) - 1
    eng = crate.engine
    lib = eng._lib
    kw = inputs(name)
    rays = RK.rays_of(name)
    o, d, rptr = tensor(rays.origins, 2), tensor(rays.directions, 2), tensor(rays.ray_ptr)
    R = len(rays.origins)
    offsets, counts = U.full(n + 1, "cuda"), U.full(2, "cuda")
    eng.pairs_count(kw["points"], radius=RK.RADIUS, offsets=offsets, counts=counts)  # unbatched
    labels, sizes, roots, cptr, out = U.full(n, "cuda"), U.full(n, "cuda"), U.full(n, "cuda"), U.full(B + 1, "cuda"), U.full(2, "cuda")
    table, total = U.full((n, 4), "cuda").to(torch.int32), U.full((B, 4), "cuda")
    t, hit = U.full(R, "cuda", U.SENTINEL_F), U.full(R, "cuda")
    legs = [U.full((R, 2), "cuda", U.SENTINEL_F), U.full((R, 2), "cuda"), U.full((R, 2, 2), "cuda", U.SENTINEL_F),
            U.full((R, 2, 2), "cuda", U.SENTINEL_F), U.full(R, "cuda")]
    edges = [0.0, 0.01, 0.02, 0.03, 0.04]
    ray_args = dict(origins=o, directions=d, disc_radius=rays.rho, max_t=rays.max_t, segments=rays.walls, counts=out)

    def refused(call, *args, **more):
        assert U.code_of(call, *args, **more) == N.ERR_ARG and b"batched" in lib.sc_last_error()

    refused(eng.pairs_label_batch, labels, sizes, roots, cluster_ptr=cptr, counts=out)
    refused(eng.pairs_hist_batch, table, total, edges=edges, counts=out)
    refused(eng.pairs_rays_batch, t, hit, ray_batch=None, **ray_args)
    refused(eng.pairs_ray_paths_batch, *legs, ray_batch=None, bounces=1, **ray_args)
    assert U.code_of(eng.pairs_set_query_batch, rptr) == N.ERR_ARG                   # (no batched grid to give offsets to)
    eng.synchronize()
    assert U.untouched(labels, sizes, roots, cptr, out, table, total, t, hit, *legs)
    # a null context comes first; on a batched grid the old four refuse and name the batch, the new four serve
    import ctypes as C
    for fn in ("sc_pairs_label_batch_device", "sc_pairs_hist_batch_device", "sc_pairs_rays_batch_device",
               "sc_pairs_ray_paths_batch_device"):
        rest = [0.0 if kind is C.c_double else 0 if kind in (C.c_int32, C.c_int64) else None for kind in N.SIGNATURES[fn][1][1:]]
        assert getattr(lib, fn)(None, *rest) == N.ERR_ARG and b"null context" in lib.sc_last_error()
    eng.pairs_count(kw["points"], radius=RK.RADIUS, offsets=offsets, counts=counts, batch=kw["batch"])
    refused(eng.pairs_label, labels, sizes, roots, counts=out)
    refused(eng.pairs_hist, table, total[0], edges=edges, counts=out)
    refused(eng.pairs_rays, t, hit, **ray_args)
    refused(eng.pairs_ray_paths, *legs, bounces=1, **ray_args)
    refused(eng.pairs_rays_batch, t, hit, ray_batch=None, **ray_args)                # the rays of a batched grid need their offsets
    assert U.code_of(eng.pairs_hist_batch, table, total[:B - 1], edges=edges, counts=out) == N.ERR_CAPACITY   # too few clouds of room
    eng.synchronize()
    assert U.untouched(labels, sizes, roots, cptr, out, table, total, t, hit, *legs)
    eng.pairs_rays_batch(t, hit, ray_batch=rptr, **ray_args)
    eng.synchronize()
    want = RS.rays(rays.points, rays.walls, rays.origins, rays.directions, rays.rho, rays.max_t, rays.ptr, rays.ray_ptr)
    assert U.same_values_signs(t, want[0]) and U.same_bits_on_device(hit, want[1]) and out.tolist() == [R, 0]


# ---- 5. offsets out of order

def bad_cases():
    case = RK.cases()["hist_blocks"]
    rays = RK.rays_of("hist_blocks")
    return [("batch", key) for key in BK.bad_offsets(case.ptr, len(case.points))] + [
        ("query_batch", key) for key in BK.bad_offsets(case.query_ptr, len(case.queries))] + [
        ("ray_batch", key) for key in BK.bad_offsets(rays.ray_ptr, len(rays.origins))]


@pytest.mark.parametrize("which,key", bad_cases())
def test_offsets_out_of_order_write_nothing_and_raise(crate, which, key):
    """Through the engine: the status -3 in the counts and every output as it was.  Through the crate: ValueError."""
    import torch
    from sand_crate_amd import _native as N
    name = "hist_blocks"
    case, rays = RK.cases()[name], RK.rays_of(name)
    n, q, R, B = len(case.points), len(case.queries), len(rays.origins), len(case.ptr) - 1
    good = dict(batch=case.ptr, query_batch=case.query_ptr, ray_batch=rays.ray_ptr)
    rows = dict(batch=n, query_batch=q, ray_batch=R)
    off = {k: tensor(BK.bad_offsets(v, rows[k])[key] if k == which else v) for k, v in good.items()}
    points, queries, values = tensor(case.points, 2), tensor(case.queries, 2), tensor(values_of(name))
    o, d = tensor(rays.origins, 2), tensor(rays.directions, 2)
    eng = crate.engine
    offsets, counts = U.full(n + 1, "cuda"), U.full(2, "cuda")
    eng.pairs_count(points, radius=RK.RADIUS, offsets=offsets, counts=counts, batch=off["batch"])
    status = {k: U.full(2, "cuda") for k in ("label", "hist", "hist_q", "rays", "paths")}
    labels, sizes, roots, cptr = U.full(n, "cuda"), U.full(n, "cuda"), U.full(n, "cuda"), U.full(B + 1, "cuda")
    table, total = U.full((n, 16), "cuda").to(torch.int32), U.full((B, 16), "cuda")
    table_q, total_q = U.full((q, 16), "cuda").to(torch.int32), U.full((B, 16), "cuda")
    t, hit = U.full(R, "cuda", U.SENTINEL_F), U.full(R, "cuda")
    legs = [U.full((R, 2), "cuda", U.SENTINEL_F), U.full((R, 2), "cuda"), U.full((R, 2, 2), "cuda", U.SENTINEL_F),
            U.full((R, 2, 2), "cuda", U.SENTINEL_F), U.full(R, "cuda")]
    ray_args = dict(origins=o, directions=d, ray_batch=off["ray_batch"], disc_radius=rays.rho, max_t=rays.max_t, segments=rays.walls)
    eng.pairs_label_batch(labels, sizes, roots, cluster_ptr=cptr, counts=status["label"])
    eng.pairs_hist_batch(table, total, edges=edges_of(16), counts=status["hist"])
    eng.pairs_hist_batch(table_q, total_q, edges=edges_of(16), queries=queries, query_batch=off["query_batch"], counts=status["hist_q"])
    eng.pairs_rays_batch(t, hit, counts=status["rays"], **ray_args)
    eng.pairs_ray_paths_batch(*legs, bounces=1, counts=status["paths"], **ray_args)
    eng.synchronize()
    hurt = dict(batch=("label", "hist", "hist_q", "rays", "paths"), query_batch=("hist_q",), ray_batch=("rays", "paths"))[which]
    for k, got in status.items():
        assert (int(got[1]) == N.PAIRS_BATCH) if k in hurt else (int(got[1]) >= 0), k
    held = dict(label=(labels, sizes, roots, cptr), hist=(table, total), hist_q=(table_q, total_q), rays=(t, hit), paths=legs)
    for k in status:
        assert U.untouched(*held[k]) == (k in hurt), k
    assert N.PAIRS_BATCH == -3
    kw = dict(points=points, batch=off["batch"])
    ray_kw = dict(disc_radius=rays.rho, walls=rays.walls, ray_batch=off["ray_batch"], **kw)
    calls = dict(batch=[lambda: crate.cluster_tensors_batch(RK.RADIUS, **kw), lambda: crate.cluster_sums_batch(values, RK.RADIUS, **kw),
                        lambda: crate.distance_histogram_batch(edges_of(16), **kw)],
                 query_batch=[lambda: crate.distance_histogram_batch(edges_of(16), queries=queries, query_batch=off["query_batch"], **kw)],
                 ray_batch=[lambda: crate.ray_tensors(o, d, rays.max_t, **ray_kw), lambda: crate.ray_paths(o, d, rays.max_t, 1, **ray_kw)])
    for call in calls[which] + (calls["query_batch"] + calls["ray_batch"] if which == "batch" else []):
        with pytest.raises(ValueError, match=BATCH_ORDER):
            call()
    # and the next call in order is served as ever
    assert same_all(crate.cluster_tensors_batch(RK.RADIUS, **inputs(name)), clusters_spec_of(name))


# ---- 6. the wrappers' own checks, before anything is enqueued

def test_the_argument_errors(crate):
    import torch
    name = "hist_blocks"
    case, rays = RK.cases()[name], RK.rays_of(name)
    kw = inputs(name, True)
    points, queries, good, qgood = kw["points"], kw["queries"], kw["batch"], kw["query_batch"]
    o, d, rgood = tensor(rays.origins, 2), tensor(rays.directions, 2), tensor(rays.ray_ptr)
    values = tensor(values_of(name))
    parked = {k: id(v) for k, v in vars(crate).get("_parked", {}).items()}
    hist = lambda **a: crate.distance_histogram_batch(edges_of(4), **a)                          # noqa: E731
    fans = (lambda **a: crate.ray_tensors(o, d, 1.0, **a), lambda **a: crate.ray_paths(o, d, 1.0, 1, **a))
    for bad in (dict(points=None, batch=good), dict(points=points, batch=good.to(torch.int32)), dict(points=points, batch=good.cpu()),
                dict(points=points, batch=good[:1]), dict(points=points, batch=None)):
        for call in (lambda **a: crate.cluster_tensors_batch(RK.RADIUS, **a), lambda **a: crate.cluster_sums_batch(values, RK.RADIUS, **a),
                     hist):
            with pytest.raises(ValueError):
                call(**bad)
        if bad["batch"] is not None:                                                # (without `batch` these are the unbatched calls)
            for call in fans:
                with pytest.raises(ValueError):
                    call(ray_batch=rgood, **bad)
    # the second offsets: missing, alone, of the wrong length, of the wrong type, without their rows
    for bad in (dict(batch=good, queries=queries), dict(batch=good, queries=queries, query_batch=qgood[:-1].contiguous()),
                dict(batch=good, queries=queries, query_batch=qgood.to(torch.float64)), dict(batch=good, query_batch=qgood)):
        with pytest.raises(ValueError):
            hist(points=points, **bad)
    for bad in (dict(batch=good), dict(ray_batch=rgood), dict(batch=good, ray_batch=rgood[:-1].contiguous()),
                dict(batch=good, ray_batch=rgood.to(torch.float64))):
        for call in fans:
            with pytest.raises(ValueError):
                call(points=points, disc_radius=rays.rho, walls=rays.walls, **bad)
    assert {k: id(v) for k, v in vars(crate).get("_parked", {}).items()} == parked   # nothing was enqueued, nothing parked
