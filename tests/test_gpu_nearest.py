"""GPU tests of the device nearest-k tables (sc_pairs_nearest_device, `Engine.pairs_nearest`, `Crate.neighbor_tensors`):
neighbors, d2, partners and counts equal tests/nearest_spec.py bit for bit -- on every case of tests/nearest_cases.py, with
and without the optional outputs, on the state after ticks, after a load and on an empty crate --, the partners equal the
pair list's row lengths, searching changes nothing, a fill and a label after the table still match their rules (also after a
query outside the domain), rows past the row count stay untouched, the domain error, the error codes, the invalidation rule
and the path that does not synchronise."""
import functools

import numpy as np
import pytest

import cluster_spec as CS
import gpu_support as U
import nearest_cases as NK
import nearest_spec as NS
import pairs_cases as K
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [name for name in NK.cases() if name != NK.OUTSIDE]


@functools.lru_cache(maxsize=None)
def spec(name):
    return NS.nearest(*NK.cases()[name])


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert U.same_bits(g, w)


def search(eng, points, radius, k, queries=None, *, optional=True, half=False, spare=8):
    """count + nearest through the engine into sentinel-filled tensors with `spare` rows of room beyond the rows ->
    (neighbors, d2, partners, counts), synchronised."""
    import torch
    dev = torch.device("cuda", eng.device)
    n = len(points)
    rows = n if queries is None else len(queries)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    neighbors = U.full((rows + spare, k), dev)
    d2 = U.full((rows + spare, k), dev, U.SENTINEL_F) if optional else None
    partners = U.full(rows + spare, dev) if optional else None
    t, q = U.tensor(points), None if queries is None else U.tensor(queries)               # (alive until the synchronisation)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
    assert eng.pairs_nearest(neighbors, d2, partners, k=k, queries=q, counts=counts) is counts
    eng.synchronize()
    return neighbors, d2, partners, counts


# ---- 1. every case, both ways in

@pytest.mark.parametrize("name", CASES)
def test_case_equals_the_spec(crate, name):
    points, radius, k, queries = NK.cases()[name]
    want = spec(name)
    rows = len(want[2])
    q = None if queries is None else U.tensor(queries)
    got = crate.neighbor_tensors(k, radius, points=U.tensor(points), queries=q, squared_distances=True, partner_counts=True)
    assert all(t.is_cuda for t in got)
    assert_same(got, want)
    cut = int((want[2] > k).sum())
    for optional in (True, False):
        neighbors, d2, partners, counts = search(crate.engine, points, radius, k, queries, optional=optional,
                                                 half=not optional)
        assert counts.cpu().tolist() == [rows, cut]
        assert U.same_bits(neighbors[:rows], want[0]) and U.untouched(neighbors[rows:])
        if optional:
            assert U.same_bits(d2[:rows], want[1]) and U.same_bits(partners[:rows], want[2]) and \
                U.untouched(d2[rows:], partners[rows:])
    assert_same(crate.neighbor_tensors(k, radius, points=U.tensor(points), queries=q), want[:1])


# ---- 2. the domain

def test_query_outside_the_domain_leaves_the_count_as_it_was(crate):
    import torch
    points, radius, k, queries = NK.cases()[NK.OUTSIDE]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    t, q = U.tensor(points), U.tensor(queries)
    with pytest.raises(ValueError, match="domain"):
        crate.neighbor_tensors(k, radius, points=t, queries=q)
    n = len(points)
    want = S.pairs(points, radius)
    offsets, counts, other = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    neighbors, partners = U.full((len(queries), k), dev), U.full(len(queries), dev)
    d2 = U.full((len(queries), k), dev, U.SENTINEL_F)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(neighbors, d2, partners, k=k, queries=q, counts=other)
    pair_j, pair_d2 = U.full(len(want[1]), dev), U.full(len(want[1]), dev, U.SENTINEL_F)
    labels, label_counts = U.full(n, dev), U.full(2, dev)
    eng.pairs_fill(pair_j, pair_d2)                                                 # the count's flag is still down
    eng.pairs_label(labels, counts=label_counts)
    table, table_counts = U.full((n, k), dev), U.full(2, dev)
    eng.pairs_nearest(table, k=k, counts=table_counts)                              # ... and so is the next table's own
    eng.synchronize()
    assert other.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(neighbors, d2, partners)
    assert counts.cpu().tolist() == [n, len(want[1])]
    assert_same((offsets, pair_j, pair_d2), want)
    clusters = CS.clusters(points, radius)
    assert U.same_bits(labels, clusters[0]) and label_counts.cpu().tolist() == [n, len(clusters[1])]
    self_want = NS.nearest(points, radius, k)
    assert U.same_bits(table, self_want[0]) and table_counts.cpu().tolist() == [n, int((self_want[2] > k).sum())]
    out = crate.neighbor_tensors(k, radius, points=t, queries=q, sync=False)
    crate.synchronize()
    assert int(out[-1][1]) == -1


def test_point_outside_the_domain(crate):
    points, radius = K.outside_domain()
    with pytest.raises(ValueError, match="domain"):
        crate.neighbor_tensors(4, radius, points=U.tensor(points))
    for queries in (None, np.array([[0.5, 0.5], [0.25, 0.75]])):
        neighbors, d2, partners, counts = search(crate.engine, points, radius, 4, queries)
        rows = len(points)                                                           # (counts[0] is the count's n)
        assert counts.cpu().tolist() == [rows, -1] and U.untouched(neighbors, d2, partners)


# ---- 3. the state form

def test_state_after_ticks_after_a_load_and_with_queries(sc):
    import torch
    from sand_crate_amd import pairs
    first = sc.Crate(U.scene(sc))
    for _ in range(40):
        first.physics_tick()
    particles, velocities = first.state_tensors(pressure=False)
    n = len(particles)
    assert n > 100
    points = particles.cpu().numpy()
    for k, factor in ((3, 1.0), (16, 1.0), (33, 2.0)):
        radius = factor * first.diameter
        got = first.neighbor_tensors(k, None if factor == 1.0 else radius, squared_distances=True, partner_counts=True)
        want = NS.nearest(points, radius, k)
        assert_same(got, want)
        offsets, partners = first.pair_tensors(radius)
        assert torch.equal(got[2], pairs.row_lengths(offsets))                      # the uncapped row lengths
        whole = got[2] <= k
        edges = pairs.neighbor_edge_index(got[0])
        assert int(pairs.neighbor_mask(got[0]).sum()) == edges.shape[1] == int(got[2].clamp(max=k).sum())
        assert bool(whole.any()) and int(edges[1].max()) < n
    assert first.particle_count == n
    rs = np.random.RandomState(5)
    lo, hi = points.min(axis=0), points.max(axis=0)
    queries = lo + (hi - lo) * rs.rand(200, 2)
    queries[::10] = points[rs.choice(n, 20, replace=False)]
    got = first.neighbor_tensors(5, queries=U.tensor(queries), squared_distances=True, partner_counts=True)
    assert_same(got, NS.nearest(points, first.diameter, 5, queries))
    assert first.particle_count == n
    ids = torch.from_numpy(np.random.RandomState(7).permutation(n) * 3 + 5).cuda()  # row k gets id ids[k]: sparse, shuffled
    torch.cuda.synchronize()
    other = sc.Crate(U.scene(sc), noise="none", capacity=n + 100)
    other.load_state_tensors(particles, velocities, ids)
    order = np.argsort(ids.cpu().numpy())
    got = other.neighbor_tensors(17, squared_distances=True, partner_counts=True)
    assert_same(got, NS.nearest(points[order], other.diameter, 17))                 # rows of that export
    assert other.particle_count == n


def test_state_of_an_empty_crate(sc):
    crate = sc.Crate(U.scene(sc))
    neighbors, d2, partners = crate.neighbor_tensors(4, squared_distances=True, partner_counts=True)   # before the first tick
    assert neighbors.shape == d2.shape == (0, 4) and partners.shape == (0,)
    out = crate.neighbor_tensors(4, sync=False)
    crate.synchronize()
    assert out[-1].cpu().tolist() == [0, 0]
    queries = np.array([[0.5, 0.5], [np.nan, 1.0]])
    got = crate.neighbor_tensors(2, queries=U.tensor(queries), squared_distances=True, partner_counts=True)
    assert_same(got, NS.nearest(np.zeros((0, 2)), crate.diameter, 2, queries))


def test_searching_changes_nothing(sc):
    def trajectory(searching):
        crate = sc.Crate(U.scene(sc))
        probes = U.tensor(np.random.RandomState(9).rand(50, 2)) if searching else None
        for _ in range(30):
            crate.physics_tick()
            if searching:
                crate.neighbor_tensors(16)
                crate.neighbor_tensors(3, 2 * crate.diameter, queries=probes, sync=False)
        state = crate.engine.download()
        crate.sync_host_rng()
        rng = np.random.get_state()
        return state, (rng[1].copy(), rng[2])

    (a, rng_a), (b, rng_b) = trajectory(False), trajectory(True)
    assert len(a[0]) > 100
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(rng_a[0], rng_b[0]) and rng_a[1] == rng_b[1]


# ---- 4. the workspace is left as it is

@pytest.mark.parametrize("half", [False, True])
def test_a_fill_and_a_label_after_the_table_still_match(crate, half):
    import torch
    name = next(n for n in NK.cases() if n.startswith("long_rows"))
    points, radius, _, _ = NK.cases()[name]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n, k = len(points), 5
    want = S.pairs(points, radius, half)
    clusters = CS.clusters(points, radius)
    table = NS.nearest(points, radius, k)
    offsets, counts, other, third = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev), U.full(2, dev)
    neighbors, again, labels = U.full((n, k), dev), U.full((n, k), dev), U.full(n, dev)
    partners, d2 = U.full(len(want[1]), dev), U.full(len(want[1]), dev, U.SENTINEL_F)
    queries = U.tensor(points[:40] + 0.25 * radius)
    probes = U.full((40, k), dev)
    t = U.tensor(points)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
    eng.pairs_nearest(neighbors, k=k, counts=other)
    eng.pairs_nearest(probes, k=k, queries=queries, counts=third)
    eng.pairs_fill(partners, d2)
    eng.pairs_label(labels, counts=third)
    eng.pairs_nearest(again, k=k, counts=third)                                     # ... and repeated
    eng.synchronize()
    assert counts.cpu().tolist() == [n, len(want[1])] and other.cpu().tolist() == [n, int((table[2] > k).sum())]
    assert_same((offsets, partners, d2), want)
    assert U.same_bits(labels, clusters[0])
    assert U.same_bits(neighbors, table[0]) and U.same_bits(again, table[0]) and third.cpu().tolist() == other.cpu().tolist()
    assert U.same_bits(probes, NS.nearest(points, radius, k, points[:40] + 0.25 * radius)[0])


# ---- 5. rows past the row count

def test_rows_past_the_row_count_are_untouched(sc):
    import torch
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    crate.particles = points
    room, k = eng.capacity, 17
    offsets, counts = U.full(room + 1, dev), U.full(2, dev)
    neighbors, d2, partners = U.full((room, k), dev), U.full((room, k), dev, U.SENTINEL_F), U.full(room, dev)
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(neighbors, d2, partners, k=k, counts=counts)
    eng.synchronize()
    want = NS.nearest(points, radius, k)
    n = len(points)
    assert counts.cpu().tolist() == [n, int((want[2] > k).sum())]
    assert_same((neighbors[:n], d2[:n], partners[:n]), want)
    assert U.untouched(neighbors[n:], d2[n:], partners[n:])


# ---- 6. errors

def test_state_errors_and_the_invalidation_rule(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    t = U.tensor(points)
    k = 4
    offsets = torch.zeros(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    neighbors, out = U.full((eng.capacity, k), dev), U.full(2, dev)
    torch.cuda.synchronize()
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, counts=out) == N.ERR_STATE    # no count yet
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, queries=t, counts=out) == N.ERR_STATE
    eng.synchronize()
    assert U.untouched(neighbors, out)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(neighbors, k=k, counts=out)                                   # ... with one: fine, and again
    eng.pairs_nearest(neighbors, k=k, queries=t, counts=out)
    crate.particles = points                                                        # an upload since the count
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, counts=out) == N.ERR_STATE
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(neighbors, k=k, counts=out)
    eng.append(points[:3] + 2.0, np.zeros((3, 2)))                                  # an append since the count
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, counts=out) == N.ERR_STATE
    crate.particles = points
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_nearest(neighbors, k=k, counts=out)
    crate.physics_tick()                                                            # a tick since the count
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, counts=out) == N.ERR_STATE
    assert U.code_of(eng.pairs_nearest, neighbors, k=k, queries=t, counts=out) == N.ERR_STATE
    eng.synchronize()
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    crate._send_tick_inputs()                                                       # inside a tick
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_nearest, neighbors, k=k, counts=out) == N.ERR_STATE
    finally:
        eng.step_finish()


def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n, k = 300, 6
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points = np.random.RandomState(3).rand(n, 2)
    t = U.tensor(points)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    neighbors, d2, partners, out = U.full((n, k), dev), U.full((n, k), dev, U.SENTINEL_F), U.full(n, dev), U.full(2, dev)
    torch.cuda.synchronize()
    eng.pairs_count(t, radius=0.05, offsets=offsets, counts=counts)
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_nearest_device
    args = lambda **kw: tuple({**dict(ctx=ctx, q=None, nq=0, k=k, nb=ptr(neighbors), d2=ptr(d2), p=ptr(partners), room=n,  # noqa: E731
                                      counts=ptr(out)), **kw}.values())
    assert fn(*args(ctx=None)) == N.ERR_ARG
    assert fn(*args(nb=None)) == N.ERR_ARG
    assert fn(*args(counts=None)) == N.ERR_ARG
    for bad in (0, -1, N.NEAREST_MAX_K + 1):
        assert fn(*args(k=bad)) == N.ERR_ARG
    assert fn(*args(room=-1)) == N.ERR_ARG
    assert fn(*args(q=ptr(t), nq=-1)) == N.ERR_ARG
    assert fn(*args(q=N._P(t.data_ptr() + 8), nq=n - 1)) == N.ERR_ARG               # misaligned queries
    assert fn(*args(room=n - 1)) == N.ERR_CAPACITY                                  # short table, self form
    assert fn(*args(q=ptr(t), nq=n, room=n - 1)) == N.ERR_CAPACITY                  # ... and for the queries
    assert fn(*args(q=ptr(t), nq=(1 << 28) + 1, room=(1 << 28) + 1)) == N.ERR_CAPACITY
    assert U.code_of(eng.pairs_nearest, neighbors[:n - 1], k=k, counts=out) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    eng.synchronize()
    assert U.untouched(neighbors, d2, partners, out)
    assert fn(*args(d2=None, p=None)) == 0                                          # without the optional outputs: fine
    assert fn(*args(q=ptr(t), nq=10, room=10)) == 0                                 # fewer queries than points: fine
    eng.synchronize()
    want = NS.nearest(points, 0.05, k, points[:10])
    assert_same((neighbors[:10], d2[:10], partners[:10]), want)
    assert U.untouched(d2[10:], partners[10:])
    eng.close()


# ---- 7. the path that does not synchronise

def test_sync_false_does_not_synchronise_and_equals_the_default(crate, monkeypatch):
    import torch
    points, radius, k, queries = NK.cases()["q_300"]
    t, q = U.tensor(points), U.tensor(queries)

    def forbidden(*args, **kw):
        raise AssertionError("the call synchronised")

    for probes in (None, q):
        want = crate.neighbor_tensors(k, radius, points=t, queries=probes, squared_distances=True, partner_counts=True)
        rows = len(want[0])
        with monkeypatch.context() as m:
            m.setattr(type(crate.engine), "synchronize", forbidden)
            m.setattr(torch.cuda, "synchronize", forbidden)
            m.setattr(torch.cuda.Stream, "synchronize", forbidden)
            m.setattr(torch.Tensor, "item", forbidden)
            m.setattr(torch.Tensor, "cpu", forbidden)
            out = crate.neighbor_tensors(k, radius, points=t, queries=probes, squared_distances=True, partner_counts=True,
                                         sync=False)
        crate.synchronize()
        assert len(out) == 4 and out[3].cpu().tolist() == [rows, int((want[2] > k).sum())]
        assert all(torch.equal(a, b) for a, b in zip(out[:3], want))
    with pytest.raises(ValueError, match="k must be"):
        crate.neighbor_tensors(65, radius, points=t)
