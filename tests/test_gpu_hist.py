"""GPU tests of the device distance histograms (sc_pairs_hist_device, `Engine.pairs_hist`, `Crate.distance_histogram`):
table and totals equal tests/hist_spec.py exactly -- every case of tests/hist_cases.py, in the self form and the query
form, synchronising and not --; the totals are the table's column sums, also beyond 2^32; one bin is the partner count of
the other readers; the state form after ticks and the invalidation rule; capacity independence; the domain error writes
the status and nothing else; the workspace of the count is left as it is; the half flag is ignored; a last edge below the
count's radius; the error codes."""
import functools

import numpy as np
import pytest

import gpu_support as U
import hist_cases as HK
import hist_spec as HS
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = sorted(HK.cases())


@functools.lru_cache(maxsize=None)
def spec(name, query_form):
    case = HK.cases()[name]
    return HS.histogram(case.points, case.edges, HK.queries_of(case) if query_form else case.queries)


def through_the_engine(eng, points, edges, queries=None, *, radius=None, half=False, spare=8, table=True, total=True):
    """count + histogram through the engine into sentinel-filled tensors with `spare` rows of room beyond the rows ->
    (table or None, total or None, counts), synchronised."""
    import torch
    dev = torch.device("cuda", eng.device)
    n = len(points)
    rows = n if queries is None else len(queries)
    bins = len(edges) - 1
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    tb = U.full((rows + spare, bins), dev, dtype=torch.int32) if table else None
    tt = U.full(bins, dev) if total else None
    t, q = U.tensor(points), U.tensor(queries)                                          # (alive until the synchronisation)
    eng.pairs_count(t, radius=float(edges[-1]) if radius is None else radius, offsets=offsets, counts=counts, half=half)
    assert eng.pairs_hist(tb, tt, edges=edges, queries=q, counts=out) is out
    eng.synchronize()
    return tb, tt, out


# ---- 1. every case, both forms, synchronising and not

@pytest.mark.parametrize("query_form", [False, True], ids=["self", "queries"])
@pytest.mark.parametrize("name", CASES)
def test_case_equals_the_spec(crate, name, query_form):
    import torch
    case = HK.cases()[name]
    queries = HK.queries_of(case) if query_form else case.queries
    want_table, want_total = spec(name, query_form)
    rows = len(want_table)
    points, q = U.tensor(case.points), U.tensor(queries)
    table, total = crate.distance_histogram(case.edges, points=points, queries=q, per_row=True)
    assert table.is_cuda and total.is_cuda and U.same_bits(table, want_table) and U.same_bits(total, want_total)
    assert torch.equal(total, table.sum(0))
    only, = crate.distance_histogram(case.edges, points=points, queries=q)
    assert U.same_bits(only, want_total)
    rows_only, = crate.distance_histogram(list(case.edges), points=points, queries=q, per_row=True, totals=False)
    assert U.same_bits(rows_only, want_table)
    out = crate.distance_histogram(case.edges, points=points, queries=q, per_row=True, sync=False)
    crate.synchronize()
    assert len(out) == 3 and out[2].cpu().tolist() == [rows, 0]
    assert U.same_bits(out[0][:rows], want_table) and U.same_bits(out[1], want_total)
    for half in (False, True):
        tb, tt, counts = through_the_engine(crate.engine, case.points, case.edges, queries, half=half, total=half)
        assert counts.cpu().tolist() == [rows, 0]
        assert U.same_bits(tb[:rows], want_table) and U.untouched(tb[rows:]) and (tt is None or U.same_bits(tt, want_total))


def test_totals_beyond_32_bits(sc):
    """66,000 coincident points: every row has 65,999 partners in bin 0, and the total n (n - 1) does not fit 32 bits."""
    n = HK.BEYOND_32_BITS
    want = HK.coincident_total(n)
    assert int(want[0]) > 2 ** 32
    crate = sc.Crate(U.scene(sc), noise="none", capacity=16)
    total, = crate.distance_histogram([0.0, 0.1], points=U.tensor(HK.coincident(n)))
    assert U.same_bits(total, want)


# ---- 2. one bin is what the other readers count

def test_one_bin_is_the_partner_count_of_the_table_and_the_list(crate):
    import torch
    from sand_crate_amd import pairs
    case = HK.cases()["bins_16"]
    points, radius = U.tensor(case.points), float(case.edges[-1])
    table, total = crate.distance_histogram([0.0, radius], points=points, per_row=True)
    _, partners = crate.neighbor_tensors(4, radius, points=points, partner_counts=True)
    offsets, listed = crate.pair_tensors(radius, points=points)
    assert table.shape == (300, 1) and torch.equal(table[:, 0].long(), partners)
    assert torch.equal(table[:, 0].long(), pairs.row_lengths(offsets)) and int(total[0]) == len(listed) > 0


# ---- 3. the state form

def test_state_after_ticks_and_the_stale_count(sc):
    import torch
    from sand_crate_amd import _native as N
    from sand_crate_amd import pairs
    crate = sc.Crate(U.scene(sc))
    for _ in range(50):
        crate.physics_tick()
    edges = pairs.shell_edges(3 * crate.diameter, 24)
    table, total = crate.distance_histogram(edges, per_row=True)
    particles, = crate.state_tensors(pressure=False)[:1]
    n = len(particles)
    assert n > 100 and crate.particle_count == n and table.shape == (n, 24)
    as_points = crate.distance_histogram(edges, points=particles, per_row=True)
    assert torch.equal(table, as_points[0]) and torch.equal(total, as_points[1])
    want = HS.histogram(particles.cpu().numpy(), edges)
    assert U.same_bits(table, want[0]) and U.same_bits(total, want[1]) and int(total.sum()) > 0
    g = pairs.radial_distribution(total, edges, n, 1.0)
    assert g.shape == (24,) and bool(torch.isfinite(g).all())
    # a tick since the count: the grid is stale
    eng = crate.engine
    dev = particles.device
    out, counts = U.full(24, dev), U.full(2, dev)
    offsets = U.full(eng.capacity + 1, dev)
    torch.cuda.synchronize()
    eng.pairs_count(None, radius=float(edges[-1]), offsets=offsets, counts=counts)
    eng.pairs_hist(None, out, edges=edges, counts=counts)
    eng.synchronize()
    assert U.same_bits(out, want[1])
    crate.physics_tick()
    assert U.code_of(eng.pairs_hist, None, out, edges=edges, counts=counts) == N.ERR_STATE
    assert U.code_of(eng.pairs_hist, None, out, edges=edges, queries=particles[:16].contiguous(), counts=counts) == N.ERR_STATE
    slab = sc.Engine(capacity=256)
    slab.set_slab(0, 50, 3, False, True)
    assert U.code_of(slab.pairs_count, None, radius=0.1, offsets=offsets[:257], counts=counts) == N.ERR_STATE
    assert U.code_of(slab.pairs_hist, None, out, edges=edges, counts=counts) == N.ERR_STATE
    slab.close()


def test_the_capacity_does_not_reach_the_result(sc):
    import torch
    case = HK.cases()["far_cells"]
    points = U.tensor(case.points)
    results = []
    for capacity in (16, 100_000):
        crate = sc.Crate(U.scene(sc), noise="none", capacity=capacity)
        results.append(crate.distance_histogram(case.edges, points=points, per_row=True))
    assert all(torch.equal(a, b) for a, b in zip(*results))
    assert U.same_bits(results[0][0], spec("far_cells", False)[0])


# ---- 4. the status

def test_a_query_outside_writes_the_status_only(crate):
    import torch
    case = HK.outside()
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    tb, tt, counts = through_the_engine(eng, case.points, case.edges, case.queries)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(tb, tt)
    # the count's own verdict is unchanged: a fill afterwards succeeds, and so does the next histogram
    want = S.pairs(case.points, case.edges[-1])
    partners, again = U.full(len(want[1]), dev), U.full(2, dev)
    eng.pairs_fill(partners)
    tb = U.full((len(case.points), 3), dev, dtype=torch.int32)
    eng.pairs_hist(tb, tt, edges=case.edges, counts=again)
    eng.synchronize()
    rule = HS.histogram(case.points, case.edges)
    assert U.same_bits(partners, want[1]) and again.cpu().tolist() == [len(case.points), 0]
    assert U.same_bits(tb, rule[0]) and U.same_bits(tt, rule[1])
    points, q = U.tensor(case.points), U.tensor(case.queries)
    with pytest.raises(ValueError, match="domain"):
        crate.distance_histogram(case.edges, points=points, queries=q)
    out = crate.distance_histogram(case.edges, points=points, queries=q, per_row=True, sync=False)
    crate.synchronize()
    assert int(out[-1][1]) == -1
    # a point outside: the count's flag
    far = case.points.copy()
    far[7, 1] = -(2.0 ** 32) * case.edges[-1]
    tb, tt, counts = through_the_engine(eng, far, case.edges)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(tb, tt)


# ---- 5. the workspace is left as it is; the half flag; a shorter last edge

@pytest.mark.parametrize("half", [False, True])
def test_fill_hist_fill(crate, half):
    import torch
    case = HK.cases()["bins_33"]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(case.points)
    want = S.pairs(case.points, case.edges[-1], half)
    k = len(want[1])
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    before, after = (U.full(k, dev), torch.full((k,), -1.5, dtype=torch.float64, device=dev)), \
                    (U.full(k, dev), torch.full((k,), -1.5, dtype=torch.float64, device=dev))
    tb, tt = U.full((n, 33), dev, dtype=torch.int32), U.full(33, dev)
    probes = U.tensor(case.points[:40] + 0.01)
    probe_table = U.full((40, 33), dev, dtype=torch.int32)
    t = U.tensor(case.points)
    eng.pairs_count(t, radius=float(case.edges[-1]), offsets=offsets, counts=counts, half=half)
    eng.pairs_fill(*before)
    eng.pairs_hist(tb, tt, edges=case.edges, counts=out)
    eng.pairs_hist(probe_table, None, edges=case.edges, queries=probes, counts=out)
    eng.pairs_hist(None, tt, edges=case.edges, counts=out)                          # ... and again, the totals alone
    eng.pairs_fill(*after)
    eng.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert U.same_bits(after[0], want[1]) and U.same_bits(after[1], want[2])
    rule = spec("bins_33", False)
    assert U.same_bits(tb, rule[0]) and U.same_bits(tt, rule[1])                                  # the half flag is ignored
    assert U.same_bits(probe_table, HS.histogram(case.points, case.edges, case.points[:40] + 0.01)[0])


def test_pair_tensors_are_the_same_before_and_after(crate):
    import torch
    case = HK.cases()["bins_17"]
    points, radius = U.tensor(case.points), float(case.edges[-1])
    before = crate.pair_tensors(radius, points=points, squared_distances=True)
    crate.distance_histogram(case.edges, points=points, per_row=True)
    after = crate.pair_tensors(radius, points=points, squared_distances=True)
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_a_last_edge_below_the_counts_radius(crate):
    pts, _ = HK.cloud(21, 400)
    edges = np.linspace(0.0, 0.06, 8)
    wide = through_the_engine(crate.engine, pts, edges, radius=0.1)
    own = through_the_engine(crate.engine, pts, edges)
    want = HS.histogram(pts, edges)
    assert want[1].sum() > 0
    for tb, tt, counts in (wide, own):
        assert counts.cpu().tolist() == [400, 0] and U.same_bits(tb[:400], want[0]) and U.same_bits(tt, want[1])
    probes = pts[:70] * 0.5 + 0.2
    wide = through_the_engine(crate.engine, pts, edges, probes, radius=0.1)
    assert U.same_bits(wide[0][:70], HS.histogram(pts, edges, probes)[0])


# ---- 6. errors

def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n, bins = 300, 5
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points = np.random.RandomState(3).rand(n, 2)
    t = U.tensor(points)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    table, total, out = U.full((n, bins), dev, dtype=torch.int32), U.full(bins, dev), U.full(2, dev)
    edges = np.linspace(0.0, 0.05, bins + 1)
    torch.cuda.synchronize()
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_hist_device
    good = edges * edges
    args = lambda **kw: tuple({**dict(ctx=ctx, q=None, nq=0, e2=N.dptr(good), bins=bins, table=ptr(table),  # noqa: E731
                                      total=ptr(total), room=n, counts=ptr(out)), **kw}.values())
    assert fn(*args()) == N.ERR_STATE                                               # no count yet
    eng.pairs_count(t, radius=0.05, offsets=offsets, counts=counts)
    assert fn(*args(ctx=None)) == N.ERR_ARG
    assert fn(*args(counts=None)) == N.ERR_ARG
    assert fn(*args(table=None, total=None)) == N.ERR_ARG                           # both outputs null
    for bad in (0, -1, N.HIST_MAX_BINS + 1):
        assert fn(*args(bins=bad)) == N.ERR_ARG
    assert fn(*args(e2=None)) == N.ERR_ARG                                          # null edges
    for bad in ([0.0, 1e-4, 1e-4, 2e-4, 3e-4, 4e-4], [0.0, 2e-4, 1e-4, 3e-4, 4e-4, 5e-4], [1e-4, 0.0, 2e-4, 3e-4, 4e-4, 5e-4],
                [0.0, 1e-4, 2e-4, 3e-4, 4e-4, float("nan")], [-1e-9, 1e-4, 2e-4, 3e-4, 4e-4, 5e-4],
                [float("nan"), 1e-4, 2e-4, 3e-4, 4e-4, 5e-4], [float("-inf"), 1e-4, 2e-4, 3e-4, 4e-4, 5e-4],
                [float("inf")] * 6):
        held = np.array(bad, dtype=np.float64)                                      # (alive over the call)
        assert fn(*args(e2=N.dptr(held))) == N.ERR_ARG, bad
    beyond = good.copy()
    beyond[-1] = np.nextafter(0.05 * 0.05, 1.0)                                     # one ulp above the count's r2
    assert fn(*args(e2=N.dptr(beyond))) == N.ERR_ARG
    assert fn(*args(room=-1)) == N.ERR_ARG
    assert fn(*args(q=ptr(t), nq=-1)) == N.ERR_ARG
    assert fn(*args(q=N._P(t.data_ptr() + 8), nq=n - 1)) == N.ERR_ARG               # misaligned queries
    assert fn(*args(room=n - 1)) == N.ERR_CAPACITY                                  # a short table, self form
    assert fn(*args(q=ptr(t), nq=n, room=n - 1)) == N.ERR_CAPACITY                  # ... and for the queries
    assert fn(*args(q=ptr(t), nq=(1 << 28) + 1, room=(1 << 28) + 1)) == N.ERR_CAPACITY
    assert U.code_of(eng.pairs_hist, table[:n - 1], total, edges=edges, counts=out) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    for call in (lambda: eng.pairs_hist(None, None, edges=edges, counts=out), lambda: eng.pairs_hist(table, total[:4], edges=edges, counts=out),
                 lambda: eng.pairs_hist(table[:, :4], total, edges=edges, counts=out), lambda: eng.pairs_hist(table.long(), total, edges=edges, counts=out),
                 lambda: eng.pairs_hist(table, total, edges=edges[::-1], counts=out), lambda: eng.pairs_hist(table, total, edges=edges, room=n + 1, counts=out),
                 lambda: eng.pairs_hist(table, total, edges=np.linspace(0, 0.05, 66), counts=out)):
        with pytest.raises(ValueError):
            call()
    eng.synchronize()
    assert U.untouched(table, total, out)
    assert fn(*args(total=None)) == 0                                               # the table alone: fine
    assert fn(*args(table=None, room=0)) == 0                                       # the totals alone need no room
    eng.synchronize()
    want = HS.histogram(points, edges)
    assert U.same_bits(table, want[0]) and U.same_bits(total, want[1]) and out.cpu().tolist() == [n, 0]
    eng.close()


def test_wrapper_errors(crate):
    points = U.tensor(HK.cases()["rows_65"].points)
    for call in (lambda: crate.distance_histogram([0.0, 0.1], points=points, totals=False),
                 lambda: crate.distance_histogram([0.1, 0.0], points=points), lambda: crate.distance_histogram([0.0], points=points),
                 lambda: crate.distance_histogram(np.linspace(0, 1, 66), points=points),
                 lambda: crate.distance_histogram([0.0, 0.1], points=points.float())):
        with pytest.raises(ValueError):
            call()
