"""GPU tests of the device weighted sums (sc_pairs_sum_device, `Engine.pairs_sum`, `Crate.field_tensors`): sums and weight
sums equal tests/field_spec.py bit for bit -- every row and every channel of every case of tests/field_cases.py, NaN where
the rule has NaN --, through the crate and through the engine, with and without the weight sums; two calls give the same
bits; the domain error and short values write the status and nothing else; the workspace of the count is left as it is;
rows past the row count stay untouched; the state form after ticks, the invalidation rule, the error codes and the path
that does not synchronise."""
import functools

import numpy as np
import pytest

import cluster_spec as CS
import field_cases as FK
import field_spec as FS
import gpu_support as U
import nearest_spec as NS
import pairs_cases as K
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [name for name in FK.cases() if name not in FK.OUTSIDE]


def two_dimensional(case):
    return None if case.values is None else case.values.reshape(len(case.points), -1 if case.values.ndim == 1 else case.values.shape[1])


@functools.lru_cache(maxsize=None)
def spec(name):
    case = FK.cases()[name]
    with np.errstate(all="ignore"):
        return FS.field(case.points, case.radius, two_dimensional(case), case.power, case.include_self, case.queries)


def through_the_crate(crate, case, **kw):
    return crate.field_tensors(U.tensor(case.values, None), case.radius, power=case.power, include_self=case.include_self,
                               points=U.tensor(case.points, 2), queries=U.tensor(case.queries, 2), **kw)


def through_the_engine(eng, case, *, weight_sums=True, half=False, spare=8, values_rows=None):
    """count + sum through the engine into sentinel-filled tensors with `spare` rows of room beyond the rows ->
    (sums or None, wsum or None, counts), synchronised."""
    import torch
    dev = torch.device("cuda", eng.device)
    n = len(case.points)
    rows = n if case.queries is None else len(case.queries)
    values = U.tensor(two_dimensional(case), None)
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    sums = None if values is None else U.full((rows + spare, values.shape[1]), dev, U.SENTINEL_F)
    wsum = U.full(rows + spare, dev, U.SENTINEL_F) if weight_sums or values is None else None
    t, q = U.tensor(case.points, 2), U.tensor(case.queries, 2)                          # (alive until the synchronisation)
    eng.pairs_count(t, radius=case.radius, offsets=offsets, counts=counts, half=half)
    assert eng.pairs_sum(values, sums, wsum, power=case.power, include_self=case.include_self, queries=q, counts=out,
                         values_rows=values_rows) is out
    eng.synchronize()
    return sums, wsum, out


# ---- 1. every case, both ways in

@pytest.mark.parametrize("name", CASES)
def test_case_equals_the_spec(crate, name):
    case = FK.cases()[name]
    want_sums, want_wsum = spec(name)
    rows = len(want_wsum)
    got = through_the_crate(crate, case, weight_sums=True)
    assert all(t.is_cuda for t in got)
    if case.values is None:
        assert len(got) == 1 and U.same_bits_or_nan(got[0], want_wsum)
        assert U.same_bits_or_nan(through_the_crate(crate, case)[0], want_wsum)
    else:
        shaped = want_sums[:, 0] if case.values.ndim == 1 else want_sums
        assert len(got) == 2 and U.same_bits_or_nan(got[0], shaped) and U.same_bits_or_nan(got[1], want_wsum)
        only = through_the_crate(crate, case)
        assert len(only) == 1 and U.same_bits_or_nan(only[0], shaped)
    if want_sums.shape[1] > 8:
        return
    for weight_sums in (True, False):
        sums, wsum, counts = through_the_engine(crate.engine, case, weight_sums=weight_sums, half=not weight_sums)
        assert counts.cpu().tolist() == [rows, 0]
        if sums is not None:
            assert U.same_bits_or_nan(sums[:rows], want_sums) and U.untouched(sums[rows:])
        if wsum is not None:
            assert U.same_bits_or_nan(wsum[:rows], want_wsum) and U.untouched(wsum[rows:])


def test_two_calls_give_identical_bits(crate):
    case = FK.cases()[FK.ORDER]
    a = through_the_crate(crate, case, weight_sums=True)
    other = FK.cases()["channels_8"]
    through_the_crate(crate, other)                                                 # another grid and other values in between
    b = through_the_crate(crate, case, weight_sums=True)
    assert all(x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes() for x, y in zip(a, b))


# ---- 2. the status: the domain and the values' rows

@pytest.mark.parametrize("name", FK.OUTSIDE)
def test_outside_the_domain_writes_the_status_only(crate, name):
    case = FK.cases()[name]
    with pytest.raises(ValueError, match="domain"):
        through_the_crate(crate, case)
    sums, wsum, counts = through_the_engine(crate.engine, case)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(sums, wsum)
    out = through_the_crate(crate, case, sync=False)
    crate.synchronize()
    assert int(out[-1][1]) == -1


def test_a_query_outside_leaves_the_counts_flag_as_it_was(crate):
    import torch
    case = FK.cases()[FK.OUTSIDE[1]]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(case.points)
    want = S.pairs(case.points, case.radius)
    t, q, values = U.tensor(case.points, 2), U.tensor(case.queries, 2), U.tensor(two_dimensional(case), None)
    offsets, counts, out, again = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev), U.full(2, dev)
    sums = U.full((len(case.queries), values.shape[1]), dev, U.SENTINEL_F)
    own = U.full((n, values.shape[1]), dev, U.SENTINEL_F)
    partners, d2 = U.full(len(want[1]), dev), U.full(len(want[1]), dev, U.SENTINEL_F)
    eng.pairs_count(t, radius=case.radius, offsets=offsets, counts=counts)
    eng.pairs_sum(values, sums, power=case.power, queries=q, counts=out)
    eng.pairs_fill(partners, d2)                                                    # the count's flag is still down
    eng.pairs_sum(values, own, power=case.power, counts=again)                      # ... and so is the next sum's own
    eng.synchronize()
    assert out.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(sums)
    assert U.same_bits_or_nan(partners, want[1]) and U.same_bits_or_nan(d2, want[2])
    with np.errstate(all="ignore"):
        rule = FS.field(case.points, case.radius, two_dimensional(case), case.power, True)
    assert again.cpu().tolist() == [n, 0] and U.same_bits_or_nan(own, rule[0])


def test_values_one_row_short_and_one_row_long(crate):
    import torch
    case = FK.cases()["channels_3"]
    n = len(case.points)
    want_sums, want_wsum = spec("channels_3")
    sums, wsum, counts = through_the_engine(crate.engine, case, values_rows=n - 1)
    assert counts.cpu().tolist() == [U.SENTINEL, -2] and U.untouched(sums, wsum)
    points = U.tensor(case.points, 2)
    short = U.tensor(case.values[:n - 1], None)
    with pytest.raises(ValueError, match="rows"):
        crate.field_tensors(short, case.radius, points=points)
    out = crate.field_tensors(short, case.radius, points=points, sync=False)
    crate.synchronize()
    assert int(out[-1][1]) == -2
    long = torch.cat([U.tensor(case.values, None), U.full((1, 3), points.device, float("nan"))])
    torch.cuda.synchronize()
    got = crate.field_tensors(long, case.radius, points=points, weight_sums=True)
    assert U.same_bits_or_nan(got[0], want_sums) and U.same_bits_or_nan(got[1], want_wsum)
    # the status wins over the queries' rows, and the domain over the values
    outside = FK.cases()[FK.OUTSIDE[1]]
    sums, wsum, counts = through_the_engine(crate.engine, outside, values_rows=len(outside.points) - 1)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(sums, wsum)


# ---- 3. the workspace is left as it is

@pytest.mark.parametrize("half", [False, True])
def test_lists_labels_and_tables_are_the_same_before_and_after(crate, half):
    import torch
    case = FK.cases()["long_rows_p0"]
    points, radius = case.points, case.radius
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n, k = len(points), 5
    want = S.pairs(points, radius, half)
    total = len(want[1])
    offsets, counts, other, third = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev), U.full(2, dev)
    before = [U.full(total, dev), U.full(total, dev, U.SENTINEL_F), U.full(n, dev), U.full((n, k), dev)]
    after = [U.full(total, dev), U.full(total, dev, U.SENTINEL_F), U.full(n, dev), U.full((n, k), dev)]
    values = U.tensor(two_dimensional(case), None)
    sums, wsum = U.full((n, values.shape[1]), dev, U.SENTINEL_F), U.full(n, dev, U.SENTINEL_F)
    probes = U.tensor(points[:40] + 0.25 * radius, 2)
    probe_sums = U.full((40, values.shape[1]), dev, U.SENTINEL_F)
    t = U.tensor(points, 2)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
    for partners, d2, labels, table in (before, after):
        eng.pairs_fill(partners, d2)
        eng.pairs_label(labels, counts=third)
        eng.pairs_nearest(table, k=k, counts=third)
        if partners is before[0]:
            eng.pairs_sum(values, sums, wsum, power=2, include_self=False, counts=other)
            eng.pairs_sum(values, probe_sums, power=1, queries=probes, counts=third)
            eng.pairs_sum(None, None, wsum, power=0, counts=third)                  # ... and repeated, without values
    eng.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, after))
    assert U.same_bits_or_nan(after[0], want[1]) and U.same_bits_or_nan(after[1], want[2]) and \
        U.same_bits_or_nan(after[2], CS.clusters(points, radius)[0])
    assert U.same_bits_or_nan(after[3], NS.nearest(points, radius, k)[0])
    with np.errstate(all="ignore"):
        assert other.cpu().tolist() == [n, 0] and \
            U.same_bits_or_nan(sums, FS.field(points, radius, two_dimensional(case), 2, False)[0])
        assert U.same_bits_or_nan(probe_sums,
                                  FS.field(points, radius, two_dimensional(case), 1, True, points[:40] + 0.25 * radius)[0])
        assert U.same_bits_or_nan(wsum, FS.field(points, radius, None, 0, True)[1])


def test_the_crates_other_tensors_are_the_same_before_and_after(crate):
    import torch
    case = FK.cases()["channels_9"]
    points = U.tensor(case.points, 2)
    before = (crate.pair_tensors(case.radius, points=points, squared_distances=True),
              crate.neighbor_tensors(7, case.radius, points=points), crate.cluster_tensors(case.radius, points=points))
    through_the_crate(crate, case, weight_sums=True)
    after = (crate.pair_tensors(case.radius, points=points, squared_distances=True),
             crate.neighbor_tensors(7, case.radius, points=points), crate.cluster_tensors(case.radius, points=points))
    assert all(torch.equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))


# ---- 4. the state form

def test_state_after_ticks_with_queries_and_the_stale_count(sc):
    import torch
    from sand_crate_amd import _native as N
    from sand_crate_amd import pairs
    crate = sc.Crate(U.scene(sc))
    for _ in range(40):
        crate.physics_tick()
    particles, velocities = crate.state_tensors(pressure=False)
    n = len(particles)
    assert n > 100
    points, v = particles.cpu().numpy(), velocities.cpu().numpy()
    for power, factor, include_self in ((3, 1.0, True), (1, 2.0, False)):
        radius = factor * crate.diameter
        got = crate.field_tensors(velocities, None if factor == 1.0 else radius, power=power, include_self=include_self,
                                  weight_sums=True)
        want = FS.field(points, radius, v, power, include_self)
        assert U.same_bits_or_nan(got[0], want[0]) and U.same_bits_or_nan(got[1], want[1])
    assert crate.particle_count == n
    density, = crate.field_tensors()
    assert U.same_bits_or_nan(density, FS.field(points, crate.diameter)[1])
    offsets, _ = crate.pair_tensors()
    count, = crate.field_tensors(power=0, include_self=False)
    assert torch.equal(count, pairs.row_lengths(offsets).double())                  # power 0 counts the partners
    lo, hi = points.min(axis=0), points.max(axis=0)
    grid = pairs.grid_queries(lo[0], hi[0], lo[1], hi[1], 16, 12, particles.device)
    torch.cuda.synchronize()
    sums, wsum = crate.field_tensors(velocities, 2 * crate.diameter, queries=grid, weight_sums=True)
    want = FS.field(points, 2 * crate.diameter, v, 3, True, grid.cpu().numpy())
    assert U.same_bits_or_nan(sums, want[0]) and U.same_bits_or_nan(wsum, want[1]) and crate.particle_count == n
    image = pairs.normalized(sums, wsum).reshape(12, 16, 2)
    assert bool(torch.isfinite(image).all()) and bool((wsum > 0).any())
    # a tick since the count: the grid is stale
    eng = crate.engine
    out, counts = torch.zeros((eng.capacity, 2), dtype=torch.float64, device=particles.device), U.full(2, particles.device)
    torch.cuda.synchronize()
    values = torch.zeros((eng.capacity, 2), dtype=torch.float64, device=particles.device)
    torch.cuda.synchronize()
    eng.pairs_sum(values, out, counts=counts)
    crate.physics_tick()
    assert U.code_of(eng.pairs_sum, values, out, counts=counts) == N.ERR_STATE
    assert U.code_of(eng.pairs_sum, values, out[:16], queries=grid[:16], counts=counts) == N.ERR_STATE


def test_state_of_an_empty_crate_and_rows_past_the_row_count(sc):
    import torch
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    wsum, = crate.field_tensors()                                                   # before the first tick
    assert wsum.shape == (0,)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    empty = torch.zeros((0, 3), dtype=torch.float64, device=dev)
    sums, wsum = crate.field_tensors(empty, weight_sums=True)
    assert sums.shape == (0, 3) and wsum.shape == (0,)
    queries = np.array([[0.5, 0.5], [np.nan, 1.0]])
    sums, wsum = crate.field_tensors(empty, queries=U.tensor(queries, 2), weight_sums=True)
    assert sums.cpu().tolist() == [[0.0] * 3] * 2 and wsum.cpu().tolist() == [0.0, 0.0]
    case = FK.cases()["rows_65"]
    crate.particles = case.points
    room, n = eng.capacity, len(case.points)
    offsets, counts = U.full(room + 1, dev), U.full(2, dev)
    values = torch.cat([U.tensor(case.values, None), U.full((room - n, 2), dev, float("nan"))])
    sums, wsum = U.full((room, 2), dev, U.SENTINEL_F), U.full(room, dev, U.SENTINEL_F)
    torch.cuda.synchronize()
    eng.pairs_count(None, radius=case.radius, offsets=offsets, counts=counts)
    eng.pairs_sum(values, sums, wsum, counts=counts)
    eng.synchronize()
    want = spec("rows_65")
    assert counts.cpu().tolist() == [n, 0]
    assert U.same_bits_or_nan(sums[:n], want[0]) and U.same_bits_or_nan(wsum[:n], want[1]) and U.untouched(sums[n:], wsum[n:])
    # values with fewer rows than the STATE has particles: only the device knows
    eng.pairs_sum(values[:n - 1], sums, wsum, counts=counts, room=room)
    eng.synchronize()
    assert counts.cpu().tolist() == [n, -2] and U.same_bits_or_nan(sums[:n], want[0]) and U.untouched(sums[n:], wsum[n:])
    with pytest.raises(ValueError, match="rows"):
        crate.field_tensors(values[:n - 1])


def test_summing_changes_nothing(sc):
    def trajectory(summing):
        crate = sc.Crate(U.scene(sc))
        probes = U.tensor(np.random.RandomState(9).rand(50, 2), 2) if summing else None
        for _ in range(30):
            crate.physics_tick()
            if summing:
                crate.field_tensors(crate.state_tensors()[1])
                crate.field_tensors(None, 2 * crate.diameter, queries=probes, sync=False)
        state = crate.engine.download()
        crate.sync_host_rng()
        rng = np.random.get_state()
        return state, (rng[1].copy(), rng[2])

    (a, rng_a), (b, rng_b) = trajectory(False), trajectory(True)
    assert len(a[0]) > 100
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(rng_a[0], rng_b[0]) and rng_a[1] == rng_b[1]


# ---- 5. errors

def test_state_errors_and_the_slab(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    t = U.tensor(points, 2)
    offsets = torch.zeros(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    values = torch.zeros((eng.capacity, 2), dtype=torch.float64, device=dev)
    sums, out = U.full((eng.capacity, 2), dev, U.SENTINEL_F), U.full(2, dev)
    torch.cuda.synchronize()
    assert U.code_of(eng.pairs_sum, values, sums, counts=out) == N.ERR_STATE          # no count yet
    assert U.code_of(eng.pairs_sum, values, sums, queries=t, counts=out) == N.ERR_STATE
    eng.synchronize()
    assert U.untouched(sums, out)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_sum(values, sums, counts=out)                                         # ... with one: fine, and again
    eng.pairs_sum(values, sums, queries=t, counts=out)
    crate.particles = points                                                        # an upload since the count
    assert U.code_of(eng.pairs_sum, values, sums, counts=out) == N.ERR_STATE
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_sum(values, sums, counts=out)
    eng.append(points[:3] + 2.0, np.zeros((3, 2)))                                  # an append since the count
    assert U.code_of(eng.pairs_sum, values, sums, counts=out) == N.ERR_STATE
    eng.synchronize()
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    crate._send_tick_inputs()                                                       # inside a tick
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_sum, values, sums, counts=out) == N.ERR_STATE
    finally:
        eng.step_finish()
    # a slab context has no state form -- the count refuses it, as before --, but sums over a caller's points
    slab = sc.Engine(capacity=256)
    slab.set_slab(0, 50, 3, False, True)
    assert U.code_of(slab.pairs_count, None, radius=radius, offsets=offsets[:257], counts=counts) == N.ERR_STATE
    assert U.code_of(slab.pairs_sum, values, sums, counts=out) == N.ERR_STATE
    own = U.tensor(FK.make_values(3, 65, 2), None)
    slab.pairs_count(t, radius=radius, offsets=offsets[:66], counts=counts)
    slab.pairs_sum(own, sums[:65], counts=out)
    slab.synchronize()
    assert U.same_bits_or_nan(sums[:65], FS.field(points, radius, own.cpu().numpy())[0])
    slab.close()


def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n, width = 300, 3
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points = np.random.RandomState(3).rand(n, 2)
    t = U.tensor(points, 2)
    values = U.tensor(FK.make_values(4, n, width), None)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    sums, wsum, out = U.full((n, width), dev, U.SENTINEL_F), U.full(n, dev, U.SENTINEL_F), U.full(2, dev)
    torch.cuda.synchronize()
    eng.pairs_count(t, radius=0.05, offsets=offsets, counts=counts)
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_sum_device
    args = lambda **kw: tuple({**dict(ctx=ctx, q=None, nq=0, v=ptr(values), vrows=n, c=width, power=3, flags=0,  # noqa: E731
                                      sums=ptr(sums), wsum=ptr(wsum), room=n, counts=ptr(out)), **kw}.values())
    assert fn(*args(ctx=None)) == N.ERR_ARG
    assert fn(*args(counts=None)) == N.ERR_ARG
    assert fn(*args(sums=None, wsum=None, c=0, v=None)) == N.ERR_ARG                # both outputs null
    for bad in (-1, N.FIELDS_MAX_CHANNELS + 1):
        assert fn(*args(c=bad)) == N.ERR_ARG
    assert fn(*args(v=None)) == N.ERR_ARG                                           # channels without values
    assert fn(*args(sums=None)) == N.ERR_ARG                                        # ... or without sums
    for bad in (-1, 4):
        assert fn(*args(power=bad)) == N.ERR_ARG
    for bad in (2, 3, -1):
        assert fn(*args(flags=bad)) == N.ERR_ARG
    assert fn(*args(room=-1)) == N.ERR_ARG
    assert fn(*args(vrows=-1)) == N.ERR_ARG
    assert fn(*args(q=ptr(t), nq=-1)) == N.ERR_ARG
    assert fn(*args(q=N._P(t.data_ptr() + 8), nq=n - 1)) == N.ERR_ARG               # misaligned queries
    assert fn(*args(room=n - 1)) == N.ERR_CAPACITY                                  # short sums, self form
    assert fn(*args(q=ptr(t), nq=n, room=n - 1)) == N.ERR_CAPACITY                  # ... and for the queries
    assert fn(*args(q=ptr(t), nq=(1 << 28) + 1, room=(1 << 28) + 1)) == N.ERR_CAPACITY
    assert U.code_of(eng.pairs_sum, values, sums[:n - 1], counts=out) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    for call in (lambda: eng.pairs_sum(values, sums, power=4, counts=out), lambda: eng.pairs_sum(values, None, wsum, counts=out),
                 lambda: eng.pairs_sum(None, None, None, counts=out), lambda: eng.pairs_sum(values, sums[:, :2], counts=out),
                 lambda: eng.pairs_sum(values, sums, room=n + 1, counts=out), lambda: eng.pairs_sum(values, sums, values_rows=n + 1, counts=out)):
        with pytest.raises(ValueError):
            call()
    eng.synchronize()
    assert U.untouched(sums, wsum, out)
    assert fn(*args(wsum=None)) == 0                                                # without the weight sums: fine
    assert fn(*args(q=ptr(t), nq=10, room=10, sums=None, v=None, c=0, flags=N.FIELDS_SELF)) == 0   # wsum alone, few queries
    eng.synchronize()
    want = FS.field(points, 0.05, values.cpu().numpy(), 3, False)
    assert U.same_bits_or_nan(sums, want[0])
    assert U.same_bits_or_nan(wsum[:10], FS.field(points, 0.05, None, 3, True, points[:10])[1]) and U.untouched(wsum[10:])
    eng.close()


# ---- 6. the path that does not synchronise

@pytest.mark.parametrize("name", ["queries_257", "channels_17", "one_dimensional", "density"])
def test_sync_false_does_not_synchronise_and_equals_the_default(crate, monkeypatch, name):
    import torch
    case = FK.cases()[name]
    values, points, queries = U.tensor(case.values, None), U.tensor(case.points, 2), U.tensor(case.queries, 2)
    kw = dict(power=case.power, include_self=case.include_self, points=points, queries=queries, weight_sums=True)
    want = crate.field_tensors(values, case.radius, **kw)
    rows = len(want[-1])

    def forbidden(*args, **kw):
        raise AssertionError("the call synchronised")

    crate.engine.set_stream(torch.cuda.current_stream().cuda_stream)                 # the wrapper's own torch work is ordered
    try:
        with monkeypatch.context() as m:
            m.setattr(type(crate.engine), "synchronize", forbidden)
            m.setattr(torch.cuda, "synchronize", forbidden)
            m.setattr(torch.cuda.Stream, "synchronize", forbidden)
            m.setattr(torch.Tensor, "item", forbidden)
            m.setattr(torch.Tensor, "cpu", forbidden)
            out = crate.field_tensors(values, case.radius, sync=False, **kw)
        crate.synchronize()
        torch.cuda.synchronize()
    finally:
        crate.engine.use_own_stream()
    assert len(out) == len(want) + 1 and out[-1].cpu().tolist() == [rows, 0]
    assert all(a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(out[:-1], want))
    with pytest.raises(ValueError, match="power"):
        crate.field_tensors(values, case.radius, power=4)
