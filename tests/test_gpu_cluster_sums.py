"""GPU tests of the per-cluster sums (sc_pairs_cluster_sums_device, `Engine.pairs_cluster_sums`, `Crate.cluster_sums`,
`Crate.cluster_observables`): sums, minima and maxima equal tests/cluster_sums_spec.py byte for byte (a NaN equal to any
NaN: the spec says why) -- on the cases of tests/cluster_sums_cases.py, on 70,001 points with the device's own labels, on
the state after ticks, in a twin of eight times the capacity and after a load with permuted ids --, the same bytes when
repeated, after a half and a full count and after another reader, a fill after the reduction, a room below the cluster
count, the statuses, the error codes and the path that does not synchronise."""
import functools

import numpy as np
import pytest

import cluster_cases as CK
import cluster_sums_cases as SK
import cluster_sums_spec as SS
import gpu_support as U
import pairs_cases as K
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

MARK = -1.25                        # what the float tensors hold before a call


def marked(shape, device):
    return U.full(shape, device, MARK)


def host(t):
    return t if isinstance(t, np.ndarray) else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def spec(name, width):
    """The reference of a case over its first `width` channels, computed once and shared."""
    _, values, labels, sizes, _ = SK.cases()[name]
    out = SS.cluster_sums(labels, values[:, :width], clusters=len(sizes))
    for a in out:
        a.setflags(write=False)
    return out


def assert_tables(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert SS.same(host(g), w)


def assert_label(got, case):
    for g, w in zip(got, case[2:]):
        assert host(g).dtype == np.int64 and host(g).tobytes() == w.tobytes()


def reduce(eng, points, radius, values, *, half=True, extrema=True, room=None, repeat=1, between=None):
    """count + label + sums through the engine into marked tensors -> (sums, mins, maxs, counts), synchronised."""
    import torch
    dev = torch.device("cuda", eng.device)
    n, width = len(points), values.shape[1]
    room = n if room is None else room
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    labels = U.full(n, dev)
    tables = [marked((room + 4, width), dev) for _ in range(3 if extrema else 1)]
    t, v = U.tensor(points), U.tensor(values, width)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
    eng.pairs_label(labels, counts=counts)
    for k in range(repeat):
        if between is not None and k:
            between()
        out = U.full(2, dev)
        assert eng.pairs_cluster_sums(v, *tables, counts=out, room_clusters=room) is out
    eng.synchronize()
    return (*tables, out)


# ---- 1. the cases on the points= path

@pytest.mark.parametrize("width,extrema", [(1, False), (1, True), (8, False), (8, True)])
def test_ladder_equals_the_spec(crate, width, extrema):
    case = SK.cases()["ladder"]
    pts, values = case[0], case[1][:, 3:4] if width == 1 else case[1]               # (one channel: the one that shows the order)
    got = crate.cluster_sums(U.tensor(values, width), SK.RADIUS, points=U.tensor(pts), extrema=extrema)
    assert len(got) == (6 if extrema else 4) and all(t.is_cuda for t in got)
    assert_label(got[:3], case)
    want = SS.cluster_sums(case[2], values, clusters=len(case[3])) if width == 1 else spec("ladder", 8)
    assert_tables(got[3:], want[:3 if extrema else 1])
    flat = crate.cluster_sums(U.tensor(values, width)[:, 0].contiguous(), SK.RADIUS, points=U.tensor(pts))   # (n,): one channel
    assert flat[3].shape == (len(case[3]), 1) and SS.same(host(flat[3]), want[0][:, :1])


def test_chain4_reaches_the_fourth_level(crate):
    case = SK.cases()["chain4"]
    got = crate.cluster_sums(U.tensor(case[1]), SK.RADIUS, points=U.tensor(case[0]), extrema=True)
    assert_label(got[:3], case)
    assert_tables(got[3:], spec("chain4", 2))


def test_isolated_with_dead_rows_never_reads_them(crate):
    case = SK.cases()["isolated_dead"]
    got = crate.cluster_sums(U.tensor(case[1], 3), SK.RADIUS, points=U.tensor(case[0]), extrema=True)
    assert_label(got[:3], case)
    assert_tables(got[3:], spec("isolated_dead", 3))
    assert not np.isnan(host(got[3])).any() and np.isnan(case[1][case[2] < 0]).all()


def test_special_values(crate):
    case = SK.cases()["special"]
    got = crate.cluster_sums(U.tensor(case[1]), SK.RADIUS, points=U.tensor(case[0]), extrema=True)
    sums, mins, maxs = (host(t) for t in got[3:])
    assert_tables((sums, mins, maxs), spec("special", 2))
    assert sums[0, 0] == 0.0 and not np.signbit(sums[0, 0]) and np.signbit(mins[0, 0])    # -0.0 only: +0.0 by the rule
    assert np.isnan([sums[1, 0], mins[1, 0], maxs[1, 0]]).all()
    assert np.isnan(sums[2, 0]) and mins[2, 0] == -np.inf and maxs[2, 0] == np.inf
    assert sums[3, 0] == mins[3, 0] == maxs[3, 0] == -7.25


def test_wide_with_the_devices_own_labels(crate):
    points, radius = CK.cases()["wide"]
    values = SK.table(96, len(points), 3)
    got = crate.cluster_sums(U.tensor(values, 3), radius, points=U.tensor(points), extrema=True)
    labels, sizes = host(got[0]), host(got[1])
    assert 100 < len(sizes) < len(points) // 4 and sizes.max() > 1000                # big and small ones: two levels at least
    assert np.array_equal(np.bincount(labels[labels >= 0]), sizes)
    assert_tables(got[3:], SS.cluster_sums(labels, values, clusters=len(sizes)))


# ---- 2. the state

def state_of(crate):
    xy, vv, p, ids = crate.state_tensors(ids=True)
    return xy, vv, p, ids


def test_observables_after_ticks_in_a_twin_and_after_a_load_with_permuted_ids(sc):
    import torch
    from sand_crate_amd import pairs
    first = sc.Crate(U.scene(sc), noise="host", noise_seed=3)
    for _ in range(200):
        first.physics_tick()
    xy, vv, p, _ = state_of(first)
    n = len(xy)
    assert n > 1000
    labels, roots, table = first.cluster_observables()
    want_labels, want_sizes, want_roots = first.cluster_tensors()
    assert torch.equal(labels, want_labels) and torch.equal(roots, want_roots) and table.shape == (len(roots), 14)
    want = SS.observables(host(labels), host(want_sizes), host(xy), host(vv), host(p))
    assert SS.same(host(table), want) and len(roots) > 1 and (host(p) > 0).any()
    centers = pairs.cluster_centers(table)
    assert centers.shape == (len(roots), 2) and bool((centers[:, 0] >= table[:, 7]).all()) and bool((centers[:, 0] <= table[:, 8]).all())
    assert pairs.cluster_mean_velocities(table).shape == (len(roots), 2)
    twin = sc.Crate(U.scene(sc), noise="host", noise_seed=3, capacity=8 * first.engine.capacity)
    for _ in range(200):
        twin.physics_tick()
    assert all(torch.equal(a, b) for a, b in zip(state_of(twin), state_of(first)))
    for g, w in zip(twin.cluster_observables(), (labels, roots, table)):
        assert host(g).tobytes() == host(w).tobytes()
    # without a synchronisation, on torch's stream: the same table below min(C, K), and the counts last
    stream = torch.cuda.current_stream(torch.device("cuda", first.engine.device))
    first.engine.set_stream(stream.cuda_stream)
    try:
        for room in (len(roots) + 3, 2):
            out = first.cluster_observables(max_clusters=room)
            torch.cuda.synchronize()
            assert len(out) == 4 and out[3].cpu().tolist() == [n, len(roots)] and out[2].shape == (room, 14)
            k = min(room, len(roots))
            assert torch.equal(out[0][:n], labels) and torch.equal(out[1][:k], roots[:k])
            assert host(out[2][:k]).tobytes() == host(table[:k]).tobytes()
    finally:
        first.engine.use_own_stream()
    # a load with permuted ids: the rows are those of that crate's export
    ids = torch.from_numpy(np.random.RandomState(7).permutation(n) * 3 + 5).cuda()
    torch.cuda.synchronize()
    other = sc.Crate(U.scene(sc), noise="none", capacity=n + 100)
    other.load_state_tensors(xy, vv, ids)
    order = np.argsort(host(ids))
    labels, roots, table = other.cluster_observables(1.5 * other.diameter)
    sizes = other.cluster_tensors(1.5 * other.diameter)[1]
    want = SS.observables(host(labels), host(sizes), host(xy)[order], host(vv)[order], np.zeros(n))   # (pressures: zero after a load)
    assert SS.same(host(table), want)


def test_state_of_an_empty_crate(sc):
    crate = sc.Crate(U.scene(sc))
    labels, roots, table = crate.cluster_observables()                              # before the first tick: n = 0
    assert labels.shape == roots.shape == (0,) and table.shape == (0, 14)


# ---- 3. a pure function of the members' values

def test_same_bytes_repeated_after_half_and_full_and_after_another_reader(crate):
    import torch
    case = SK.cases()["ladder"]
    pts, values = case[0], case[1]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    want, total = spec("ladder", 8), len(case[3])

    def another_reader():                                                           # a table and a sum in between
        crate.engine.pairs_nearest(U.full((len(pts), 4), dev), k=4, counts=U.full(2, dev))

    results = [reduce(eng, pts, SK.RADIUS, values, half=True), reduce(eng, pts, SK.RADIUS, values, half=False),
               reduce(eng, pts, SK.RADIUS, values, half=True, repeat=3, between=another_reader)]
    for sums, mins, maxs, counts in results:
        assert counts.cpu().tolist() == [len(pts), total]
        assert_tables((sums[:total], mins[:total], maxs[:total]), want)
        assert all(bool((t[total:] == MARK).all()) for t in (sums, mins, maxs))


def test_a_fill_after_the_reduction_gives_the_list_it_gave_before(crate):
    import torch
    points, radius = CK.cases()["piles"]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(points)
    want = S.pairs(points, radius, False)
    offsets, counts, other, third = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev), U.full(2, dev)
    labels, again = U.full(n, dev), U.full(n, dev)
    partners = U.full(len(want[1]), dev)
    values = U.tensor(SK.table(97, n, 2))
    sums = marked((n, 2), dev)
    t = U.tensor(points)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=False)
    eng.pairs_label(labels, counts=other)
    eng.pairs_cluster_sums(values, sums, counts=third)
    eng.pairs_fill(partners)
    eng.pairs_label(again, counts=other)                                            # ... and another label
    eng.synchronize()
    assert counts.cpu().tolist() == [n, len(want[1])] and third.cpu().tolist() == other.cpu().tolist()
    assert host(offsets).tobytes() == want[0].tobytes() and host(partners).tobytes() == want[1].tobytes()
    assert torch.equal(labels, again)
    total = int(third[1])
    assert SS.same(host(sums[:total]), SS.cluster_sums(host(labels), host(values), clusters=total)[0])


# ---- 4. the room and the path that does not synchronise

@pytest.mark.parametrize("room", [0, 1, 5])
def test_room_below_the_cluster_count(crate, room):
    case = SK.cases()["ladder"]
    total = len(case[3])
    sums, mins, maxs, counts = reduce(crate.engine, case[0], SK.RADIUS, case[1], room=room)
    assert counts.cpu().tolist() == [len(case[0]), total] and room < total
    assert_tables((sums[:room], mins[:room], maxs[:room]), [w[:room] for w in spec("ladder", 8)])
    assert all(bool((t[room:] == MARK).all()) for t in (sums, mins, maxs))          # the mark stays from the room on


def test_max_clusters_does_not_synchronise_and_equals_the_default(crate, monkeypatch):
    import torch
    case = SK.cases()["ladder"]
    t, v = U.tensor(case[0]), U.tensor(case[1], 8)
    default = crate.cluster_sums(v, SK.RADIUS, points=t, extrema=True)
    n, total = len(case[0]), len(case[3])

    def forbidden(*args, **kw):
        raise AssertionError("the call synchronised")

    for room in (total + 50, total, 5):
        with monkeypatch.context() as m:
            m.setattr(type(crate.engine), "synchronize", forbidden)
            m.setattr(torch.cuda, "synchronize", forbidden)
            m.setattr(torch.cuda.Stream, "synchronize", forbidden)
            m.setattr(torch.Tensor, "item", forbidden)
            m.setattr(torch.Tensor, "cpu", forbidden)
            out = crate.cluster_sums(v, SK.RADIUS, points=t, extrema=True, max_clusters=room)
        crate.synchronize()
        assert len(out) == 7 and out[6].cpu().tolist() == [n, total]
        assert out[0].shape == (n,) and all(o.shape == (room,) for o in out[1:3]) and all(o.shape == (room, 8) for o in out[3:6])
        k = min(room, total)
        assert torch.equal(out[0], default[0])
        assert all(host(o[:k]).tobytes() == host(d[:k]).tobytes() for o, d in zip(out[1:6], default[1:6]))
    with pytest.raises(ValueError, match="max_clusters"):
        crate.cluster_sums(v, SK.RADIUS, points=t, max_clusters=-1)


# ---- 5. statuses and errors

def test_too_few_value_rows_and_the_domain(crate):
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    case = SK.cases()["special"]
    pts, values = case[0], case[1]
    n = len(pts)
    t, v = U.tensor(pts), U.tensor(values)
    with pytest.raises(ValueError, match="fewer"):
        crate.cluster_sums(v[:n - 1].contiguous(), SK.RADIUS, points=t)
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    labels, sums, mins = U.full(n, dev), marked((n, 2), dev), marked((n, 2), dev)
    eng.pairs_count(t, radius=SK.RADIUS, offsets=offsets, counts=counts)
    eng.pairs_label(labels, counts=counts)
    eng.pairs_cluster_sums(v[:n - 1].contiguous(), sums, mins, counts=out)
    eng.synchronize()
    assert out.cpu().tolist() == [U.SENTINEL, -2] and bool((sums == MARK).all()) and bool((mins == MARK).all())
    eng.pairs_cluster_sums(v, sums, mins, counts=out)                               # the call's own flag: gone with the call
    eng.synchronize()
    assert out.cpu().tolist() == [n, 4] and SS.same(host(sums[:4]), spec("special", 2)[0])
    short = crate.cluster_sums(v[:n - 1].contiguous(), SK.RADIUS, points=t, max_clusters=8)
    crate.synchronize()
    assert int(short[-1][1]) == -2
    # a coordinate outside the domain: -1, nothing else
    points, radius = K.outside_domain()
    t, v = U.tensor(points), U.tensor(SK.table(98, len(points), 2))
    with pytest.raises(ValueError, match="domain"):
        crate.cluster_sums(v, radius, points=t)
    offsets, out = U.full(len(points) + 1, dev), U.full(2, dev)
    labels, sums = U.full(len(points), dev), marked((len(points), 2), dev)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_label(labels, counts=counts)
    eng.pairs_cluster_sums(v, sums, counts=out)
    eng.synchronize()
    assert out.cpu().tolist() == [U.SENTINEL, -1] and bool((sums == MARK).all())


def test_state_and_argument_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    from sand_crate_amd import pairs
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    eng = crate.engine
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    n = len(points)
    t, v = U.tensor(points), U.tensor(SK.table(99, n, 2))
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    labels, sums, mins, maxs = U.full(n, dev), marked((n, 2), dev), marked((n, 2), dev), marked((n, 2), dev)
    torch.cuda.synchronize()
    args = (v, sums, mins, maxs)

    def untouched():
        eng.synchronize()
        return bool((counts == U.SENTINEL).all()) and all(bool((a == MARK).all()) for a in (sums, mins, maxs))

    assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE     # no count, no label
    other = U.full(2, dev)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=other)
    assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE     # a count, no label
    eng.pairs_label(labels, counts=other)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=other)
    assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE     # a count since the label
    eng.pairs_label(labels, counts=other)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=other, batch=pairs.batch_ptr([30, n - 30], dev))
    assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE     # a batched count: no label to read
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=other)
    eng.pairs_label(labels, counts=other)
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_cluster_sums_device
    for channels in (0, 9, -1):
        assert fn(ctx, ptr(v), n, channels, ptr(sums), ptr(mins), ptr(maxs), n, ptr(counts)) == N.ERR_ARG
    assert fn(ctx, ptr(v), n, 2, ptr(sums), None, None, -1, ptr(counts)) == N.ERR_ARG            # a negative room
    assert fn(ctx, ptr(v), -1, 2, ptr(sums), None, None, n, ptr(counts)) == N.ERR_ARG
    assert fn(ctx, N._P(v.data_ptr() + 8), n - 1, 2, ptr(sums), None, None, n, ptr(counts)) == N.ERR_ARG   # misaligned values
    assert fn(ctx, None, n, 2, ptr(sums), None, None, n, ptr(counts)) == N.ERR_ARG
    assert fn(ctx, ptr(v), n, 2, ptr(sums), None, None, n, None) == N.ERR_ARG
    assert lib.sc_last_error() and untouched()
    crate.particles = points                                                        # an upload since the label
    assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=other)
    eng.pairs_label(labels, counts=other)
    crate._send_tick_inputs()                                                       # inside a tick
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_cluster_sums, *args, counts=counts) == N.ERR_STATE
    finally:
        eng.step_finish()
    assert untouched()
    # no points at all: n = 0, C = 0, nothing written
    empty = U.tensor(np.zeros((0, 2)))
    eng.pairs_count(empty, radius=radius, offsets=U.full(1, dev), counts=other)
    eng.pairs_label(U.full(0, dev), counts=other)
    eng.pairs_cluster_sums(U.tensor(np.zeros((0, 2))), sums, mins, maxs, counts=counts)
    eng.synchronize()
    assert counts.cpu().tolist() == [0, 0] and all(bool((a == MARK).all()) for a in (sums, mins, maxs))
