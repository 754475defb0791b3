"""GPU tests of the device cluster labelling (sc_pairs_label_device, `Engine.pairs_label`, `Crate.cluster_tensors`): labels,
sizes and roots equal tests/cluster_spec.py exactly -- on every small case of tests/cluster_cases.py, on 70,001 points
against the spec's label propagation over the device's own pair list, on the state after ticks and a load with permuted
ids --, the same bytes after a half and a full count and when repeated, a fill after the label, a room below the cluster
count, the domain error, the error codes and the path that does not synchronise."""
import functools

import numpy as np
import pytest

import cluster_cases as CK
import cluster_spec as CS
import gpu_support as U
import pairs_cases as K
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def spec(name):
    return CS.clusters(*CK.cases()[name])


def assert_same(got, want):
    import torch
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        g = g.cpu().numpy() if isinstance(g, torch.Tensor) else g
        assert g.dtype == w.dtype == np.int64 and g.shape == w.shape and g.tobytes() == w.tobytes()


def label(eng, points, radius, *, half, rooms=None, twice=False):
    """count + label through the engine into sentinel-filled tensors -> (labels, sizes, roots, counts), synchronised."""
    import torch
    dev = torch.device("cuda", eng.device)
    n = len(points)
    room = n if rooms is None else rooms
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    labels, sizes, roots = U.full(n + 8, dev), U.full(room + 8, dev), U.full(room + 8, dev)
    t = U.tensor(points)
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
    for _ in range(2 if twice else 1):
        assert eng.pairs_label(labels, sizes, roots, counts=counts, room=n, room_clusters=room) is counts
    eng.synchronize()
    return labels, sizes, roots, counts


# ---- 1. every case on the points= path

@pytest.mark.parametrize("name", list(CK.small_cases()))
def test_case_equals_the_spec(crate, name):
    points, radius = CK.cases()[name]
    got = crate.cluster_tensors(radius, points=U.tensor(points))
    assert all(t.is_cuda for t in got)
    assert_same(got, spec(name))


def test_wide_equals_the_propagation_over_the_device_list(crate):
    points, radius = CK.cases()["wide"]
    t = U.tensor(points)
    offsets, partners = crate.pair_tensors(radius, points=t, half=True)
    want = CS.components(len(points), offsets.cpu().numpy(), partners.cpu().numpy())
    assert 100 < len(want[1]) < len(points) // 4 and want[1].max() > 1000        # near percolation: big and small ones
    assert_same(crate.cluster_tensors(radius, points=t), want)


# ---- 2. a pure function of the points

@pytest.mark.parametrize("name", ["n_4097_partners_4.5", "serpentine_shuffled", "lattice", "piles", "not_finite"])
def test_half_full_and_repeated_give_the_same_bytes(crate, name):
    points, radius = CK.cases()[name]
    n, want = len(points), spec(name)
    total = len(want[1])
    results = [label(crate.engine, points, radius, half=True), label(crate.engine, points, radius, half=False),
               label(crate.engine, points, radius, half=True, twice=True)]
    for labels, sizes, roots, counts in results:
        assert counts.cpu().tolist() == [n, total]
        assert_same((labels[:n], sizes[:total], roots[:total]), want)
        assert (labels[n:] == U.SENTINEL).all() and (sizes[total:] == U.SENTINEL).all() and (roots[total:] == U.SENTINEL).all()


def test_a_fill_after_the_label_still_matches(crate):
    import torch
    points, radius = CK.cases()["piles"]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(points)
    for half in (False, True):
        want = S.pairs(points, radius, half)
        offsets, counts, other = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
        labels = U.full(n, dev)
        partners = U.full(len(want[1]), dev)
        d2 = torch.full((len(want[1]),), -1.5, dtype=torch.float64, device=dev)
        t = U.tensor(points)
        eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts, half=half)
        eng.pairs_label(labels, counts=other)                                       # without sizes and roots
        eng.pairs_fill(partners, d2)
        eng.synchronize()
        assert counts.cpu().tolist() == [n, len(want[1])] and other.cpu().tolist() == [n, len(spec("piles")[1])]
        for g, w in zip((offsets, partners, d2), want):
            assert g.cpu().numpy().tobytes() == w.tobytes()
        assert labels.cpu().numpy().tobytes() == spec("piles")[0].tobytes()


# ---- 3. the room

@pytest.mark.parametrize("room", [0, 1, 7, 300])
def test_room_below_the_cluster_count(crate, room):
    name = "n_2049_partners_2.0"
    points, radius = CK.cases()[name]
    want = spec(name)
    n, total = len(points), len(want[1])
    assert total > 300
    labels, sizes, roots, counts = label(crate.engine, points, radius, half=True, rooms=room)
    assert counts.cpu().tolist() == [n, total]
    assert_same((labels[:n], sizes[:room], roots[:room]), (want[0], want[1][:room], want[2][:room]))
    assert (labels[n:] == U.SENTINEL).all() and (sizes[room:] == U.SENTINEL).all() and (roots[room:] == U.SENTINEL).all()


# ---- 4. the domain

def test_outside_the_domain(crate):
    points, radius = K.outside_domain()
    t = U.tensor(points)
    with pytest.raises(ValueError, match="domain"):
        crate.cluster_tensors(radius, points=t)
    labels, sizes, roots, counts = label(crate.engine, points, radius, half=True)
    assert counts.cpu().tolist() == [len(points), -1]                               # (n is the count's; the label wrote -1)
    assert (labels == U.SENTINEL).all() and (sizes == U.SENTINEL).all() and (roots == U.SENTINEL).all()
    import torch
    alone = U.full(2, torch.device("cuda", crate.engine.device))
    crate.engine.pairs_label(labels, sizes, roots, counts=alone)                    # counts[1] = -1 and nothing else
    crate.engine.synchronize()
    assert alone.cpu().tolist() == [U.SENTINEL, -1] and (labels == U.SENTINEL).all()
    out = crate.cluster_tensors(radius, points=t, max_clusters=16)
    crate.synchronize()
    assert int(out[-1][1]) == -1
    inside = points.copy()
    inside[33, 1] = np.nextafter(inside[33, 1], 0)                                  # one ulp inside: fine
    assert_same(crate.cluster_tensors(radius, points=U.tensor(inside)), CS.clusters(inside, radius))


# ---- 5. the state form

def test_state_after_ticks_and_a_load_with_permuted_ids(sc):
    import torch
    from sand_crate_amd import pairs
    first = sc.Crate(U.scene(sc))
    for _ in range(40):
        first.physics_tick()
    particles, velocities = first.state_tensors(pressure=False)
    n = len(particles)
    assert n > 100
    points = particles.cpu().numpy()
    assert_same(first.cluster_tensors(), CS.clusters(points, first.diameter))       # radius defaults to the diameter
    ids = torch.from_numpy(np.random.RandomState(7).permutation(n) * 3 + 5).cuda()  # row k gets id ids[k]: sparse, shuffled
    torch.cuda.synchronize()
    other = sc.Crate(U.scene(sc), noise="none", capacity=n + 100)
    other.load_state_tensors(particles, velocities, ids)
    exported, _, exported_ids = other.state_tensors(pressure=False, ids=True)
    order = np.argsort(ids.cpu().numpy())
    assert np.array_equal(exported_ids.cpu().numpy(), ids.cpu().numpy()[order])
    assert np.array_equal(exported.cpu().numpy(), points[order]) and not np.array_equal(order, np.arange(n))
    for factor in (1.0, 1.5):
        radius = factor * other.diameter
        labels, sizes, roots = other.cluster_tensors(radius)
        want = CS.clusters(points[order], radius)                                   # labels index rows of that export
        assert_same((labels, sizes, roots), want)
        assert len(labels) == n and torch.equal(labels[roots], torch.arange(len(roots), device=labels.device))
        c, size = pairs.largest_cluster(sizes)
        assert size == want[1].max() and int((pairs.cluster_size_of(labels, sizes) == size).sum()) >= size
    assert other.particle_count == n


def test_state_of_an_empty_crate(sc):
    crate = sc.Crate(U.scene(sc))
    labels, sizes, roots = crate.cluster_tensors()                                  # before the first tick
    assert labels.shape == sizes.shape == roots.shape == (0,)
    out = crate.cluster_tensors(max_clusters=4)
    crate.synchronize()
    assert out[-1].cpu().tolist() == [0, 0]


def test_labelling_changes_nothing(sc):
    def trajectory(labelling):
        crate = sc.Crate(U.scene(sc))
        for _ in range(30):
            crate.physics_tick()
            if labelling:
                crate.cluster_tensors()
                crate.cluster_tensors(2 * crate.diameter, max_clusters=10)
        state = crate.engine.download()
        crate.sync_host_rng()
        rng = np.random.get_state()
        return state, (rng[1].copy(), rng[2])

    (a, rng_a), (b, rng_b) = trajectory(False), trajectory(True)
    assert len(a[0]) > 100
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert np.array_equal(rng_a[0], rng_b[0]) and rng_a[1] == rng_b[1]


# ---- 6. errors

def test_state_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc), noise="none", capacity=512)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    t = U.tensor(points)
    offsets = torch.zeros(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    labels, sizes, roots = U.full(eng.capacity, dev), U.full(eng.capacity, dev), U.full(eng.capacity, dev)
    torch.cuda.synchronize()
    args = (labels, sizes, roots)
    assert U.code_of(eng.pairs_label, *args, counts=counts) == N.ERR_STATE            # no count yet
    eng.synchronize()
    assert (labels == U.SENTINEL).all() and (sizes == U.SENTINEL).all() and (roots == U.SENTINEL).all()
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_label(*args, counts=counts)                                           # ... with one: fine, and again
    eng.pairs_label(*args, counts=counts)
    crate.particles = points                                                        # an upload since the count
    assert U.code_of(eng.pairs_label, *args, counts=counts) == N.ERR_STATE
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_label(*args, counts=counts)
    eng.append(points[:3] + 2.0, np.zeros((3, 2)))                                  # an append since the count
    assert U.code_of(eng.pairs_label, *args, counts=counts) == N.ERR_STATE
    crate.particles = points
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_label(*args, counts=counts)
    crate.physics_tick()                                                            # a tick since the count
    assert U.code_of(eng.pairs_label, *args, counts=counts) == N.ERR_STATE
    eng.synchronize()
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    crate._send_tick_inputs()                                                       # inside a tick
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_label, *args, counts=counts) == N.ERR_STATE
    finally:
        eng.step_finish()


def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n = 300
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points = np.random.RandomState(3).rand(n, 2)
    t = U.tensor(points)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    labels, sizes, roots, out = U.full(n, dev), U.full(n, dev), U.full(n, dev), U.full(2, dev)
    torch.cuda.synchronize()
    eng.pairs_count(t, radius=0.05, offsets=offsets, counts=counts)
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_label_device
    assert fn(None, ptr(labels), n, ptr(sizes), ptr(roots), n, ptr(out)) == N.ERR_ARG
    assert fn(ctx, None, n, ptr(sizes), ptr(roots), n, ptr(out)) == N.ERR_ARG
    assert fn(ctx, ptr(labels), n, ptr(sizes), ptr(roots), n, None) == N.ERR_ARG
    assert fn(ctx, ptr(labels), -1, ptr(sizes), ptr(roots), n, ptr(out)) == N.ERR_ARG
    assert fn(ctx, ptr(labels), n, ptr(sizes), ptr(roots), -1, ptr(out)) == N.ERR_ARG
    assert fn(ctx, ptr(labels), n - 1, ptr(sizes), ptr(roots), n, ptr(out)) == N.ERR_CAPACITY      # short labels
    assert U.code_of(eng.pairs_label, labels[:n - 1], sizes, roots, counts=out) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    eng.synchronize()
    for a in (labels, sizes, roots, out):
        assert (a == U.SENTINEL).all()
    eng.pairs_label(labels, None, roots, counts=out)                                # sizes or roots alone: fine
    eng.pairs_label(labels, sizes, None, counts=out)
    eng.synchronize()
    assert_same((labels, sizes[:int(out[1])], roots[:int(out[1])]), CS.clusters(points, 0.05))
    eng.close()


# ---- 7. the path that does not synchronise

def test_max_clusters_does_not_synchronise_and_equals_the_default(crate, monkeypatch):
    import torch
    name = "n_2049_partners_4.5"
    points, radius = CK.cases()[name]
    t = U.tensor(points)
    labels, sizes, roots = crate.cluster_tensors(radius, points=t)
    n, total = len(points), len(sizes)
    assert_same((labels, sizes, roots), spec(name))

    def forbidden(*args, **kw):
        raise AssertionError("the call synchronised")

    for room in (total + 50, total, 5):
        with monkeypatch.context() as m:
            m.setattr(type(crate.engine), "synchronize", forbidden)
            m.setattr(torch.cuda, "synchronize", forbidden)
            m.setattr(torch.cuda.Stream, "synchronize", forbidden)
            m.setattr(torch.Tensor, "item", forbidden)
            m.setattr(torch.Tensor, "cpu", forbidden)
            out = crate.cluster_tensors(radius, points=t, max_clusters=room)
        crate.synchronize()
        assert len(out) == 4 and out[3].cpu().tolist() == [n, total]
        assert out[0].shape == (n,) and out[1].shape == out[2].shape == (room,)
        k = min(room, total)
        assert torch.equal(out[0], labels) and torch.equal(out[1][:k], sizes[:k]) and torch.equal(out[2][:k], roots[:k])
    with pytest.raises(ValueError, match="max_clusters"):
        crate.cluster_tensors(radius, points=t, max_clusters=-1)
