"""GPU tests of the device pair search (sc_pairs_count_device / sc_pairs_fill_device, `Engine.pairs_count` /
`Engine.pairs_fill`, `Crate.pair_tensors`): offsets, partners and squared distances equal tests/pairs_spec.py bit for bit --
on every named case of tests/pairs_cases.py with and without `half`, on the state after real ticks, after a load and on an
empty crate --, a pair count beyond 31 bits against the closed form, searching changes nothing, `max_pairs` clips and
writes nothing past the room, the domain error and the error codes."""
import numpy as np
import pytest

import gpu_support as U
import pairs_cases as K
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_is_spec(got, points, radius, half):
    import torch
    offsets, partners, d2 = got
    assert offsets.dtype == partners.dtype == torch.int64 and d2.dtype == torch.float64
    want = S.pairs(points, radius, half)
    for g, w in zip((offsets, partners, d2), want):
        U.same_bytes(g.cpu().numpy(), w)


# ---- 1. every case on the points= path

@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("name", list(K.cases()))
def test_case_equals_the_spec(crate, name, half):
    points, radius = K.cases()[name]
    got = crate.pair_tensors(radius, points=U.tensor(points), half=half, squared_distances=True)
    assert len(got) == 3 and len(got[0]) == len(points) + 1
    assert_is_spec(got, points, radius, half)
    plain = crate.pair_tensors(radius, points=U.tensor(points), half=half)            # without the distances: the same list
    assert len(plain) == 2
    U.same_bytes(plain[0].cpu().numpy(), got[0].cpu().numpy())
    U.same_bytes(plain[1].cpu().numpy(), got[1].cpu().numpy())


def test_edge_index_of_a_case(crate):
    import torch
    from sand_crate_amd import pairs
    points, radius = K.cases()["n_257"]
    offsets, partners = crate.pair_tensors(radius, points=U.tensor(points))
    e = pairs.edge_index(offsets, partners)
    want = S.pairs(points, radius)
    assert e.shape == (2, len(want[1])) and e.is_cuda
    assert np.array_equal(e[0].cpu().numpy(), np.repeat(np.arange(len(points)), np.diff(want[0])))
    assert torch.equal(e[1], partners) and np.array_equal(pairs.row_lengths(offsets).cpu().numpy(), np.diff(want[0]))


# ---- 2. the state path

@pytest.fixture(scope="module")
def ticked(sc):
    crate = sc.Crate(U.scene(sc))
    for _ in range(200):
        crate.physics_tick()
    return crate


@pytest.mark.parametrize("factor", [1, 3])
def test_state_after_ticks(ticked, factor):
    crate = ticked
    radius = factor * crate.diameter
    particles, _, ids = crate.state_tensors(pressure=False, ids=True)
    points = particles.cpu().numpy()
    assert len(points) > 500 and np.array_equal(ids.cpu().numpy(), np.sort(ids.cpu().numpy()))
    for half in (False, True):
        got = crate.pair_tensors(radius, half=half, squared_distances=True)
        assert len(got[0]) == len(points) + 1
        assert_is_spec(got, points, radius, half)
    if factor == 1:
        default = crate.pair_tensors()                                              # radius defaults to the diameter
        want = S.pairs(points, crate.diameter)
        U.same_bytes(default[0].cpu().numpy(), want[0])
        U.same_bytes(default[1].cpu().numpy(), want[1])
        assert int(want[0][-1]) > len(points)                                       # a packed bed: some partners each


def test_state_right_after_a_load(sc, ticked):
    import torch
    particles, velocities, ids = ticked.state_tensors(pressure=False, ids=True)
    n = len(particles)
    order = torch.from_numpy(np.random.RandomState(5).permutation(n)).cuda()
    sparse = ids * 1000 + 17                                                        # sparse ids, shuffled storage order
    wc = U.scene(sc)
    other = sc.Crate(wc, noise="none", capacity=n + 100)
    p, v, i = particles[order].contiguous(), velocities[order].contiguous(), sparse[order].contiguous()
    torch.cuda.synchronize()
    other.load_state_tensors(p, v, i)
    points = other.state_tensors(pressure=False)[0].cpu().numpy()
    U.same_bytes(points, particles.cpu().numpy())                                     # index order is id order again
    radius = 3 * other.diameter
    assert_is_spec(other.pair_tensors(radius, squared_distances=True), points, radius, False)


def test_state_of_an_empty_crate(sc):
    wc = U.scene(sc)
    crate = sc.Crate(wc)
    offsets, partners, d2 = crate.pair_tensors(squared_distances=True)              # before the first tick
    assert offsets.cpu().tolist() == [0] and partners.shape == d2.shape == (0,)
    out = crate.pair_tensors(max_pairs=8)
    crate.synchronize()
    assert out[-1].cpu().tolist() == [0, 0] and int(out[0][0]) == 0


# ---- 3. reads only

def test_searching_changes_nothing(sc):
    def trajectory(searching):
        crate = sc.Crate(U.scene(sc))
        for _ in range(50):
            crate.physics_tick()
            if searching:
                crate.pair_tensors(squared_distances=True)
                crate.pair_tensors(2 * crate.diameter, max_pairs=1000)
        state = crate.engine.download()
        crate.sync_host_rng()
        rng = np.random.get_state()
        return state, (rng[1].copy(), rng[2])

    (a, rng_a), (b, rng_b) = trajectory(False), trajectory(True)
    assert len(a[0]) > 100
    for x, y in zip(a, b):
        U.same_bytes(x, y)
    assert np.array_equal(rng_a[0], rng_b[0]) and rng_a[1] == rng_b[1]


# ---- 4. max_pairs

def test_max_pairs_not_clipped_equals_the_default(crate):
    import torch
    points, radius = K.cases()["long_rows"]
    t = U.tensor(points)
    offsets, partners, d2 = crate.pair_tensors(radius, points=t, squared_distances=True)
    total = len(partners)
    out = crate.pair_tensors(radius, points=t, squared_distances=True, max_pairs=total + 50)
    crate.synchronize()
    assert len(out) == 4 and out[3].cpu().tolist() == [len(points), total]
    assert len(out[0]) == len(points) + 1 and len(out[1]) == len(out[2]) == total + 50
    assert torch.equal(out[0], offsets) and torch.equal(out[1][:total], partners) and torch.equal(out[2][:total], d2)
    out = crate.pair_tensors(radius, points=t, max_pairs=total)                     # exactly the room
    crate.synchronize()
    assert len(out) == 3 and torch.equal(out[1], partners)


@pytest.mark.parametrize("room", [0, 1, 1000, 70000])
def test_clipped_list_is_right_below_the_room_and_untouched_beyond(crate, room):
    import torch
    points, radius = K.cases()["long_rows"]                                         # about 160,000 entries; rows of 300 cross the room
    want = S.pairs(points, radius)
    assert int(want[0][-1]) > 70000
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(points)
    offsets = torch.full((n + 1,), U.SENTINEL, dtype=torch.int64, device=dev)
    counts = torch.full((2,), U.SENTINEL, dtype=torch.int64, device=dev)
    partners = torch.full((room + 64,), U.SENTINEL, dtype=torch.int64, device=dev)
    d2 = torch.full((room + 64,), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    t = U.tensor(points)
    assert eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts) is counts
    eng.pairs_fill(partners, d2, room=room)
    eng.synchronize()
    assert counts.cpu().tolist() == [n, int(want[0][-1])]
    U.same_bytes(offsets.cpu().numpy(), want[0])
    U.same_bytes(partners[:room].cpu().numpy(), want[1][:room])
    U.same_bytes(d2[:room].cpu().numpy(), want[2][:room])
    assert (partners[room:] == U.SENTINEL).all() and (d2[room:] == U.SENTINEL_FAR).all()


# ---- 5. a pair count beyond 31 bits

def test_big_pile_against_the_closed_form(sc):
    import torch
    n = K.BIG_PILE
    eng = sc.Engine(capacity=16)
    dev = torch.device("cuda", eng.device)
    points = torch.full((n, 2), 0.375, dtype=torch.float64, device=dev)
    room = 1 << 20
    for half in (False, True):
        offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        partners = torch.full((room + 64,), U.SENTINEL, dtype=torch.int64, device=dev)
        d2 = torch.full((room + 64,), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()
        eng.pairs_count(points, radius=0.01, offsets=offsets, counts=counts, half=half)
        eng.pairs_fill(partners, d2, room=room)
        eng.synchronize()
        want = S.coincident_offsets(n, half)
        assert counts.cpu().tolist() == [n, int(want[n])]
        if not half:
            assert int(want[n]) == 4294901760 and int(want[7]) == 7 * 65535
        U.same_bytes(offsets.cpu().numpy(), want)
        U.same_bytes(partners[:room].cpu().numpy(), S.coincident_partners(n, 0, room, half))
        assert not d2[:room].any() and (partners[room:] == U.SENTINEL).all() and (d2[room:] == U.SENTINEL_FAR).all()
    eng.close()


# ---- 6. the domain

def test_outside_the_domain(crate):
    import torch
    points, radius = K.outside_domain()
    t = U.tensor(points)
    with pytest.raises(ValueError, match="domain"):
        crate.pair_tensors(radius, points=t)
    # on the path that does not synchronise: E = -1, and nothing else is written
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    offsets = torch.full((len(points) + 1,), U.SENTINEL, dtype=torch.int64, device=dev)
    counts = torch.full((2,), U.SENTINEL, dtype=torch.int64, device=dev)
    partners = torch.full((100,), U.SENTINEL, dtype=torch.int64, device=dev)
    d2 = torch.full((100,), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_fill(partners, d2)
    eng.synchronize()
    assert counts.cpu().tolist() == [len(points), -1]
    assert (offsets == U.SENTINEL).all() and (partners == U.SENTINEL).all() and (d2 == U.SENTINEL_FAR).all()
    out = crate.pair_tensors(radius, points=t, max_pairs=100)
    crate.synchronize()
    assert int(out[-1][1]) == -1
    inside = points.copy()
    inside[33, 1] = np.nextafter(inside[33, 1], 0)                                  # one ulp inside: fine
    assert_is_spec(crate.pair_tensors(radius, points=U.tensor(inside), squared_distances=True), inside, radius, False)


# ---- 7. errors

def test_state_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    wc = U.scene(sc)
    crate = sc.Crate(wc, noise="none", capacity=512)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points, radius = K.cases()["n_65"]
    t = U.tensor(points)
    offsets = torch.zeros(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    partners = torch.full((4096,), U.SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert U.code_of(eng.pairs_fill, partners) == N.ERR_STATE                         # no count yet
    eng.pairs_count(t, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_fill(partners)                                                        # ... with one: fine, and again
    eng.pairs_fill(partners)
    crate.particles = points                                                        # an upload since the count
    assert U.code_of(eng.pairs_fill, partners) == N.ERR_STATE
    eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)
    eng.pairs_fill(partners)
    crate.physics_tick()                                                            # a tick since the count
    assert U.code_of(eng.pairs_fill, partners) == N.ERR_STATE
    eng.synchronize()
    # inside a tick
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_count, t, radius=radius, offsets=offsets, counts=counts) == N.ERR_STATE
        assert U.code_of(eng.pairs_fill, partners) == N.ERR_STATE
    finally:
        eng.step_finish()
    # a slab context has no state form, but searches a caller's points
    slab = sc.Engine(capacity=256)
    slab.set_slab(0, 50, 3, False, True)
    assert U.code_of(slab.pairs_count, None, radius=radius, offsets=offsets[:257], counts=counts) == N.ERR_STATE
    slab.pairs_count(t, radius=radius, offsets=offsets[:66], counts=counts)
    slab.pairs_fill(partners)
    slab.synchronize()
    want = S.pairs(points, radius)
    U.same_bytes(partners[:len(want[1])].cpu().numpy(), want[1])
    slab.close()


def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n = 300
    eng = sc.Engine(capacity=n + 64)
    rs = np.random.RandomState(3)
    eng.upload(rs.rand(n, 2), np.zeros((n, 2)))
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    t = U.tensor(rs.rand(n, 2))
    offsets = torch.full((n + 1,), U.SENTINEL, dtype=torch.int64, device=dev)
    counts = torch.full((2,), U.SENTINEL, dtype=torch.int64, device=dev)
    partners = torch.full((64,), U.SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    count = lib.sc_pairs_count_device
    assert count(None, ptr(t), n, 0.1, 0, ptr(offsets), n, ptr(counts)) == N.ERR_ARG
    assert count(ctx, ptr(t), n, 0.1, 0, None, n, ptr(counts)) == N.ERR_ARG
    assert count(ctx, ptr(t), n, 0.1, 0, ptr(offsets), n, None) == N.ERR_ARG
    assert count(ctx, N._P(t.data_ptr() + 8), n - 1, 0.1, 0, ptr(offsets), n, ptr(counts)) == N.ERR_ARG   # misaligned
    assert count(ctx, ptr(t), -1, 0.1, 0, ptr(offsets), n, ptr(counts)) == N.ERR_ARG
    assert count(ctx, ptr(t), n, 0.1, 0, ptr(offsets), -1, ptr(counts)) == N.ERR_ARG
    assert count(ctx, ptr(t), n, 0.1, 2, ptr(offsets), n, ptr(counts)) == N.ERR_ARG                        # unknown flags
    for radius in (0.0, -0.1, float("inf"), float("nan"), 1e-200, 1e200):
        assert count(ctx, ptr(t), n, radius, 0, ptr(offsets), n, ptr(counts)) == N.ERR_ARG
    # room one below the bound: refused before anything is launched, for the points and for the state
    assert count(ctx, ptr(t), n, 0.1, 0, ptr(offsets), n - 1, ptr(counts)) == N.ERR_CAPACITY
    assert count(ctx, None, 0, 0.1, 0, ptr(offsets), n - 1, ptr(counts)) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    fill = lib.sc_pairs_fill_device
    assert fill(None, ptr(partners), None, 64) == N.ERR_ARG
    assert fill(ctx, ptr(partners), None, 64) == N.ERR_STATE                                               # nothing was counted
    eng.synchronize()
    assert (offsets == U.SENTINEL).all() and (counts == U.SENTINEL).all() and (partners == U.SENTINEL).all()
    eng.pairs_count(t, radius=0.1, offsets=offsets, counts=counts)                                         # with the room: fine
    assert fill(ctx, None, None, 64) == N.ERR_ARG
    assert fill(ctx, ptr(partners), None, -1) == N.ERR_ARG
    eng.pairs_fill(partners)
    eng.synchronize()
    want = S.pairs(t.cpu().numpy(), 0.1)
    U.same_bytes(offsets.cpu().numpy(), want[0])
    U.same_bytes(partners.cpu().numpy(), want[1][:64])
    eng.close()
