"""GPU tests of the device state exchange (sc_export_state_device / sc_import_state_device, `Engine.export_state` /
`Engine.import_state`, `Crate.state_tensors` / `Crate.load_state_tensors`): the exported tensors hold bit for bit what
`Engine.download()` of the same context returns -- at the sizes where the sort's tiles, the scan's blocks and the gather's
blocks begin and end, with sparse and shuffled ids, after real ticks (emitting sources, fused ticks, a removal), after an
append, in slab mode --, exporting changes nothing, importing equals uploading, and the error codes."""
import copy

import numpy as np
import pytest

import gpu_support as U
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu


def launch_widths():
    from sand_crate_amd import _native as N
    return N.STATE_TILE, N.STATE_SCAN_BLOCK, N.STATE_GATHER_BLOCK


def edge_sizes():
    """0, 1, around a wave, and one below, at and above every width at which a launch of the export gains a workgroup:
    a tile of the sort (and a block of the gather), a block of the scan over the tiles' 256 digit counts (one more block
    per 8 tiles = 2048 keys), and two sizes with several scan blocks."""
    tile, scan, gather = launch_widths()
    sizes = {0, 1, 63, 64, 65}
    for w in (tile, gather, scan, 2 * scan, 32 * scan):
        sizes |= {w - 1, w, w + 1}
    assert max(sizes) <= 70000
    return sorted(sizes)


def cloud(seed, n, lo=0.05, hi=0.95):
    rs = np.random.RandomState(seed)
    return lo + (hi - lo) * rs.rand(n, 2), 0.2 * (rs.rand(n, 2) - 0.5)


def spread_crate(sc, n, seed=3, noise="none", capacity=None):
    crate = sc.Crate(U.spread_world(sc, n), noise=noise, noise_seed=1, capacity=capacity or n + 64)
    p, v = cloud(seed, n)
    crate.particles = p
    crate.particle_velocities = v
    return crate


def export(eng, room=None, extra=0):
    """-> (particles, velocities, pressure, ids) as NumPy arrays cut to the exported count, from tensors of `room` + `extra`
    rows filled with a sentinel; the rows past the count must still hold it."""
    import torch
    room = eng.capacity if room is None else room
    dev = torch.device("cuda", eng.device)
    rows = room + extra
    p = torch.full((rows, 2), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    v = torch.full((rows, 2), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    pr = torch.full((rows,), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    ids = torch.full((rows,), U.SENTINEL, dtype=torch.int64, device=dev)
    count = torch.full((1,), U.SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    assert eng.export_state(p, v, pr, ids, count=count, room=room) is count
    eng.synchronize()
    n = int(count.item())
    assert 0 <= n <= room
    assert (p[n:] == U.SENTINEL_FAR).all() and (v[n:] == U.SENTINEL_FAR).all() and (pr[n:] == U.SENTINEL_FAR).all()
    assert (ids[n:] == U.SENTINEL).all()
    return tuple(t[:n].cpu().numpy() for t in (p, v, pr, ids))


def assert_export_is_download(eng, **kw):
    got = export(eng, **kw)
    want = eng.download()
    for g, w in zip(got, want):
        U.same_bytes(g, w)
    return got


# ---- 1. sizes at the edges

@pytest.mark.parametrize("n", edge_sizes())
def test_sizes_at_the_edges(sc, n):
    eng = sc.Engine(capacity=n + 64)
    p, v = cloud(n, n)
    order = np.random.RandomState(n + 1).permutation(n)        # storage order is not id order
    eng.upload_with_ids(p[order], v[order], order.astype(np.int64))
    gp, gv, gpr, gids = assert_export_is_download(eng, extra=3)
    assert len(gids) == n and np.array_equal(gids, np.arange(n)) and not gpr.any()
    U.same_bytes(gp, p)
    U.same_bytes(gv, v)
    eng.upload(p, v)                                            # a fresh upload: particle i gets id i
    gp, _, gpr, gids = assert_export_is_download(eng)
    assert np.array_equal(gids, np.arange(n)) and not gpr.any()
    U.same_bytes(gp, p)
    eng.close()


# ---- 2. sparse ids

@pytest.mark.parametrize("top", [2 ** 20 + 1, 2 ** 31 - 2])
def test_sparse_ids_in_shuffled_storage_order(sc, top):
    ids = np.array(sorted({0, 31, 32, 33, 63, 64, 255, 256, 257, 1023, 1024, 65535, 65536, 2 ** 20 + 1, 2 ** 24, top}), dtype=np.int64)
    n = len(ids)
    p, v = cloud(5, n)
    order = np.random.RandomState(6).permutation(n)
    eng = sc.Engine(capacity=n + 7)
    eng.upload_with_ids(p[order], v[order], ids[order])
    gp, gv, _, gids = assert_export_is_download(eng)
    assert np.array_equal(gids, ids)
    U.same_bytes(gp, p)
    U.same_bytes(gv, v)
    eng.close()


# ---- 3. after real ticks

def test_after_ticks_with_emitting_sources(sc):
    crate = sc.Crate(U.scene(sc), noise="host")                # the sources emit on the device: ids grow, storage is cell-sorted
    counts = []
    for tick in range(1, 41):
        crate.physics_tick()
        if tick in (1, 2, 40):
            _, _, pr, ids = assert_export_is_download(crate.engine)
            counts.append(len(ids))
            assert len(ids) > 0 and np.array_equal(ids, np.sort(ids))
            assert (pr > 0).any() or tick == 1
    assert counts[0] < counts[1] < counts[2]
    p, v, pr = crate.state_tensors()                            # the crate's own form: the attributes, on the device
    U.same_bytes(p.cpu().numpy(), crate.particles)
    U.same_bytes(v.cpu().numpy(), crate.particle_velocities)
    U.same_bytes(pr.cpu().numpy(), crate.particles_pressure)
    assert crate.particle_count == len(p)


def test_after_fused_ticks(sc):
    crate = spread_crate(sc, 3000)
    crate.run(8)                                                # every tick but the last rides on its predecessor's force kernel
    _, _, pr, ids = assert_export_is_download(crate.engine)
    assert len(ids) == 3000 and (pr > 0).any()


def test_after_a_removal_the_ids_have_a_gap(sc):
    from oracle.tick import remove_outside
    n = 500
    crate = sc.Crate(U.spread_world(sc, n), noise="none", capacity=n + 64)
    p, v = cloud(8, n)
    r = crate.particle_radius
    p[123] = (0.5, 1.0 + 1.5 * r)                               # crate.py:152: a coordinate above 1 + r is removed
    kept = remove_outside(p, v, r, np.arange(n))[2]
    assert len(kept) == n - 1 and 123 not in kept
    crate.particles = p
    crate.particle_velocities = v
    crate.physics_tick()
    _, _, _, ids = assert_export_is_download(crate.engine)
    assert np.array_equal(ids, kept)


# ---- 4. pressure validity

def test_appended_slots_carry_no_pressure(sc):
    crate = spread_crate(sc, 700)
    crate.physics_tick()
    more, more_v = cloud(9, 3)
    crate.engine.append(more, more_v)
    gp, _, pr, ids = assert_export_is_download(crate.engine)
    assert np.array_equal(ids, np.arange(703)) and not pr[700:].any() and (pr[:700] > 0).any()
    U.same_bytes(gp[700:], more)


# ---- 5. slabs

def test_slab_contexts_export_their_own_download(sc):
    import bench
    from sand_crate_amd.slab import SlabChain
    n = 4000
    wc, _ = bench.world_for(n)
    p, v = bench.synthetic_state(n)
    chain = SlabChain(copy.deepcopy(wc), p, v, 2, noise="counter", noise_seed=1)
    chain.run(3)
    chain.synchronize()
    total = 0
    for member in chain.members:
        eng = member.engine
        _, _, _, ids = assert_export_is_download(eng)           # ghost copies are skipped
        assert len(ids) == eng.owned_count() <= eng.count()
        total += len(ids)
    assert total == n


# ---- 6. reads only

def test_exporting_changes_nothing(sc):
    import torch

    def trajectory(exporting):
        crate = spread_crate(sc, 1500, noise="counter")
        for _ in range(10):
            crate.physics_tick()
            if exporting:
                out = crate.state_tensors(ids=True, sync=False)
                assert len(out) == 5 and all(len(t) == crate.engine.capacity for t in out[:4]) and out[4].shape == (1,)
        return crate.engine.download()

    for a, b in zip(trajectory(False), trajectory(True)):
        U.same_bytes(a, b)
    crate = spread_crate(sc, 1500, noise="counter")
    crate.run(3)
    first = crate.state_tensors(ids=True)
    second = crate.state_tensors(ids=True)
    assert len(first) == 4 and all(torch.equal(a, b) for a, b in zip(first, second))
    p, v = crate.state_tensors(pressure=False)
    assert torch.equal(p, first[0]) and torch.equal(v, first[1]) and crate.particle_count == len(p) == 1500


# ---- 7. import

def tensors(*arrays):
    import torch
    out = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)
    torch.cuda.synchronize()
    return out


def test_load_state_tensors_equals_upload(sc):
    n = 1200
    p, v = cloud(11, n)
    ids = np.sort(np.random.RandomState(12).choice(50000, n, replace=False)).astype(np.int64)
    order = np.random.RandomState(13).permutation(n)
    for with_ids in (False, True):
        a = sc.Crate(U.spread_world(sc, n), noise="none", capacity=n + 64)
        b = sc.Crate(U.spread_world(sc, n), noise="none", capacity=n + 64)
        if with_ids:
            a.engine.upload_with_ids(p[order], v[order], ids[order])
            b.load_state_tensors(*tensors(p[order], v[order], ids[order]))
        else:
            a.engine.upload(p, v)
            b.load_state_tensors(*tensors(p, v))
        assert b.particle_count == n
        for x, y in zip(a.engine.download(), b.engine.download()):
            U.same_bytes(x, y)
        for crate in (a, b):
            crate._state_changed()
            crate.physics_tick()
        for x, y in zip(a.engine.download(), b.engine.download()):
            U.same_bytes(x, y)
        U.same_bytes(b.particles, a.engine.download()[0])


def test_round_trip_into_a_fresh_crate(sc):
    n = 900
    a = spread_crate(sc, n)
    for _ in range(5):
        a.physics_tick()
    p, v, ids = a.state_tensors(pressure=False, ids=True)
    b = sc.Crate(U.spread_world(sc, n), noise="none", capacity=n + 64)
    for body_a, body_b in zip(a.rigid_bodies, b.rigid_bodies):   # the walls where crate A has them
        body_b.__dict__.update(copy.deepcopy(body_a.__dict__))
    b.load_state_tensors(p, v, ids)
    b.engine.restore_counters(5, n)
    b.tick = a.tick
    for _ in range(5):
        a.physics_tick()
        b.physics_tick()
    for x, y in zip(a.engine.download(), b.engine.download()):
        U.same_bytes(x, y)


def test_import_refuses_ids_out_of_range(sc):
    from sand_crate_amd import _native as N
    n = 300
    crate = spread_crate(sc, n)
    crate.physics_tick()
    before = crate.engine.download()
    p, v = cloud(14, 70)
    for bad in (2 ** 31 - 1, -1, 2 ** 40):
        ids = np.arange(70, dtype=np.int64)
        ids[69] = bad
        assert U.code_of(crate.engine.import_state, *tensors(p, v, ids)) == N.ERR_ARG
        for x, y in zip(before, crate.engine.download()):       # the context still holds its old state, pressures included
            U.same_bytes(x, y)
    ids[69] = 2 ** 31 - 2                                        # the largest id there is
    crate.engine.import_state(*tensors(p, v, ids))
    assert crate.engine.download()[3].tolist() == ids.tolist()


def test_import_beyond_the_capacity(sc):
    from sand_crate_amd import _native as N
    crate = spread_crate(sc, 100, capacity=128)
    before = crate.engine.download()
    p, v = cloud(15, 129)
    assert U.code_of(crate.engine.import_state, *tensors(p, v)) == N.ERR_CAPACITY
    for x, y in zip(before, crate.engine.download()):
        U.same_bytes(x, y)
    old = crate.engine
    crate.load_state_tensors(*tensors(p, v))                    # the crate grows into a larger context
    assert crate.engine is not old and crate.engine.capacity >= 129 and crate.particle_count == 129
    U.same_bytes(crate.particles, p)
    U.same_bytes(crate.particle_velocities, v)
    U.same_bytes(crate.state_tensors()[0].cpu().numpy(), p)


# ---- 8. errors

def test_state_error_inside_a_tick(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc), noise="host-sync")
    crate.physics_tick()
    eng = crate.engine
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    p, v = tensors(*cloud(16, 10))
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(eng.export_state, count=count, room=eng.capacity) == N.ERR_STATE
        assert U.code_of(eng.import_state, p, v) == N.ERR_STATE
        stats = eng.step_stats()
        eng.set_noise_host(np.random.rand(stats.neighbor_slots, 2))
    finally:
        eng.step_finish()
    assert_export_is_download(eng)


def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n = 300
    eng = sc.Engine(capacity=n + 64)
    eng.upload(*cloud(17, n))
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    p = torch.full((n, 2), U.SENTINEL_FAR, dtype=torch.float64, device=dev)
    ids = torch.full((n,), U.SENTINEL, dtype=torch.int64, device=dev)
    count = torch.full((1,), U.SENTINEL, dtype=torch.int64, device=dev)
    torch.cuda.synchronize(dev)
    ptr = lambda t: N._P(t.data_ptr())  # noqa: E731
    assert lib.sc_export_state_device(ctx, ptr(p), None, None, ptr(ids), n, None) == N.ERR_ARG        # no count pointer
    assert lib.sc_export_state_device(ctx, ptr(p), None, None, ptr(ids), -1, ptr(count)) == N.ERR_ARG
    assert lib.sc_export_state_device(None, ptr(p), None, None, ptr(ids), n, ptr(count)) == N.ERR_ARG
    assert lib.sc_export_state_device(ctx, N._P(p.data_ptr() + 8), None, None, None, n - 1, ptr(count)) == N.ERR_ARG
    assert lib.sc_import_state_device(None, ptr(p), ptr(p), None, n) == N.ERR_ARG
    assert lib.sc_import_state_device(ctx, ptr(p), None, None, n) == N.ERR_ARG
    assert lib.sc_import_state_device(ctx, ptr(p), ptr(p), None, -1) == N.ERR_ARG
    # room one below the bound of the stored count: refused before anything is launched
    assert U.code_of(eng.export_state, p[:n - 1], ids=ids[:n - 1], count=count) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    eng.synchronize()
    assert (p == U.SENTINEL_FAR).all() and (ids == U.SENTINEL).all() and int(count.item()) == U.SENTINEL
    eng.export_state(p, ids=ids, count=count)                                                         # with the room: fine
    eng.synchronize()
    assert int(count.item()) == n and np.array_equal(ids.cpu().numpy(), np.arange(n))
    U.same_bytes(p.cpu().numpy(), eng.download()[0])
    eng.close()
