"""GPU tests of the device ray sensors (sc_pairs_rays_device, `Engine.pairs_rays`, `Crate.ray_tensors`): t and hit equal
tests/ray_spec.py bit for bit -- every case of tests/ray_cases.py, through the crate and through the engine,
synchronising and not --; the state form after ticks; a fan from inside the
closed box always ends somewhere; capacity independence; a raised status writes counts[1] and nothing else; the
workspace of the count is left as it is; the error codes."""
import functools

import numpy as np
import pytest

import gpu_support as U
import pairs_spec as S
import ray_cases as K
import ray_spec as RS
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def spec(name):
    c = K.cases()[name]
    return RS.rays(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t)


def through_the_engine(eng, c, *, spare=8, rho=None, walls=True):
    """count + rays through the engine into sentinel-filled tensors with `spare` rows of room beyond the rays ->
    (t, hit, counts), synchronised.  The float t holds the integer sentinel too: `U.untouched(..., sentinel=U.SENTINEL)`."""
    import torch
    dev = torch.device("cuda", eng.device)
    n, rays = len(c.points), len(c.origins)
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    t, hit = U.full(rays + spare, dev, dtype=torch.float64), U.full(rays + spare, dev)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)                # (alive until the synchronisation)
    eng.pairs_count(p, radius=float(2 * c.rho if c.radius is None else c.radius), offsets=offsets, counts=counts)
    assert eng.pairs_rays(t, hit, origins=o, directions=d, disc_radius=c.rho if rho is None else rho, max_t=c.max_t,
                          segments=c.walls if walls else None, counts=out) is out
    eng.synchronize()
    return t, hit, out


# ---- 1. every case, through the crate and the engine, synchronising and not

@pytest.mark.parametrize("name", K.served())
def test_case_equals_the_spec(crate, name):
    c = K.cases()[name]
    want_t, want_hit = spec(name)
    rays = len(want_t)
    t, hit, counts = through_the_engine(crate.engine, c)
    assert counts.cpu().tolist() == [rays, 0]
    assert U.same_values_signs(t[:rays], want_t) and U.same_values_signs(hit[:rays], want_hit) and \
        U.untouched(t[rays:], hit[rays:], sentinel=U.SENTINEL)
    if c.radius is not None:
        return                                                                      # (the crate counts at 2 rho)
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    t, hit = crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, points=points)
    assert t.is_cuda and hit.is_cuda and U.same_values_signs(t, want_t) and U.same_values_signs(hit, want_hit)
    out = crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, points=points, sync=False)
    crate.synchronize()
    assert len(out) == 3 and out[2].cpu().tolist() == [rays, 0] and U.same_values_signs(out[0], want_t) and \
        U.same_values_signs(out[1], want_hit)
    # walls alone and particles alone are the spec's, too
    alone = RS.rays(None, c.walls, c.origins, c.directions, c.rho, c.max_t)
    t, hit = crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, particles=False, points=points)
    assert U.same_values_signs(t, alone[0]) and U.same_values_signs(hit, alone[1])
    if RS.status(c.points, None, c.origins, c.directions, c.rho, c.max_t) == 0:
        alone = RS.rays(c.points, None, c.origins, c.directions, c.rho, c.max_t)
        t, hit = crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=False, points=points)
        assert U.same_values_signs(t, alone[0]) and U.same_values_signs(hit, alone[1])


# ---- 2. the state form, and a fan in the closed box

def test_state_after_ticks_and_a_fan_in_the_box(sc):
    import torch
    from sand_crate_amd import _native as N
    from sand_crate_amd import pairs
    crate = sc.Crate(U.scene(sc))
    for _ in range(40):
        crate.physics_tick()
    particles, = crate.state_tensors(pressure=False)[:1]
    host = particles.cpu().numpy()
    n = len(host)
    walls = crate.segments
    lo, hi = walls.reshape(-1, 2).min(axis=0), walls.reshape(-1, 2).max(axis=0)
    reach = float(np.hypot(*(hi - lo)))
    o, d = pairs.ray_fan((0.5, 0.5), 257, 0.0, 2 * np.pi, device=particles.device)  # inside the unit box of the scene
    torch.cuda.synchronize()
    t, hit = crate.ray_tensors(o, d, reach)
    assert n > 100 and crate.particle_count == n and t.shape == hit.shape == (257,)
    want = RS.rays(host, walls, o.cpu().numpy(), d.cpu().numpy(), crate.diameter / 2, reach)
    assert U.same_values_signs(t, want[0]) and U.same_values_signs(hit, want[1])
    assert int((hit == -1).sum()) == 0 and bool(torch.isfinite(t).all())         # the box is closed
    assert int((pairs.hit_walls(hit) >= 0).sum()) + int((pairs.hit_particles(hit) >= 0).sum()) == 257
    as_points = crate.ray_tensors(o, d, reach, points=particles)
    assert torch.equal(t, as_points[0]) and torch.equal(hit, as_points[1])
    ends = pairs.ray_points(o, d, t).cpu().numpy()
    assert (ends >= lo - 1e-9).all() and (ends <= hi + 1e-9).all()
    # looking down on the surface from the top of the box (gravity points along +y): a particle or the floor
    xs = np.linspace(0.01, 0.99, 64)
    down_o = U.tensor(np.stack([xs, np.full(64, 0.01)], axis=1))
    down_d = U.tensor(np.tile([0.0, 1.0], (64, 1)))
    t, hit = crate.ray_tensors(down_o, down_d, reach)
    want = RS.rays(host, walls, down_o.cpu().numpy(), down_d.cpu().numpy(), crate.diameter / 2, reach)
    assert U.same_values_signs(t, want[0]) and U.same_values_signs(hit, want[1]) and int((hit >= 0).sum()) > 0 and \
        int((hit == -1).sum()) == 0
    # a tick since the count: the grid is stale
    eng = crate.engine
    dev = particles.device
    out_t, out_hit, counts = U.full(64, dev, dtype=torch.float64), U.full(64, dev), U.full(2, dev)
    crate.physics_tick()
    assert U.code_of(eng.pairs_rays, out_t, out_hit, origins=down_o, directions=down_d, disc_radius=crate.diameter / 2,
                     max_t=1.0, counts=counts) == N.ERR_STATE
    eng.synchronize()
    assert U.untouched(out_t, out_hit, counts, sentinel=U.SENTINEL)


def test_the_capacity_does_not_reach_the_result(sc):
    import torch
    c = K.cases()["dense"]
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    results = []
    for capacity in (256, 100_000):
        crate = sc.Crate(U.scene(sc), noise="none", capacity=capacity)
        results.append(crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, points=points))
    assert all(torch.equal(a, b) or U.same_values_signs(a, b.cpu().numpy()) for a, b in zip(*results))
    assert U.same_values_signs(results[0][0], spec("dense")[0]) and U.same_values_signs(results[0][1], spec("dense")[1])


# ---- 3. the status

@pytest.mark.parametrize("name", K.refused())
def test_a_status_writes_counts_1_and_nothing_else(crate, name):
    c = K.cases()[name]
    status = c.claims["status"]
    t, hit, counts = through_the_engine(crate.engine, c)
    assert counts.cpu().tolist() == [U.SENTINEL, status] and U.untouched(t, hit, sentinel=U.SENTINEL)
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    with pytest.raises(ValueError, match="max_t" if status == -4 else "domain"):
        crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, points=points)
    out = crate.ray_tensors(o, d, c.max_t, disc_radius=c.rho, walls=c.walls, points=points, sync=False)
    crate.synchronize()
    assert int(out[-1][1]) == status
    # the count's own verdict is unchanged: a fill afterwards succeeds, and so do the next rays
    again = through_the_engine(crate.engine, c._replace(max_t=1.0, origins=c.origins[:1], directions=c.directions[:1]))
    assert again[2].cpu().tolist() == [1, 0]


def test_a_point_outside_is_the_counts_flag(crate):
    c = K.cases()["dense"]
    far = c.points.copy()
    far[7, 1] = -(2.0 ** 32) * 2 * c.rho
    t, hit, counts = through_the_engine(crate.engine, c._replace(points=far))
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(t, hit, sentinel=U.SENTINEL)


def test_walls_alone_need_no_range(crate):
    """disc_radius = 0 walks nothing: a max_t beyond the cap is served, the origins are still tested."""
    c = K.cases()["cap_exceeded"]
    walls = np.array([[[5000.0, -1.0], [5000.0, 1.0]]])
    t, hit, counts = through_the_engine(crate.engine, c._replace(walls=walls, max_t=6000.0), rho=0.0)
    assert counts.cpu().tolist() == [1, 0] and t[:1].cpu().tolist() == [5000.0] and hit[:1].cpu().tolist() == [-2]
    t, hit, counts = through_the_engine(crate.engine, K.cases()["origin_outside"], rho=0.0)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(t, hit, sentinel=U.SENTINEL)


# ---- 4. the workspace is left as it is

def test_fill_rays_fill(crate):
    import torch
    c = K.cases()["dense"]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n, rays = len(c.points), len(c.origins)
    want = S.pairs(c.points, 2 * c.rho)
    k = len(want[1])
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    before, after = U.full(k, dev), U.full(k, dev)
    t, hit = U.full(rays, dev, dtype=torch.float64), U.full(rays, dev)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    eng.pairs_fill(before)
    eng.pairs_rays(t, hit, origins=o, directions=d, disc_radius=c.rho, max_t=c.max_t, segments=c.walls, counts=out)
    eng.pairs_rays(t, hit, origins=o, directions=d, disc_radius=c.rho / 2, max_t=c.max_t, counts=out)   # ... and again, smaller discs
    eng.pairs_rays(t, hit, origins=o, directions=d, disc_radius=c.rho, max_t=c.max_t, segments=c.walls, counts=out)
    eng.pairs_fill(after)
    eng.synchronize()
    assert torch.equal(before, after) and U.same_values_signs(after, want[1]) and k > 0
    assert U.same_values_signs(t, spec("dense")[0]) and U.same_values_signs(hit, spec("dense")[1]) and \
        out.cpu().tolist() == [rays, 0]


# ---- 5. errors

def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    c = K.cases()["dense"]
    n, rays = len(c.points), len(c.origins)
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    t, hit = U.full(rays, dev, dtype=torch.float64), U.full(rays, dev)
    walls = np.ascontiguousarray(c.walls)
    torch.cuda.synchronize()
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_rays_device
    args = lambda **kw: tuple({**dict(ctx=ctx, o=ptr(o), d=ptr(d), n=rays, rho=c.rho, max_t=c.max_t, seg=N.dptr(walls),  # noqa: E731
                                      ns=len(walls), t=ptr(t), hit=ptr(hit), room=rays, counts=ptr(out)), **kw}.values())
    assert fn(*args()) == N.ERR_STATE                                               # no count yet
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    for null in ("ctx", "o", "d", "t", "hit", "counts"):
        assert fn(*args(**{null: None})) == N.ERR_ARG, null
    assert fn(*args(n=-1)) == N.ERR_ARG and fn(*args(room=-1)) == N.ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert fn(*args(max_t=bad)) == N.ERR_ARG and fn(*args(rho=bad)) == N.ERR_ARG
    assert fn(*args(rho=np.nextafter(c.rho, 1.0))) == N.ERR_ARG                     # one ulp above half the count's radius
    assert fn(*args(seg=None)) == N.ERR_ARG                                         # segments announced, none given
    assert fn(*args(ns=-1)) == N.ERR_CAPACITY and fn(*args(ns=N.MAX_SEGMENTS + 1)) == N.ERR_CAPACITY
    assert fn(*args(o=N._P(o.data_ptr() + 8), n=rays - 1)) == N.ERR_ARG             # misaligned origins
    assert fn(*args(d=N._P(d.data_ptr() + 8), n=rays - 1)) == N.ERR_ARG             # ... and directions
    assert fn(*args(room=rays - 1)) == N.ERR_CAPACITY                               # too few rows
    assert fn(*args(n=(1 << 28) + 1, room=(1 << 28) + 1)) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    good = dict(origins=o, directions=d, disc_radius=c.rho, max_t=c.max_t, segments=walls, counts=out)
    for change in (dict(t=t[:-1]), dict(hit=hit.int()), dict(origins=o[:-1]), dict(directions=d.float()), dict(disc_radius=-1.0),
                   dict(max_t=float("inf")), dict(segments=np.zeros((17, 2, 2))), dict(segments=np.zeros((2, 2))), dict(room=rays + 1),
                   dict(counts=out[:1])):
        with pytest.raises(ValueError):
            eng.pairs_rays(change.pop("t", t), change.pop("hit", hit), **{**good, **change})
    # a batched grid is refused; inside a tick the call is refused
    ptr_b = torch.tensor([0, n // 2, n], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts, batch=ptr_b)
    assert fn(*args()) == N.ERR_ARG and b"batched" in lib.sc_last_error()
    eng.synchronize()
    assert U.untouched(t, hit, out, sentinel=U.SENTINEL)
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    assert fn(*args(seg=None, ns=0)) == 0                                           # no walls: fine
    assert fn(*args()) == 0
    eng.synchronize()
    assert U.same_values_signs(t, spec("dense")[0]) and U.same_values_signs(hit, spec("dense")[1]) and \
        out.cpu().tolist() == [rays, 0]
    eng.close()


def test_inside_a_tick(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc))
    for _ in range(3):
        crate.physics_tick()
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    o, d = U.tensor([[0.5, 0.5]]), U.tensor([[1.0, 0.0]])
    offsets, counts = U.full(eng.capacity + 1, dev), U.full(2, dev)
    t, hit = U.full(1, dev, dtype=torch.float64), U.full(1, dev)
    eng.pairs_count(None, radius=crate.diameter, offsets=offsets, counts=counts)
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_rays, t, hit, origins=o, directions=d, disc_radius=crate.diameter / 2, max_t=1.0,
                         counts=counts) == N.ERR_STATE
        assert b"inside a tick" in eng._lib.sc_last_error()
    finally:
        eng.step_finish()
    eng.synchronize()
    assert U.untouched(t, hit, sentinel=U.SENTINEL)


def test_wrapper_errors(crate):
    c = K.cases()["rays_65"]
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    for call in (lambda: crate.ray_tensors(o, d[:-1], 1.0, points=points), lambda: crate.ray_tensors(o.float(), d, 1.0, points=points),
                 lambda: crate.ray_tensors(o, d, -1.0, points=points), lambda: crate.ray_tensors(o, d, float("inf"), points=points),
                 lambda: crate.ray_tensors(o, d, 1.0, disc_radius=0.0, points=points),
                 lambda: crate.ray_tensors(o, d, 1.0, walls=np.zeros((17, 2, 2)), points=points),
                 lambda: crate.ray_tensors(o.cpu(), d.cpu(), 1.0, points=points)):
        with pytest.raises(ValueError):
            call()
