"""GPU tests of the device ray paths (sc_pairs_ray_paths_device, `Engine.pairs_ray_paths`, `Crate.ray_paths`): t, hit,
points, normals and end equal tests/ray_path_spec.py bit for bit -- every case of tests/ray_path_cases.py, through the
engine and through the crate, synchronising and not --; the state form after ticks; the same result twice and on a crate
of another capacity; bounces = 0 is `ray_tensors`; paths and rays leave each other's results alone; a status of leg 0
writes counts[1] and nothing else; the refusals."""
import functools

import numpy as np
import pytest

import gpu_support as U
import ray_cases as K
import ray_path_cases as PK
import ray_path_spec as PS
import ray_spec as RS
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def spec(name):
    return PS.paths(*PK.spec_args(PK.cases()[name]))


def same(got, want):
    """(t, hit, points, normals, end) against the spec's: NaN where the rule has NaN, every other element bit for bit."""
    return len(got) >= 5 and all((U.same_bits_or_nan if w.dtype == np.float64 else U.same_bits)(g, w) for g, w in zip(got, want))


def outputs(rows, legs, dev):
    import torch
    return (U.full((rows, legs), dev, dtype=torch.float64), U.full((rows, legs), dev), U.full((rows, legs, 2), dev, dtype=torch.float64),
            U.full((rows, legs, 2), dev, dtype=torch.float64), U.full(rows, dev))


def through_the_engine(eng, c, bounces, *, spare=8, particles=True, max_t=None):
    """count + paths through the engine into sentinel-filled tensors with `spare` rows of room beyond the rays ->
    (t, hit, points, normals, end, counts), synchronised.  The float tensors hold the integer sentinel too."""
    import torch
    dev = torch.device("cuda", eng.device)
    n, rays = len(c.points), len(c.origins)
    offsets, counts, got = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    out = outputs(rays + spare, bounces + 1, dev)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)                # (alive until the synchronisation)
    eng.pairs_count(p, radius=float(2 * c.rho), offsets=offsets, counts=counts)
    assert eng.pairs_ray_paths(*out, origins=o, directions=d, bounces=bounces, disc_radius=c.rho if particles else 0.0,
                               max_t=c.max_t if max_t is None else max_t, segments=c.walls, counts=got) is got
    eng.synchronize()
    return (*out, got)


# ---- 1. every case, through the engine and the crate, synchronising and not

@pytest.mark.parametrize("name", PK.names())
def test_case_equals_the_spec(crate, name):
    c = PK.cases()[name]
    want = spec(name)
    rays = len(c.origins)
    *got, counts = through_the_engine(crate.engine, c, c.bounces, particles=c.particles)
    assert counts.cpu().tolist() == [rays, 0]
    assert same([g[:rays] for g in got], want) and U.untouched(*(g[rays:] for g in got), sentinel=U.SENTINEL)
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    kw = dict(disc_radius=c.rho, walls=c.walls, particles=c.particles, points=points)
    got = crate.ray_paths(o, d, c.max_t, c.bounces, **kw)
    assert type(got).__name__ == "RayPaths" and got.t.is_cuda and same(got, want)
    again = crate.ray_paths(o, d, c.max_t, c.bounces, **kw)                          # the same result twice in a row
    assert same(again, want)
    out = crate.ray_paths(o, d, c.max_t, c.bounces, sync=False, **kw)
    crate.synchronize()
    assert len(out) == 6 and out[5].cpu().tolist() == [rays, 0] and same(out, want)


def test_leg_0_and_no_bounces_are_ray_tensors(crate):
    import torch
    for name in ("fuzz", "dead_rows", "no_bounces"):
        c = PK.cases()[name]
        points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
        kw = dict(disc_radius=c.rho, walls=c.walls, points=points)
        t, hit = crate.ray_tensors(o, d, c.max_t, **kw)
        want = RS.rays(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t)
        assert U.same_values_signs(t, want[0]) and U.same_values_signs(hit, want[1])
        flat = crate.ray_paths(o, d, c.max_t, 0, **kw)
        assert tuple(flat.t.shape) == (len(t), 1) and U.same_values_signs(flat.t[:, 0], want[0]) and torch.equal(flat.hit[:, 0], hit)
        paths = crate.ray_paths(o, d, c.max_t, c.bounces, **kw)
        assert U.same_values_signs(paths.t[:, 0].contiguous(), want[0]) and torch.equal(paths.hit[:, 0], hit)
        # ... and neither reader disturbs the other on the same grid: rays, paths, rays, paths
        t2, hit2 = crate.ray_tensors(o, d, c.max_t, **kw)
        assert U.same_values_signs(t2, want[0]) and torch.equal(hit2, hit) and same(crate.ray_paths(o, d, c.max_t, c.bounces, **kw), spec(name))


def test_rays_and_paths_on_one_count(crate):
    """One count, then paths, rays, paths through the engine: the workspace is left as it was."""
    import torch
    c = PK.cases()["fuzz"]
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n, rays, legs = len(c.points), len(c.origins), c.bounces + 1
    offsets, counts, got = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    first, second = outputs(rays, legs, dev), outputs(rays, legs, dev)
    t, hit = U.full(rays, dev, dtype=torch.float64), U.full(rays, dev)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    kw = dict(origins=o, directions=d, disc_radius=c.rho, max_t=c.max_t, segments=c.walls, counts=got)
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    eng.pairs_ray_paths(*first, bounces=c.bounces, **kw)
    eng.pairs_rays(t, hit, **kw)
    eng.pairs_ray_paths(*second, bounces=c.bounces, **kw)
    eng.synchronize()
    want = spec("fuzz")
    assert same(first, want) and same(second, want) and U.same_values_signs(t, want[0][:, 0].copy()) and torch.equal(hit, first[1][:, 0])


# ---- 2. the state form, and another capacity

def test_state_after_ticks(sc):
    import torch
    from sand_crate_amd import pairs
    crate = sc.Crate(U.scene(sc))
    for _ in range(40):
        crate.physics_tick()
    particles, = crate.state_tensors(pressure=False)[:1]
    host = particles.cpu().numpy()
    walls = crate.segments
    lo, hi = walls.reshape(-1, 2).min(axis=0), walls.reshape(-1, 2).max(axis=0)
    reach = 4 * float(np.hypot(*(hi - lo)))
    o, d = pairs.ray_fan((0.5, 0.5), 65, 0.0, 2 * np.pi, device=particles.device)
    torch.cuda.synchronize()
    got = crate.ray_paths(o, d, reach, 3)
    want = PS.paths(host, walls, o.cpu().numpy(), d.cpu().numpy(), crate.diameter / 2, reach, 3)
    assert len(host) > 100 and crate.particle_count == len(host) and same(got, want)
    assert int((got.end == 0).sum()) > 0 and int((got.hit >= 0).sum()) > 0 and int((got.hit <= -2).sum()) > 0
    assert pairs.path_legs(got.hit).cpu().tolist() == (want[1] != -1).sum(axis=1).tolist()
    arrows = pairs.path_arrows(o, got.points, got.hit)
    assert arrows.shape == (int((want[1] != -1).sum()), 2, 2) and np.isfinite(arrows).all()
    assert same(crate.ray_paths(o, d, reach, 3, points=particles), want)


def test_the_capacity_does_not_reach_the_result(sc):
    c = PK.cases()["fuzz"]
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    for capacity in (4200, 100_000):
        crate = sc.Crate(U.scene(sc), noise="none", capacity=capacity)
        assert same(crate.ray_paths(o, d, c.max_t, c.bounces, disc_radius=c.rho, walls=c.walls, points=points), spec("fuzz")), capacity


# ---- 3. the statuses of leg 0

@pytest.mark.parametrize("name", K.refused())
def test_a_status_of_leg_0_writes_counts_1_and_nothing_else(crate, name):
    c = K.cases()[name]
    status = c.claims["status"]
    *got, counts = through_the_engine(crate.engine, c, 2)
    assert counts.cpu().tolist() == [U.SENTINEL, status] and U.untouched(*got, sentinel=U.SENTINEL)
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    with pytest.raises(ValueError, match="max_t" if status == -4 else "domain"):
        crate.ray_paths(o, d, c.max_t, 2, disc_radius=c.rho, walls=c.walls, points=points)
    out = crate.ray_paths(o, d, c.max_t, 2, disc_radius=c.rho, walls=c.walls, points=points, sync=False)
    crate.synchronize()
    assert len(out) == 6 and int(out[-1][1]) == status
    again = through_the_engine(crate.engine, c._replace(origins=c.origins[:1], directions=c.directions[:1]), 2, max_t=1.0)
    assert again[-1].cpu().tolist() == [1, 0]


# ---- 4. the path that does not synchronise

def test_sync_false_does_not_synchronise(crate, monkeypatch):
    import torch
    c = PK.cases()["long_legs"]
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)

    def forbidden(*args, **kw):
        raise AssertionError("the call synchronised")

    with monkeypatch.context() as m:
        m.setattr(type(crate.engine), "synchronize", forbidden)
        m.setattr(torch.cuda, "synchronize", forbidden)
        m.setattr(torch.cuda.Stream, "synchronize", forbidden)
        m.setattr(torch.Tensor, "item", forbidden)
        m.setattr(torch.Tensor, "cpu", forbidden)
        out = crate.ray_paths(o, d, c.max_t, c.bounces, disc_radius=c.rho, walls=c.walls, points=points, sync=False)
    crate.synchronize()
    assert len(out) == 6 and out[5].cpu().tolist() == [len(c.origins), 0] and same(out, spec("long_legs"))


# ---- 5. errors

def test_argument_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    c = PK.cases()["long_legs"]
    n, rays, legs = len(c.points), len(c.origins), c.bounces + 1
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    p, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    offsets, counts, got = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    t, hit, at, normals, end = out = outputs(rays, legs, dev)
    walls = np.ascontiguousarray(c.walls)
    torch.cuda.synchronize()
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_ray_paths_device
    args = lambda **kw: tuple({**dict(ctx=ctx, o=ptr(o), d=ptr(d), n=rays, bounces=c.bounces, rho=c.rho, max_t=c.max_t,  # noqa: E731
                                      seg=N.dptr(walls), ns=len(walls), t=ptr(t), hit=ptr(hit), at=ptr(at), normals=ptr(normals),
                                      end=ptr(end), room=rays, counts=ptr(got)), **kw}.values())
    assert fn(*args()) == N.ERR_STATE                                               # no count yet
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    for null in ("ctx", "o", "d", "t", "hit", "at", "normals", "end", "counts"):
        assert fn(*args(**{null: None})) == N.ERR_ARG, null
    assert fn(*args(bounces=-1)) == N.ERR_ARG and fn(*args(bounces=16)) == N.ERR_ARG and b"bounces" in lib.sc_last_error()
    assert fn(*args(n=-1)) == N.ERR_ARG and fn(*args(room=-1)) == N.ERR_ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert fn(*args(max_t=bad)) == N.ERR_ARG and fn(*args(rho=bad)) == N.ERR_ARG
    assert fn(*args(rho=np.nextafter(c.rho, 1.0))) == N.ERR_ARG                     # one ulp above half the count's radius
    assert b"half the count's radius" in lib.sc_last_error()
    assert fn(*args(seg=None)) == N.ERR_ARG
    assert fn(*args(ns=-1)) == N.ERR_CAPACITY and fn(*args(ns=N.MAX_SEGMENTS + 1)) == N.ERR_CAPACITY
    for name, held in (("o", o), ("d", d), ("at", at), ("normals", normals)):       # misaligned
        assert fn(*args(**{name: N._P(held.data_ptr() + 8)}, n=rays - 1)) == N.ERR_ARG, name
    assert fn(*args(room=rays - 1)) == N.ERR_CAPACITY                               # too few rows
    good = dict(origins=o, directions=d, bounces=c.bounces, disc_radius=c.rho, max_t=c.max_t, segments=walls, counts=got)
    for change in (dict(t=t[:-1]), dict(t=t[:, :1]), dict(hit=hit.int()), dict(at=at[:, :, :1]), dict(normals=normals.float()),
                   dict(end=end[:-1]), dict(origins=o[:-1]), dict(directions=d.float()), dict(bounces=16), dict(bounces=0),
                   dict(max_t=float("inf")), dict(segments=np.zeros((17, 2, 2))), dict(room=rays + 1), dict(counts=got[:1])):
        with pytest.raises(ValueError):
            eng.pairs_ray_paths(change.pop("t", t), change.pop("hit", hit), change.pop("at", at), change.pop("normals", normals),
                                change.pop("end", end), **{**good, **change})
    # a batched grid is refused
    ptr_b = torch.tensor([0, n // 2, n], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts, batch=ptr_b)
    assert fn(*args()) == N.ERR_ARG and b"batched" in lib.sc_last_error()
    eng.synchronize()
    assert U.untouched(*out, got, sentinel=U.SENTINEL)                              # nothing above has launched anything
    eng.pairs_count(p, radius=2 * c.rho, offsets=offsets, counts=counts)
    assert fn(*args()) == 0
    eng.synchronize()
    assert same(out, PS.paths(*PK.spec_args(c))) and got.cpu().tolist() == [rays, 0]
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
    out = outputs(1, 2, dev)
    eng.pairs_count(None, radius=crate.diameter, offsets=offsets, counts=counts)
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(eng.pairs_ray_paths, *out, origins=o, directions=d, bounces=1, disc_radius=crate.diameter / 2, max_t=1.0,
                         counts=counts) == N.ERR_STATE
        assert b"inside a tick" in eng._lib.sc_last_error()
    finally:
        eng.step_finish()
    eng.synchronize()
    assert U.untouched(*out, sentinel=U.SENTINEL)


def test_wrapper_errors(crate):
    c = PK.cases()["ties_later"]
    points, o, d = U.tensor(c.points), U.tensor(c.origins), U.tensor(c.directions)
    for call in (lambda: crate.ray_paths(o, d[:-1], 1.0, points=points), lambda: crate.ray_paths(o.float(), d, 1.0, points=points),
                 lambda: crate.ray_paths(o, d, -1.0, points=points), lambda: crate.ray_paths(o, d, 1.0, 16, points=points),
                 lambda: crate.ray_paths(o, d, 1.0, -1, points=points), lambda: crate.ray_paths(o, d, 1.0, disc_radius=0.0, points=points),
                 lambda: crate.ray_paths(o, d, 1.0, walls=np.zeros((17, 2, 2)), points=points),
                 lambda: crate.ray_paths(o.cpu(), d.cpu(), 1.0, points=points)):
        with pytest.raises(ValueError):
            call()
