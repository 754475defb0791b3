"""CPU-side checks of the ray sensors: every case of tests/ray_cases.py has the property it is named for, by the rule of
tests/ray_spec.py; the walk the kernel makes (`ray_spec.walk`, csrc/sc_rays.h) finds the rule's answer on every case,
and the two wrong walks -- a 1 x 1 block, ending at the first step or batch of steps that met a disc -- get the cases
wrong that say so, and no other; the
rule against a second, slower formulation (distance from the centre to the reported point); the header, the ctypes table
and the null-context refusal of the new export; the tensor checks of `Engine.pairs_rays` on CPU tensors; and the
helpers of `sand_crate_amd.pairs` against NumPy.  No GPU."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import ray_cases as K
import ray_spec as RS
from sand_crate_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
SERVED, REFUSED = K.served(), K.refused()


@functools.lru_cache(maxsize=None)
def spec(name):
    c = K.cases()[name]
    return RS.rays(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t)


def grid(c):
    s = np.float64(2 * c.rho if c.radius is None else c.radius)
    return s, s * np.float64(N.PAIRS_CELL_FACTOR)


def terms(c, r, j):
    """a, b, cc, disc of the rule for ray r and point j."""
    o, d, p = c.origins[r], c.directions[r], c.points[j]
    fx, fy = o[0] - p[0], o[1] - p[1]
    a = d[0] * d[0] + d[1] * d[1]
    b = fx * d[0] + fy * d[1]
    cc = (fx * fx + fy * fy) - np.float64(c.rho) * np.float64(c.rho)
    return a, b, cc, b * b - a * cc


def candidate_t(c, r, kind, index):
    o, d = c.origins[r:r + 1], c.directions[r:r + 1]
    if kind == 0:
        return RS.wall_t(o, d, c.walls[index:index + 1], c.max_t)[0, 0]
    return RS.disc_t(o, d, c.points[index:index + 1], c.rho, c.max_t)[0, 0]


def same(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


# ---- the cases are what they say

def test_the_list_of_cases_covers_the_issue():
    names = set(K.cases())
    assert {f"grazed_{side}" for side in K.SIDES} <= names and len(K.SIDES) == 8
    assert {f"rays_{n}" for n in K.RAYS} <= names
    assert {N.RAY_BLOCK - 1, N.RAY_BLOCK, N.RAY_BLOCK + 1, 2 * N.RAY_BLOCK + 1, 0, 1} <= set(K.RAYS)
    for n in K.RAYS:
        assert len(K.cases()[f"rays_{n}"].origins) == n
    assert sorted(K.cases()[n].claims["status"] for n in REFUSED) == [N.PAIRS_RANGE, N.PAIRS_DOMAIN, N.PAIRS_DOMAIN]
    assert RS.MAX_STEPS == N.RAY_MAX_STEPS and RS.CELL_FACTOR == N.PAIRS_CELL_FACTOR
    assert K.cases()["small_rho"].rho * 20 < K.cases()["small_rho"].radius and K.cases()["dense"].radius is None
    assert all(len(c.points) <= 128 and len(c.walls) <= N.MAX_SEGMENTS for c in K.cases().values())   # a 256-bucket table


@pytest.mark.parametrize("name", sorted(K.cases()))
def test_status(name):
    c = K.cases()[name]
    assert RS.status(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.radius) == c.claims.get("status", 0)


CLAIMED = [(name, kind) for name, c in sorted(K.cases().items()) for kind in sorted(c.claims) if kind != "status"]


@pytest.mark.parametrize("name,kind", CLAIMED)
def test_claim(name, kind):
    c = K.cases()[name]
    claim = c.claims[kind]
    s, h = grid(c)
    if kind == "steps":
        for r, want in claim.items():
            assert RS.steps(c.origins[r], c.directions[r], c.walls, c.rho, c.max_t, c.radius) == want, r
        return
    if name in REFUSED:
        raise AssertionError("a refused case claims results")
    t, hit = spec(name)
    if kind == "hit":
        for r, want in claim.items():
            assert hit[r] == want, r
    elif kind == "t":
        for r, want in claim.items():
            assert t[r] == want or (np.isnan(want) and np.isnan(t[r])), r
            assert not (want == 0 and np.signbit(t[r])), r
    elif kind == "side":
        for r, want in claim.items():
            dt = s / np.sqrt(terms(c, r, hit[r])[0])
            k = int(np.floor(t[r] / dt))
            assert np.float64(k) * dt <= t[r] < np.float64(k + 1) * dt
            tm = np.float64(k + 0.5) * dt
            mid = c.origins[r] + tm * c.directions[r]
            centre = c.points[hit[r]]
            away = tuple(RS.cell_of(centre[i], h) - RS.cell_of(mid[i], h) for i in (0, 1))
            assert away == want and away != (0, 0), (r, away)
            # ... and the centre's cell is no cell the ray itself passes through, at any step
            passed = {(RS.cell_of(p[0], h), RS.cell_of(p[1], h))
                      for p in c.origins[r] + np.linspace(0, c.max_t, 4001)[:, None] * c.directions[r]}
            assert (RS.cell_of(centre[0], h), RS.cell_of(centre[1], h)) not in passed
    elif kind == "grazed":
        for r, (lo, hi) in claim.items():
            o, d, p = c.origins[r], c.directions[r], c.points[hit[r]]
            off = abs((p[0] - o[0]) * d[1] - (p[1] - o[1]) * d[0]) / np.hypot(*d)
            assert lo * c.rho <= off < hi * c.rho, (r, off)
    elif kind == "disc_sign":
        for (r, j), sign in claim.items():
            disc = terms(c, r, j)[3]
            assert (disc == 0.0 and sign == 0) or (disc < 0 and sign < 0) or (disc > 0 and sign > 0), (r, j, disc)
    elif kind == "rim":
        for r, j in claim:
            assert terms(c, r, j)[2] == 0.0, (r, j)
    elif kind == "tie":
        for r, first, second in claim:
            ta, tb = candidate_t(c, r, *first), candidate_t(c, r, *second)
            assert ta == tb == t[r] and np.isfinite(ta), (r, ta, tb)
            assert first < second and hit[r] == (first[1] if first[0] else -2 - first[1])
    elif kind == "block_1_fails":
        assert not same(RS.walk(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.radius, block=1), (t, hit))
    elif kind == "first_hit_fails":
        for batch in (1, N.RAY_WAVE_STEPS):
            wrong = RS.walk(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.radius, stop="first_hit", batch=batch)
            assert same(wrong, (t, hit)) == (batch not in claim), batch
    elif kind == "met_in_steps":
        dt = s / np.sqrt(terms(c, 0, 0)[0])
        for j, want in claim.items():
            cell = (RS.cell_of(c.points[j, 0], h), RS.cell_of(c.points[j, 1], h))
            first = next(k for k in range(64)
                         if all(abs(RS.cell_of(c.origins[0, i] + np.float64(k + 0.5) * dt * c.directions[0, i], h) - cell[i]) <= 1
                                for i in (0, 1)))
            assert first == want, (j, first)
        met = sorted(claim.values())                                         # either side of a border of the wave's batches
        assert met[0] % N.RAY_WAVE_STEPS == N.RAY_WAVE_STEPS - 1 and met[1] == met[0] + 1
        assert t[0] >= np.float64(met[1]) * dt                               # ... and the first batch may not end the walk
    elif kind == "shared_bucket":
        near, far = claim
        buckets = N.pairs_buckets(len(c.points))
        assert buckets == 256 and N.pairs_bucket(*near, buckets) == N.pairs_bucket(*far, buckets)
        cells = {(RS.cell_of(p[0], h), RS.cell_of(p[1], h)) for p in c.points}
        assert near in cells and far in cells and far[0] - near[0] > 10
        start = (RS.cell_of(c.origins[0, 0], h), RS.cell_of(c.origins[0, 1], h))
        assert max(abs(near[0] - start[0]), abs(near[1] - start[1])) <= 1       # in the block of step 0
        one, = [j for j, p in enumerate(c.points) if (RS.cell_of(p[0], h), RS.cell_of(p[1], h)) == far]
        assert np.isfinite(candidate_t(c, 0, 1, one)) and candidate_t(c, 0, 1, one) > t[0]   # on the ray, but not first
    elif kind == "negative_cells":
        assert any(RS.cell_of(p[0], h) < 0 and RS.cell_of(p[1], h) < 0 for p in c.points)
    else:
        raise AssertionError(f"unknown claim {kind}")


def test_the_tangent_cases_are_one_ulp_apart():
    at, outside, inside = (K.cases()[f"tangent_{n}"] for n in ("at", "outside", "inside"))
    assert inside.points[0, 1] < at.points[0, 1] < outside.points[0, 1]
    assert np.nextafter(at.points[0, 1], 1.0) == outside.points[0, 1] and np.nextafter(at.points[0, 1], 0.0) == inside.points[0, 1]
    assert [int(spec(f"tangent_{n}")[1][0]) for n in ("at", "outside", "inside")] == [0, -1, 0]
    assert spec("tangent_at")[0][0] == 0.25                              # cc / (-b + sqrt(0)) = 0.0625 / 0.25


def test_max_t_one_ulp():
    for thing in ("disc", "wall"):
        at, below = K.cases()[f"max_t_at_{thing}"], K.cases()[f"max_t_below_{thing}"]
        assert np.nextafter(at.max_t, 0.0) == below.max_t and spec(f"max_t_at_{thing}")[0][0] == at.max_t
        assert spec(f"max_t_below_{thing}")[1][0] == -1 and np.isinf(spec(f"max_t_below_{thing}")[0][0])


# ---- the walk

@pytest.mark.parametrize("batch", [1, N.RAY_WAVE_STEPS], ids=["a_step_at_a_time", "the_waves_batches"])
@pytest.mark.parametrize("name", SERVED)
def test_the_walk_finds_the_rules_answer(name, batch):
    c = K.cases()[name]
    assert same(RS.walk(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.radius, batch=batch), spec(name))


def test_the_wrong_walks_are_caught_by_the_cases_that_say_so():
    caught = {key: [n for n in SERVED if K.cases()[n].claims.get(key)] for key in ("block_1_fails", "first_hit_fails")}
    assert len(caught["block_1_fails"]) == 8 and caught["first_hit_fails"] == ["far_first_batch", "far_first_block"]
    # the kernel's own stopping rule, asked once per batch of the wave, has a case that tells its "first hit" twin
    assert N.RAY_WAVE_STEPS in K.cases()["far_first_batch"].claims["first_hit_fails"]
    for name in SERVED:                                                      # ... and no case is wrong without saying so
        c = K.cases()[name]
        for batch in (1, N.RAY_WAVE_STEPS):
            wrong = RS.walk(c.points, c.walls, c.origins, c.directions, c.rho, c.max_t, c.radius, stop="first_hit", batch=batch)
            assert same(wrong, spec(name)) == (batch not in c.claims.get("first_hit_fails", ())), (name, batch)


def test_the_walk_on_random_scenes():
    rs = np.random.RandomState(5)
    for scene in range(40):
        n, rays = rs.randint(0, 80), rs.randint(1, 12)
        pts = rs.rand(n, 2) * 4 - 2
        walls = K.BOX - 2.0 if scene % 2 else None
        angle = rs.rand(rays) * 2 * np.pi
        d = np.stack([np.cos(angle), np.sin(angle)], axis=1) * (0.2 + 3 * rs.rand(rays))[:, None]
        o = rs.rand(rays, 2) * 4 - 2
        rho, max_t = 0.05 + 0.2 * rs.rand(), 3 * rs.rand()
        radius = None if scene % 3 else 2 * rho * (1 + rs.rand())
        assert RS.status(pts, walls, o, d, rho, max_t, radius) == 0
        want = RS.rays(pts, walls, o, d, rho, max_t)
        assert same(RS.walk(pts, walls, o, d, rho, max_t, radius), want), scene
        assert same(RS.walk(pts, walls, o, d, rho, max_t, radius, batch=N.RAY_WAVE_STEPS), want), scene


# ---- the rule against geometry

@pytest.mark.parametrize("name", ["dense", "small_rho", "negative_cells", "rays_129", "cell_boundaries"])
def test_the_rule_against_the_geometry(name):
    """The reported point lies on the rim of the disc (or the origin inside it) or on the wall, within rounding, no
    disc is entered before it, and a ray that reports nothing passes every disc at more than rho or beyond max_t."""
    c = K.cases()[name]
    t, hit = spec(name)
    pts = c.points[np.isfinite(c.points).all(axis=1)]
    for r in np.nonzero(RS.live(c.origins, c.directions))[0]:
        o, d = c.origins[r], c.directions[r]
        reach = t[r] if np.isfinite(t[r]) else c.max_t
        if hit[r] >= 0:
            at = o + t[r] * d
            dist = np.hypot(*(at - c.points[hit[r]]))
            assert abs(dist - c.rho) < 1e-9 or (t[r] == 0 and dist <= c.rho)
        elif hit[r] <= -2:
            a, b = c.walls[-2 - hit[r]]
            at = o + t[r] * d
            assert abs((b - a)[0] * (at - a)[1] - (b - a)[1] * (at - a)[0]) / np.hypot(*(b - a)) < 1e-9
        along = o + np.linspace(0, reach * (1 - 1e-9), 2001)[:, None] * d      # nothing is entered before the reported point
        if len(pts) and t[r] != 0:                                                # (at t = 0 the origin may lie inside a disc)
            gap =np.hypot(along[:, None, 0] - pts[None, :, 0], along[:, None, 1] - pts[None, :, 1]).min()
            assert gap > c.rho - 1e-6, (r, gap)


# ---- the exports

def test_the_header_the_table_and_the_source_agree():
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.search(r"int sc_pairs_rays_device\s*\(([^)]*)\)", code)
    params = [" ".join(p.split()) for p in found.group(1).split(",")]
    assert params == ["sc_ctx* ctx", "const double* dev_origins", "const double* dev_directions", "int64_t n_rays",
                      "double disc_radius", "double max_t", "const double* segments", "int32_t n_segments", "double* dev_t",
                      "int64_t* dev_hit", "int64_t room_rows", "int64_t* dev_counts"]
    assert N.SIGNATURES["sc_pairs_rays_device"] == (C.c_int, [N._P, N._P, N._P, C.c_int64, C.c_double, C.c_double, N._D, C.c_int32,
                                                              N._P, N._P, C.c_int64, N._P])
    assert "#define SC_ABI_VERSION 5" in header and "#define SC_NUM_KERNELS 12" in header
    assert (N.PAIRS_RANGE, N.PAIRS_DOMAIN, N.RAY_NONE, N.RAY_WALL) == (-4, -1, -1, -2)
    source = (ROOT / "sand_crate_amd" / "csrc" / "sandcrate_hip.hip").read_text()
    assert source.index('#include "sc_hist.h"') < source.index('#include "sc_rays.h"') and source.count('#include "sc_rays.h"') == 1
    kernel = (ROOT / "sand_crate_amd" / "csrc" / "sc_rays.h").read_text()
    assert f"kRayMaxSteps = {N.RAY_MAX_STEPS};" in kernel and f"kRayBlock = {N.RAY_BLOCK};" in kernel
    assert f"kRayWaveSteps = {N.RAY_WAVE_STEPS};" in kernel and N.RAY_MAX_STEPS & (N.RAY_MAX_STEPS - 1) == 0
    assert "8192" in header and "sc_pairs_rays_device" in (ROOT / "sand_crate_amd" / "csrc" / "sc_host_state.h").read_text()


def test_a_null_context_is_refused():
    from sand_crate_amd import build
    lib = C.CDLL(str(build.build()))
    lib.sc_last_error.restype = C.c_char_p
    fn = lib.sc_pairs_rays_device
    fn.restype, fn.argtypes = N.SIGNATURES["sc_pairs_rays_device"]
    assert fn(*[kind() for kind in fn.argtypes]) == N.ERR_ARG and b"null context" in lib.sc_last_error()


def test_the_engine_checks_its_arguments_before_the_library_is_touched():
    import torch
    from sand_crate_amd.engine import Engine
    eng = Engine.__new__(Engine)                                          # (no context: nothing below may reach the library)
    eng.device = 0
    t, hit, xy, counts = torch.zeros(4, dtype=torch.float64), torch.zeros(4, dtype=torch.int64), torch.zeros((4, 2), dtype=torch.float64), \
        torch.zeros(2, dtype=torch.int64)
    good = dict(origins=xy, directions=xy, disc_radius=0.1, max_t=1.0, counts=counts)
    for change, text in ((dict(disc_radius=-0.1), "disc_radius"), (dict(disc_radius=float("nan")), "disc_radius"),
                         (dict(disc_radius=float("inf")), "disc_radius"), (dict(max_t=-1.0), "max_t"),
                         (dict(max_t=float("inf")), "max_t"), (dict(max_t=float("nan")), "max_t"),
                         (dict(segments=np.zeros((N.MAX_SEGMENTS + 1, 2, 2))), "segments"), (dict(segments=np.zeros((3, 2))), "segments"),
                         (dict(segments=np.zeros((3, 2, 3))), "segments"),
                         ({}, "t must be a contiguous CUDA float64"),            # the host's numbers pass: then the tensors
                         (dict(segments=np.zeros((N.MAX_SEGMENTS, 2, 2)), disc_radius=0.0, max_t=0.0), "t must be a contiguous CUDA")):
        with pytest.raises(ValueError, match=text):
            eng.pairs_rays(t, hit, **{**good, **change})


def test_the_messages_of_the_statuses():
    from sand_crate_amd import neighbourhood as H
    assert "ray_tensors" in H._QUERY_CALLS and set(H._STATUS) >= {N.PAIRS_RANGE, N.PAIRS_DOMAIN}
    assert H._STATUS[N.PAIRS_RANGE].format(who="ray_tensors", far="so far") == "ray_tensors: so far"
    assert "far" in H._Search.__init__.__kwdefaults__ and callable(H._Neighbourhood.ray_tensors)


# ---- the helpers

def test_ray_fan():
    from sand_crate_amd import pairs
    o, d = pairs.ray_fan((0.25, -1.5), 7, 0.5, 2.0)
    angles = 0.5 + np.arange(7) * (1.5 / 6)
    assert o.dtype == d.dtype and str(o.dtype) == "torch.float64" and tuple(o.shape) == tuple(d.shape) == (7, 2)
    assert np.array_equal(o.numpy(), np.tile([0.25, -1.5], (7, 1)))
    assert np.array_equal(d.numpy(), np.stack([np.cos(angles), np.sin(angles)], axis=1))
    assert np.allclose(np.hypot(*d.numpy().T), 1.0, rtol=1e-15)
    one = pairs.ray_fan((0, 0), 1, 0.0, 3.0)[1]
    assert one.tolist() == [[1.0, 0.0]] and tuple(pairs.ray_fan((0, 0), 0, 0.0, 1.0)[0].shape) == (0, 2)
    with pytest.raises(ValueError):
        pairs.ray_fan((0, 0), -1, 0.0, 1.0)


def test_ray_points_and_hits():
    import torch
    from sand_crate_amd import pairs
    c = K.cases()["not_finite"]
    t, hit = spec("not_finite")
    assert np.isnan(t).any() and np.isfinite(t).any() and (hit <= -2).any() and (hit >= 0).any()
    ends = pairs.ray_points(torch.from_numpy(c.origins.copy()), torch.from_numpy(c.directions.copy()), torch.from_numpy(t)).numpy()
    seen = np.isfinite(t)
    with np.errstate(all="ignore"):
        want = np.where(seen[:, None], c.origins + t[:, None] * c.directions, np.nan)
    assert np.array_equal(ends, want, equal_nan=True) and np.isnan(ends[~seen]).all()
    nothing = pairs.ray_points(torch.zeros((2, 2), dtype=torch.float64), torch.ones((2, 2), dtype=torch.float64),
                               torch.tensor([np.inf, 2.0], dtype=torch.float64)).numpy()
    assert np.isnan(nothing[0]).all() and nothing[1].tolist() == [2.0, 2.0]
    h = torch.from_numpy(hit)
    assert np.array_equal(pairs.hit_particles(h).numpy(), np.where(hit >= 0, hit, -1))
    assert np.array_equal(pairs.hit_walls(h).numpy(), np.where(hit <= -2, -2 - hit, -1))
    assert pairs.hit_walls(torch.tensor([-1, -2, -5, 7])).tolist() == [-1, 0, 3, -1]
    assert pairs.hit_particles(torch.tensor([-1, -2, -5, 7])).tolist() == [-1, -1, -1, 7]
