"""CPU-side checks of the ray paths: every case of tests/ray_path_cases.py has the properties it claims, by the rule of
tests/ray_path_spec.py; every named mistake of the spec changes the cases that say they catch it, and no other; leg 0 is
`ray_spec.rays`, bits and all; the walk the kernel makes per leg (`ray_path_spec.walk_paths`) finds the brute force's
answer on every case; the rule against the same geometry in np.longdouble; the helpers of `sand_crate_amd.pairs`; the
header, the ctypes table and the null-context refusal of the new export; and the tensor checks of
`Engine.pairs_ray_paths` on CPU tensors.  No GPU."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import ray_cases as K
import ray_path_cases as PK
import ray_path_spec as PS
import ray_spec as RS
from sand_crate_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
NAMES = PK.names()
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def spec(name, wrong=None, walk=False):
    return (PS.walk_paths if walk else PS.paths)(*PK.spec_args(PK.cases()[name]), wrong=wrong)


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def candidate_t(c, result, r, k, kind, index):
    """t of a candidate of leg k of ray r: the leg's origin, direction and budget rebuilt from the legs before."""
    t, hit, P, n, _ = result
    d, m = c.directions[r], np.float64(c.max_t)
    for leg in range(k):
        d, m = PS.reflect(d, n[r, leg]), m - t[r, leg]
    o = P[r, k - 1] if k else c.origins[r]
    if kind == 0:
        return RS.wall_t(o[None], d[None], c.walls[index:index + 1], m)[0, 0]
    return PS.disc_t(o, d, c.points[index:index + 1], c.rho, m, k > 0)[0][0]


# ---- the cases are what they say

def test_the_list_of_cases_covers_the_issue():
    assert set(NAMES) >= {"mirror_box", "head_on", "ping_pong", "overlap_wedge", "inside_out", "inside_in", "centre", "grazing",
                          "long_legs", "leaves_domain", "past_cap", "leaves_domain_past_cap", "ties_later", "dead_rows", "no_rays",
                          "no_bounces", "fuzz"}
    cases = PK.cases()
    assert cases["mirror_box"].bounces == cases["ping_pong"].bounces == PS.MAX_BOUNCES == N.RAY_MAX_BOUNCES == 15
    assert not cases["mirror_box"].particles and len(cases["mirror_box"].points) == 0
    assert len(cases["no_rays"].origins) == 0 and cases["no_bounces"].bounces == 0
    assert len(cases["fuzz"].points) == 4096 and len(cases["fuzz"].origins) == 256 and cases["fuzz"].bounces == 8
    assert set(w for c in cases.values() for w in c.catches) == set(PS.WRONG)        # every mistake has a case
    assert (PS.ALL_HIT, PS.NOTHING, PS.DEAD) == (N.RAY_END_ALL_HIT, N.RAY_END_NOTHING, N.RAY_END_DEAD) and PS.WAVE_STEPS == N.RAY_WAVE_STEPS


@pytest.mark.parametrize("name", NAMES)
def test_leg_0_is_served_and_is_the_rays(name):
    c = PK.cases()[name]
    assert PK.status(c) == 0
    points, walls, origins, directions, rho, max_t, _, _ = PK.spec_args(c)
    want_t, want_hit = RS.rays(points, walls, origins, directions, rho, max_t)
    t, hit, P, n, end = spec(name)
    assert t[:, 0].tobytes() == want_t.tobytes() and np.array_equal(hit[:, 0], want_hit)
    assert t.shape == hit.shape == (len(origins), c.bounces + 1) and P.shape == n.shape == t.shape + (2,) and end.shape == t.shape[:1]
    if c.bounces == 0:
        whole = np.isfinite(n[:, 0]).all(axis=1)                                     # (an origin at a centre: 0 / 0)
        assert np.array_equal(end, np.where(np.isnan(t[:, 0]), 2, np.where(hit[:, 0] == -1, 1, np.where(whole, 0, 2))))


@pytest.mark.parametrize("name", NAMES)
def test_the_shape_of_a_path(name):
    """Written legs come first; what `end` says is what the last written leg shows; the rest is NaN, -1, NaN, NaN."""
    t, hit, P, n, end = spec(name)
    for r in range(len(t)):
        legs = int((hit[r] != -1).sum())
        assert (hit[r, :legs] != -1).all() and (hit[r, legs:] == -1).all() and np.isfinite(t[r, :legs]).all()
        assert np.isfinite(P[r, :legs]).all() and np.isnan(P[r, legs:]).all() and np.isnan(n[r, legs:]).all()
        if end[r] == PS.ALL_HIT:
            assert legs == t.shape[1] and np.isfinite(n[r]).all()
        elif end[r] == PS.NOTHING:
            assert t[r, legs] == np.inf and np.isnan(t[r, legs + 1:]).all()
        else:
            assert np.isnan(t[r, legs:]).all() and legs < t.shape[1] or not np.isfinite(n[r, legs - 1]).all()
        assert (t[r, :legs].sum() <= PK.cases()[name].max_t * (1 + 32 * U))          # the budget covers the whole path


CLAIMED = [(name, kind) for name in NAMES for kind in sorted(PK.cases()[name].claims)]


@pytest.mark.parametrize("name,kind", CLAIMED)
def test_claim(name, kind):
    c = PK.cases()[name]
    claim = c.claims[kind]
    result = t, hit, P, n, end = spec(name)
    s = np.float64(2 * c.rho)
    if kind == "hits":
        for r, want in claim.items():
            assert hit[r, :len(want)].tolist() == want and (hit[r, len(want):] == -1).all(), r
    elif kind == "end":
        for r, want in claim.items():
            assert end[r] == want, r
    elif kind == "t":
        for (r, k), want in claim.items():
            assert t[r, k] == want or (np.isnan(want) and np.isnan(t[r, k])), (r, k, t[r, k])
            assert not (want == 0 and np.signbit(t[r, k])), (r, k)
    elif kind == "t_sum":
        for r, want in claim.items():
            assert abs(t[r].sum() - want) <= 1e-12 * want, r
    elif kind in ("reversed", "kept", "reflected"):
        for r in claim:
            d = c.directions[r]
            after = PS.reflect(d, n[r, 0])
            if kind == "reversed":
                assert after[0] == -d[0] and after[1] == -d[1], (r, after)
            else:
                assert np.array_equal(after, d) == (kind == "kept"), (r, after)
    elif kind in ("inward", "outward"):
        found = PS.branches(c.points, c.origins, c.directions, c.rho, c.max_t, result)
        for r, k, j in claim:
            assert (j, kind == "inward") in found[(r, k)], (r, k, found)
            assert (hit[r, k] == j and t[r, k] == 0) == (kind == "inward")
    elif kind == "tie":
        for r, k, first, second in claim:
            ta, tb = candidate_t(c, result, r, k, *first), candidate_t(c, result, r, k, *second)
            assert ta == tb == t[r, k] and np.isfinite(ta), (r, k, ta, tb)
            assert first < second and hit[r, k] == (first[1] if first[0] else -2 - first[1])
    elif kind == "excluded":
        for (r, k), j in claim.items():
            assert k >= 1 and hit[r, k - 1] == j and hit[r, k] != j
            assert candidate_t(c, result, r, k, 1, j) == 0                           # ... by the rule, were j not left out
            wrong = spec(name, "no_exclusion")
            assert wrong[1][r, k] == j and wrong[0][r, k] == 0
    elif kind == "batch":
        for (r, k), want in claim.items():
            d = c.directions[r]
            for leg in range(k):
                d = PS.reflect(d, n[r, leg])
            dt = s / np.sqrt(d[0] * d[0] + d[1] * d[1])
            step = int(np.floor(t[r, k] / dt))
            assert k >= 1 and hit[r, k] >= 0 and np.float64(step) * dt <= t[r, k] < np.float64(step + 1) * dt
            assert step // N.RAY_WAVE_STEPS == want, (r, k, step)
    elif kind == "leg0_steps":
        for r, want in claim.items():
            assert RS.steps(c.origins[r], c.directions[r], c.walls, c.rho, c.max_t) >= want, r
    elif kind == "nan_normal":
        for r, k in claim:
            assert np.isnan(n[r, k]).all() and np.isfinite(P[r, k]).all() and np.isnan(t[r, k + 1:]).all()
    elif kind == "all_legs":
        assert (end == 0).all() and (hit != -1).all() and (hit[:, 1:] >= 0).any() and (hit[:, 1:] <= -2).any()
        assert (t[:, 1:] > 0).all()
    else:
        raise AssertionError(f"unknown claim {kind}")


def test_the_later_legs_that_fail_fail_alone_and_for_the_reason_named():
    """The ray whose second leg leaves the domain or walks past the cap ends with -1 or -4, the other ray of the call is
    served; with both failures the domain speaks first."""
    for name, domain, cap in (("leaves_domain", True, False), ("past_cap", False, True), ("leaves_domain_past_cap", True, True)):
        c = PK.cases()[name]
        t, hit, P, n, end = spec(name)
        o, d, m = P[0, 0], PS.reflect(c.directions[0], n[0, 0]), np.float64(c.max_t) - t[0, 0]
        s = np.float64(2 * c.rho)
        with np.errstate(all="ignore"):
            tip = o + m * d
            t_end = min(m, PS.nearest_wall(o, d, c.walls, m, -2 - hit[0, 0])[0])
            assert bool((~(np.abs(tip) / s < RS.DOMAIN)).any()) == domain and not (~(np.abs(o) / s < RS.DOMAIN)).any()
            assert bool(np.float64(RS.MAX_STEPS) * (s / np.sqrt(d[0] * d[0] + d[1] * d[1])) <= t_end) == cap
        assert end.tolist() == [RS.OUTSIDE if domain else RS.RANGE, 0]
    c = PK.cases()["leaves_domain_past_cap"]
    walls_only = PS.paths(None, c.walls, c.origins, c.directions, 0.0, c.max_t, c.bounces, 2 * c.rho)
    assert walls_only[4].tolist() == [1, 0]                                           # no discs looked for: neither test


# ---- the mistakes, and the walk

@pytest.mark.parametrize("name", NAMES)
def test_every_mistake_changes_the_cases_that_say_so_and_no_other(name):
    c = PK.cases()[name]
    caught = tuple(sorted(w for w in PS.WRONG if not same(spec(name, w, w == "walk_not_restarted"), spec(name))))
    assert caught == c.catches


@pytest.mark.parametrize("batch", [1, N.RAY_WAVE_STEPS], ids=["a_step_at_a_time", "the_waves_batches"])
@pytest.mark.parametrize("name", NAMES)
def test_the_walk_finds_the_rules_answer(name, batch):
    assert same(PS.walk_paths(*PK.spec_args(PK.cases()[name]), batch=batch), spec(name))


# ---- the rule against geometry

@pytest.mark.parametrize("name", ["fuzz", "dead_rows", "overlap_wedge", "long_legs", "mirror_box"])
def test_the_rule_against_the_geometry_in_longdouble(name):
    """With u = 2^-53, f = o - c of the leg and every norm evaluated in np.longdouble:
      * a disc hit at t > 0 lies on the rim: the exact point o + t d at the computed t has | |P* - c|^2 - rho^2 | <=
        18 u |f|^2 (csrc/sc_rays.h, "the claim"), so | |P* - c| - rho | <= 18 u |f|^2 / rho; the written P is one product
        and one sum per axis away, 2 u (|o| + t |d|) each, 3 u (|o| + t |d|) in length: the sum is below
        32 u (|f|^2 / rho + |o| + t |d|);
      * the normal is unit: two products and a sum (2u on the square, u on the root), the root (u), a quotient (u):
        | |n| - 1 | <= 3u to first order, 4u with the second;
      * the next direction keeps |d| and mirrors the angle: d' = d - 2 dn n.  An error of dn cancels in |d'|^2 to first
        order; |n|^2 - 1 (8u) enters as 4 dn^2 (|n|^2 - 1), 16 u |d| in length at most; the product and the difference
        per axis add 3 u |d| each.  Both | |d'| - |d| | and | d'.n + d.n | stay below 32 u |d|."""
    c = PK.cases()[name]
    t, hit, P, n, end = spec(name)
    L = np.longdouble
    norm = lambda v: np.sqrt(L(v[0]) * L(v[0]) + L(v[1]) * L(v[1]))  # noqa: E731
    checked = 0
    for r in range(len(t)):
        o, d = c.origins[r], c.directions[r]
        for k in range(t.shape[1]):
            if hit[r, k] == -1 or not np.isfinite(n[r, k]).all():
                break
            if hit[r, k] >= 0 and t[r, k] > 0:
                centre = c.points[hit[r, k]]
                f2 = norm(o - centre) ** 2
                assert abs(norm(P[r, k] - centre) - L(c.rho)) <= 32 * U * (f2 / c.rho + norm(o) + t[r, k] * norm(d)), (r, k)
            assert abs(norm(n[r, k]) - 1) <= 4 * U, (r, k)
            after = PS.reflect(d, n[r, k])
            dot = lambda a, b: L(a[0]) * L(b[0]) + L(a[1]) * L(b[1])  # noqa: E731
            assert abs(norm(after) - norm(d)) <= 32 * U * norm(d), (r, k)
            if dot(d, n[r, k]) < 0:
                assert abs(dot(after, n[r, k]) + dot(d, n[r, k])) <= 32 * U * norm(d), (r, k)
            o, d = P[r, k], after
            checked += 1
    assert checked > 2


# ---- the helpers

def test_path_legs_and_path_arrows():
    import torch
    from sand_crate_amd import pairs
    hit = torch.tensor([[3, -2, 5], [-4, -1, -1], [-1, -1, -1]])
    assert pairs.path_legs(hit).tolist() == [3, 1, 0]
    nan = float("nan")
    origins = torch.tensor([[0.0, 0.0], [1.0, 1.0], [2.0, 2.0]], dtype=torch.float64)
    points = torch.tensor([[[1.0, 0.0], [1.0, 2.0], [0.5, 2.0]], [[1.0, 4.0], [nan, nan], [nan, nan]], [[nan, nan]] * 3], dtype=torch.float64)
    arrows = pairs.path_arrows(origins, points, hit)
    assert arrows.dtype == np.float64 and arrows.tolist() == [[[0.0, 0.0], [1.0, 0.0]], [[1.0, 0.0], [0.0, 2.0]], [[1.0, 2.0], [-0.5, 0.0]],
                                                              [[1.0, 1.0], [0.0, 3.0]]]
    assert pairs.path_arrows(origins[:0], points[:0], hit[:0]).shape == (0, 2, 2)
    t, hit_, P, n, end = spec("mirror_box")
    c = PK.cases()["mirror_box"]
    arrows = pairs.path_arrows(torch.from_numpy(c.origins.copy()), torch.from_numpy(P), torch.from_numpy(hit_))
    assert arrows.shape == (16, 2, 2) and np.array_equal(arrows[1:, 0], P[0, :-1]) and np.array_equal(arrows[0, 0], c.origins[0])
    from sand_crate_amd.addons import arrow_ends
    assert len(arrow_ends(arrows)) == 16                                               # the form render(arrows=...) draws
    assert pairs.RayPaths._fields == ("t", "hit", "points", "normals", "end")


# ---- the exports

def test_the_header_the_table_and_the_source_agree():
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    found = re.search(r"int sc_pairs_ray_paths_device\s*\(([^)]*)\)", code)
    params = [" ".join(p.split()) for p in found.group(1).split(",")]
    assert params == ["sc_ctx* ctx", "const double* dev_origins", "const double* dev_directions", "int64_t n_rays", "int32_t bounces",
                      "double disc_radius", "double max_t", "const double* segments", "int32_t n_segments", "double* dev_t",
                      "int64_t* dev_hit", "double* dev_points", "double* dev_normals", "int64_t* dev_end", "int64_t room_rows",
                      "int64_t* dev_counts"]
    assert N.SIGNATURES["sc_pairs_ray_paths_device"] == (C.c_int, [N._P, N._P, N._P, C.c_int64, C.c_int32, C.c_double, C.c_double, N._D,
                                                                   C.c_int32, N._P, N._P, N._P, N._P, N._P, C.c_int64, N._P])
    assert "#define SC_ABI_VERSION 5" in header and "#define SC_NUM_KERNELS 12" in header
    assert f"#define SC_RAY_MAX_BOUNCES {N.RAY_MAX_BOUNCES}\n" in header
    kernel = (ROOT / "sand_crate_amd" / "csrc" / "sc_rays.h").read_text()
    assert f"kRayMaxLegs = {N.RAY_MAX_BOUNCES + 1};" in kernel and "k_ray_paths" in kernel
    assert "sc_pairs_ray_paths_device" in (ROOT / "sand_crate_amd" / "csrc" / "sc_host_state.h").read_text()


def test_a_null_context_is_refused():
    from sand_crate_amd import build
    lib = C.CDLL(str(build.build()))
    lib.sc_last_error.restype = C.c_char_p
    fn = lib.sc_pairs_ray_paths_device
    fn.restype, fn.argtypes = N.SIGNATURES["sc_pairs_ray_paths_device"]
    assert fn(*[kind() for kind in fn.argtypes]) == N.ERR_ARG and b"null context" in lib.sc_last_error()


def test_the_engine_checks_its_arguments_before_the_library_is_touched():
    """What can be reached without a GPU: `bounces`, the host's numbers, and the refusal of a tensor that is not on the
    device.  That check comes first for every tensor, so a wrong dtype, shape or room of a CUDA tensor is refused in
    tests/test_gpu_ray_paths.py (`test_argument_and_capacity_errors`), not here."""
    import torch
    from sand_crate_amd.engine import Engine
    eng = Engine.__new__(Engine)                                          # (no context: nothing below may reach the library)
    eng.device = 0
    t, hit = torch.zeros((4, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.int64)
    at, xy, end, counts = torch.zeros((4, 2, 2), dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64), \
        torch.zeros(4, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    good = dict(origins=xy, directions=xy, bounces=1, disc_radius=0.1, max_t=1.0, counts=counts)
    for change, text in ((dict(bounces=16), "bounces"), (dict(bounces=-1), "bounces"), (dict(disc_radius=-0.1), "disc_radius"),
                         (dict(max_t=float("inf")), "max_t"), (dict(segments=np.zeros((N.MAX_SEGMENTS + 1, 2, 2))), "segments"),
                         ({}, "t must be a contiguous CUDA float64"),          # the host's numbers pass: then the tensors
                         (dict(bounces=15), "t must be a contiguous CUDA float64")):
        with pytest.raises(ValueError, match=text):
            eng.pairs_ray_paths(t, hit, at, at, end, **{**good, **change})


def test_the_messages_of_the_statuses():
    from sand_crate_amd import neighbourhood as H
    assert "ray_paths" in H._QUERY_CALLS and H._OF_EITHER["ray_paths"] == H._OF_EITHER["ray_tensors"]
    assert callable(H._Neighbourhood.ray_paths) and K.RHO == PK.RHO
