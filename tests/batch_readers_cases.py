"""The cases of the batched clusters, cluster sums, histograms, rays and ray paths (tests/batch_readers_spec.py is the
rule), of the kind of tests/batch_cases.py: a few hundred points at most, the clouds of a case overlapping in space, and
each built so that a kernel can go wrong in one named way.

Point cases (`cases()`: clusters, sums, histograms; `rays_of(name)` sends a few rays per cloud through them too):
  bridge               cloud A has two points 1.5 r apart, cloud B one point between them: unbatched one cluster, batched
                       A is two singletons;
  neighbours_in_index  rows ptr[b] - 1 and ptr[b] are closer than r: a union that tests only j < i joins the clouds;
  collisions           batch_cases' 16 clouds in every cell of one box: clouds share buckets under pairs_bucket;
  hist_blocks          sizes 0, 20, 0, 30, 14, 100, 5, 0 -- three clouds in the first workgroup of HIST_BLOCK = 64 rows,
                       a boundary exactly at row 64, a cloud over two workgroups, empty clouds first, in the middle and
                       last -- and queries of sizes 0, 3, 20, 41, 0, 80, 2, 0 with the same properties;
  dead_cloud           a cloud of non-finite points only between two ordinary ones: no cluster, a repeated cluster_ptr;
  long_chain           a chain of 70 members in the second cloud: its sum reaches the second level of the reduction, and
                       its members do not start at row 0.
Ray cases (`ray_cases()`):
  occluder             on the rays of cloud 1 a disc of cloud 0 lies nearer than cloud 1's: the batched hit is the
                       farther one, with its global index; the rays of cloud 2, which is empty, see only the wall;
  path_skip            a path of cloud 1 (ptr[1] = 2) hits its disc 2 and is mirrored onto its disc 0: the disc a leg
                       leaves out is a GLOBAL index -- compared as a cloud-local one it would leave out disc 0.
"""
import functools
from dataclasses import dataclass

import numpy as np

import batch_cases as BK
from batch_cases import RADIUS, _case, _cloud, _ptr

HIST_BLOCK = 64                      # sand_crate_amd/_native.py: HIST_BLOCK (test_batch_readers_cpu.py compares)
HIST_BINS = (1, 16, 17, 64)          # one bin, the last of the 16-bin kernel, the first of the 32-bin one, the most
RHO = 0.01                           # the disc radius of the ray cases: the count's radius is 2 * RHO


@dataclass(frozen=True)
class RayCase:
    points: np.ndarray
    ptr: np.ndarray
    origins: np.ndarray
    directions: np.ndarray
    ray_ptr: np.ndarray
    walls: np.ndarray
    rho: float
    max_t: float


def _ray_case(points, sizes, origins, directions, ray_sizes, walls, rho, max_t):
    arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in (points, origins, directions, walls)]
    points, origins, directions = (a.reshape(-1, 2) for a in arrays[:3])
    walls = arrays[3].reshape(-1, 2, 2)
    assert len(points) == sum(sizes) and len(origins) == len(directions) == sum(ray_sizes) and len(sizes) == len(ray_sizes)
    case = RayCase(points, _ptr(sizes), origins, directions, _ptr(ray_sizes), walls, float(rho), float(max_t))
    for a in (case.points, case.ptr, case.origins, case.directions, case.ray_ptr, case.walls):
        a.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def cases():
    rs = np.random.RandomState(4711)
    r = RADIUS
    out = {}
    out["bridge"] = _case([[0.1, 0.1], [0.1 + 1.5 * r, 0.1], [0.1 + 0.75 * r, 0.1]], [2, 1])
    sizes = [7, 9, 6, 8]
    pts = _cloud(rs, sum(sizes), 3)
    for at in np.cumsum(sizes)[:-1]:
        pts[at] = pts[at - 1] + [0.3 * r, 0.1 * r]
    out["neighbours_in_index"] = _case(pts, sizes)
    out["collisions"] = BK.cases()["collisions"]
    sizes, qsizes = [0, 20, 0, 30, 14, 100, 5, 0], [0, 3, 20, 41, 0, 80, 2, 0]
    out["hist_blocks"] = _case(_cloud(rs, sum(sizes), 3), sizes, _cloud(rs, sum(qsizes), 3), qsizes)
    dead = np.full((6, 2), np.nan)
    dead[1] = [np.inf, 0.01]
    dead[4] = [0.02, -np.inf]
    out["dead_cloud"] = _case(np.concatenate([_cloud(rs, 10, 2), dead, _cloud(rs, 10, 2)]), [10, 6, 10])
    chain = np.stack([0.01 + 0.8 * r * np.arange(70), np.full(70, 0.02)], axis=1)
    out["long_chain"] = _case(np.concatenate([chain[:10] + [0.2 * r, 0.3 * r], chain[rs.permutation(70)]]), [10, 70])
    return out


POINT_CASES = ("bridge", "neighbours_in_index", "collisions", "hist_blocks", "dead_cloud", "long_chain")
QUERY_CASES = ("hist_blocks",)


@functools.lru_cache(maxsize=None)
def rays_of(name, per_cloud=5):
    """A few rays per cloud through a point case, discs of radius r / 2 so that the count's radius is the case's: a
    RayCase with the case's points.  The origins lie in the points' box, a closed box of four walls lies round it."""
    case = cases()[name]
    rs = np.random.RandomState(len(case.points) + 17)
    finite = case.points[np.isfinite(case.points).all(axis=1)]
    lo, hi = finite.min(axis=0) - 2 * RADIUS, finite.max(axis=0) + 2 * RADIUS
    count = per_cloud * (len(case.ptr) - 1)
    origins = lo + rs.rand(count, 2) * (hi - lo)
    angles = rs.rand(count) * 2 * np.pi
    out = np.array([[-0.01, -0.01], [0.01, -0.01], [0.01, 0.01], [-0.01, 0.01]])
    corners = np.array([[lo[0], lo[1]], [hi[0], lo[1]], [hi[0], hi[1]], [lo[0], hi[1]]]) + out
    walls = np.stack([corners, np.roll(corners, -1, axis=0)], axis=1)
    return _ray_case(case.points, np.diff(case.ptr), origins, np.stack([np.cos(angles), np.sin(angles)], axis=1),
                     [per_cloud] * (len(case.ptr) - 1), walls, RADIUS / 2, 2.0 * float(np.linalg.norm(hi - lo)))


@functools.lru_cache(maxsize=None)
def ray_cases():
    out = {}
    wall = [[[0.5, -1.0], [0.5, 1.0]]]
    # cloud 0: three discs out of the way and the occluder at x = 0.1; cloud 1: the disc behind it at x = 0.2; cloud 2: empty
    points = [[0.9, 0.9], [0.9, 0.8], [0.8, 0.9], [0.10, 0.10], [0.20, 0.10]]
    origins = [[0.0, 0.1], [0.0, 0.1 + 0.5 * RHO], [0.0, 0.1], [0.0, 0.1 - 0.5 * RHO], [0.05, 0.1], [0.0, 0.1], [0.0, 0.3]]
    out["occluder"] = _ray_case(points, [4, 1, 0], origins, [[1.0, 0.0]] * 7, [2, 3, 2], wall, RHO, 1.0)
    # cloud 1, ptr[1] = 2: disc 2 (global 4) turns the ray that comes along y = 0.1 by a right angle, up onto disc 0 (global 2)
    s = RHO / np.sqrt(2.0)
    xp = 0.3
    points = [[0.9, 0.9], [0.9, 0.8], [xp, 0.2], [0.7, 0.7], [xp + s, 0.1 - s]]
    origins = [[0.0, 0.1], [0.0, 0.1], [0.0, 0.1 + 0.2 * RHO]]
    out["path_skip"] = _ray_case(points, [2, 3], origins, [[1.0, 0.0]] * 3, [1, 2], np.zeros((0, 2, 2)), RHO, 1.0)
    return out


RAY_CASES = ("occluder", "path_skip")
BOUNCES = (0, 1, 3)
