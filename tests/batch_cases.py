"""The cases of the batched neighbourhood calls (tests/batch_spec.py is the rule): small -- a few hundred points -- and
built so that a kernel can still go wrong.  All clouds of a case lie in the same small box and overlap completely, as the
frames of one scene do: only the index range keeps them apart.

  triplets    the same 40-point cloud three times, identical coordinates: without the index test every point pairs with
              its twins at d2 = 0;
  collisions  16 clouds of 40 points in one box of 6 x 6 cells, every cloud in every cell: 576 occupied (cell, cloud) keys
              in a table of 2048 buckets -- clouds collide in buckets (test_batch_cpu.py proves it from the hash), so the
              hash alone cannot separate them;
  empties     empty clouds first, in the middle and last, clouds of one point;
  single      B = 1;
  all_empty   every cloud empty, n = 0;
  boundaries  cloud sizes 63, 64, 65, 1, 255, 257: boundaries inside and on the edges of a wave and of a 256-row workgroup;
              the cloud of 255 is crowded into 2 x 2 cells, so that rows have more than 64 partners;
  nonfinite   a cloud holding NaN and infinite points between two ordinary ones;
  queries     the query form: a cloud with queries and no points, a cloud with points and no queries, queries that lie
              exactly on points of ANOTHER cloud (and some on points of their own), query cloud boundaries at 63, 64, 65.
`bad_offsets(n)` lists offsets that are out of order for n rows: first entry 1, a descent, last entry n - 1 and n + 1.
"""
import functools
from dataclasses import dataclass

import numpy as np

RADIUS = 0.05
CELL = RADIUS * (1.0 + 2.0 ** -20)   # the search's cell (csrc/sc_pairs.h)
BOX = 6                              # cells per side


@dataclass(frozen=True)
class Case:
    points: np.ndarray
    ptr: np.ndarray
    radius: float = RADIUS
    queries: np.ndarray = None
    query_ptr: np.ndarray = None


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def _cloud(rs, n, cells=BOX):
    return rs.rand(n, 2) * (cells * CELL * 0.999)


def _frozen(case):
    for a in (case.points, case.ptr, case.queries, case.query_ptr):
        if a is not None:
            a.setflags(write=False)
    return case


def _case(points, sizes, queries=None, query_sizes=None):
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 2)
    assert len(points) == int(np.sum(sizes))
    if queries is None:
        return _frozen(Case(points, _ptr(sizes)))
    queries = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 2)
    assert len(queries) == int(np.sum(query_sizes)) and len(query_sizes) == len(sizes)
    return _frozen(Case(points, _ptr(sizes), RADIUS, queries, _ptr(query_sizes)))


@functools.lru_cache(maxsize=None)
def cases():
    rs = np.random.RandomState(20250)
    out = {}
    one = _cloud(rs, 40)
    out["triplets"] = _case(np.concatenate([one, one, one]), [40, 40, 40])
    # every cloud has a point in each of the 36 cells, and four more anywhere
    centres = (np.stack(np.meshgrid(np.arange(BOX), np.arange(BOX)), -1).reshape(-1, 2) + 0.5) * CELL
    crowd = []
    for _ in range(16):
        cloud = np.concatenate([centres + (rs.rand(36, 2) - 0.5) * 0.9 * CELL, _cloud(rs, 4)])
        crowd.append(cloud[rs.permutation(40)])
    out["collisions"] = _case(np.concatenate(crowd), [40] * 16)
    sizes = [0, 5, 0, 0, 1, 7, 1, 0]
    out["empties"] = _case(_cloud(rs, sum(sizes), 2), sizes)
    out["single"] = _case(_cloud(rs, 50, 3), [50])
    out["all_empty"] = _case(np.zeros((0, 2)), [0, 0, 0])
    sizes = [63, 64, 65, 1, 255, 257]
    out["boundaries"] = _case(np.concatenate([_cloud(rs, s, 2 if s == 255 else BOX) for s in sizes]), sizes)
    odd = _cloud(rs, 30, 3)
    odd[[2, 11]] = np.nan
    odd[5, 0] = np.inf
    odd[17, 1] = -np.inf
    odd[23] = [np.nan, np.inf]
    out["nonfinite"] = _case(np.concatenate([_cloud(rs, 30, 3), odd, _cloud(rs, 30, 3)]), [30, 30, 30])
    # points: clouds 0 .. 4 of 40, 0, 40, 50, 30; queries: 63, 1, 0, 1, 65 -- boundaries at 63, 64, 64, 65, 130
    psizes, qsizes = [40, 0, 40, 50, 30], [63, 1, 0, 1, 65]
    pts = [_cloud(rs, s, 3) for s in psizes]
    q0 = np.concatenate([pts[3][:40], pts[0][:10], _cloud(rs, 13, 3)])   # on points of cloud 3, on its own, anywhere
    q4 = np.concatenate([pts[0][:20], pts[4][:5], _cloud(rs, 40, 3)])     # on points of cloud 0, on its own, anywhere
    out["queries"] = _case(np.concatenate(pts), psizes, np.concatenate([q0, pts[0][:1], pts[2][:1], q4]), qsizes)
    return out


SELF_CASES = ("triplets", "collisions", "empties", "single", "all_empty", "boundaries", "nonfinite")
QUERY_CASES = ("queries",)


def bad_offsets(ptr, n):
    """`ptr` -- good offsets of at least two clouds for n >= 2 rows -- spoilt in the four ways: name -> int64 array."""
    ptr = np.asarray(ptr, dtype=np.int64)
    assert len(ptr) >= 3 and ptr[0] == 0 and ptr[-1] == n >= 2
    out = {}
    for name, at, value in (("first_is_1", 0, 1), ("last_short", -1, n - 1), ("last_long", -1, n + 1)):
        bad = ptr.copy()
        bad[at] = value
        out[name] = bad
    bad = ptr.copy()
    bad[1] = ptr[2] + 1                         # entry 2 lies below entry 1; the ends are as they should be
    assert bad[0] == 0 and bad[-1] == n and bad[2] < bad[1]
    out["descent"] = bad
    return out
