"""CPU-side checks of the batched neighbourhood calls: the rule's wrapper (tests/batch_spec.py) against a brute force that
knows nothing of clouds being cut out -- "same cloud and within the radius", over all rows at once --, what the cases
(tests/batch_cases.py) claim of themselves, and the binding.  No GPU."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import batch_cases as BK
import batch_spec as BS
import pairs_spec

ROOT = Path(__file__).resolve().parent.parent
ALL_CASES = BK.SELF_CASES + BK.QUERY_CASES


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the brute force: every row against every point, the cloud is one more condition

@functools.lru_cache(maxsize=None)
def brute(name, query_form):
    """-> (ok bool (R, n), d2 float64 (R, n), dx, dy): which points are partners of which rows, `half` off, a row of the
    self form not its own partner."""
    case = BK.cases()[name]
    p = case.points
    rows = case.queries if query_form else p
    row_cloud = BS.cloud_of(case.query_ptr if query_form else case.ptr, len(rows))
    point_cloud = BS.cloud_of(case.ptr, len(p))
    with np.errstate(invalid="ignore", over="ignore"):
        dx = rows[:, None, 0] - p[None, :, 0]
        dy = rows[:, None, 1] - p[None, :, 1]
        d2 = dx * dx + dy * dy
        r2 = np.float64(case.radius) * np.float64(case.radius)
        ok = (d2 <= r2) & (row_cloud[:, None] == point_cloud[None, :])
    ok &= np.isfinite(p).all(axis=1)[None, :] & np.isfinite(rows).all(axis=1)[:, None]
    if not query_form:
        ok &= ~np.eye(len(p), dtype=bool)
    return ok, d2, dx, dy


def forms(name):
    return (False, True) if name in BK.QUERY_CASES else (False,)


def args_of(name, query_form):
    case = BK.cases()[name]
    return dict(queries=case.queries, query_ptr=case.query_ptr) if query_form else {}


@pytest.mark.parametrize("name", ALL_CASES)
@pytest.mark.parametrize("half", [False, True])
def test_pairs_wrapper_is_the_brute_force(name, half):
    case = BK.cases()[name]
    ok, d2, _, _ = brute(name, False)
    if half:
        ok = ok & np.triu(np.ones_like(ok), 1)
    offsets, partners, dist = BS.pairs(case.points, case.radius, case.ptr, half)
    i, j = np.nonzero(ok)                                                            # (row-major: i ascending, then j)
    assert same(offsets, np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int64))
    assert same(partners, j.astype(np.int64)) and same(dist, d2[i, j])


@pytest.mark.parametrize("name", ALL_CASES)
@pytest.mark.parametrize("k", [1, 4, 64])
def test_nearest_wrapper_is_the_brute_force(name, k):
    case = BK.cases()[name]
    for query_form in forms(name):
        ok, d2, _, _ = brute(name, query_form)
        nb, dist, count = BS.nearest(case.points, case.radius, k, case.ptr, **args_of(name, query_form))
        assert same(count, ok.sum(axis=1).astype(np.int64)) and nb.shape == (len(ok), k)
        for r in range(len(ok)):
            js = np.nonzero(ok[r])[0]
            js = js[np.lexsort((js, d2[r, js]))][:k]                                # (ascending d2, then j)
            want_j = np.full(k, -1, dtype=np.int64)
            want_d = np.full(k, np.inf)
            want_j[:len(js)], want_d[:len(js)] = js, d2[r, js]
            assert same(nb[r], want_j) and same(dist[r], want_d), (name, r)


def weight(d2, r2, power):
    if power == 0:
        return np.float64(1.0)
    t = np.float64(1.0) - d2 / r2
    return t if power == 1 else t * t if power == 2 else (t * t) * t


@pytest.mark.parametrize("name", ALL_CASES)
@pytest.mark.parametrize("power,include_self", [(0, True), (2, False), (3, True)])
def test_field_wrapper_is_the_brute_force(name, power, include_self):
    case = BK.cases()[name]
    n = len(case.points)
    values = np.random.RandomState(5).rand(n, 3) - 0.5
    r2 = np.float64(case.radius) * np.float64(case.radius)
    for query_form in forms(name):
        ok, d2, _, _ = brute(name, query_form)
        if include_self and not query_form:
            ok = ok | (np.eye(n, dtype=bool) & np.isfinite(case.points).all(axis=1)[:, None])
        out, wsum = BS.field(case.points, case.radius, case.ptr, values, power, include_self, **args_of(name, query_form))
        assert out.shape == (len(ok), 3) and wsum.shape == (len(ok),)
        for r in range(len(ok)):
            acc, w_acc = np.zeros(3), np.float64(0.0)
            for j in np.nonzero(ok[r])[0]:                                          # (ascending j)
                w = weight(d2[r, j], r2, power)
                w_acc = w_acc + w
                acc = acc + w * values[j]
            assert same(out[r], acc) and same(wsum[r], w_acc), (name, r)


def brute_position(name, query_form, transposed, power, row_a, part_b, row_s, part_s):
    """The position rule over `ok` of the brute force -- or, `transposed`, with the points as the rows and the queries as
    the partners (the gradient with respect to the points of the query form)."""
    case = BK.cases()[name]
    ok, d2, dx, dy = brute(name, query_form)
    if transposed:
        ok, d2, dx, dy = ok.T, d2.T, -dx.T, -dy.T
    r2 = np.float64(case.radius) * np.float64(case.radius)
    out = np.zeros((len(ok), 2))
    scale = -(2.0 * power) / r2
    for r in range(len(ok)):
        ax = ay = np.float64(0.0)
        for j in np.nonzero(ok[r])[0]:
            s = np.float64(0.0)
            if row_s is not None:
                s = s + row_s[r]
            if part_s is not None:
                s = s + part_s[j]
            if row_a is not None:
                for c in range(row_a.shape[1]):
                    s = s + row_a[r, c] * part_b[j, c]
            t = np.float64(1.0) - d2[r, j] / r2
            sm = s if power == 1 else s * t if power == 2 else s * (t * t)
            ax, ay = ax + sm * dx[r, j], ay + sm * dy[r, j]
        out[r] = (scale * ax, scale * ay)
    return out


@pytest.mark.parametrize("name", ALL_CASES)
def test_gradient_wrappers_are_the_brute_force(name):
    """Power 2, two channels (one launch's worth: no chunks to add up), sums and weight sums both upstream."""
    case = BK.cases()[name]
    n, power = len(case.points), 2
    rs = np.random.RandomState(9)
    V = rs.rand(n, 2) - 0.5
    G, gw = rs.rand(n, 2) - 0.5, rs.rand(n) - 0.5
    ok = brute(name, False)[0] | (np.eye(n, dtype=bool) & np.isfinite(case.points).all(axis=1)[:, None])
    r2 = np.float64(case.radius) * np.float64(case.radius)
    want = np.zeros((n, 2))
    for j in range(n):                                                              # (the sum with the roles swapped)
        for r in np.nonzero(ok[:, j])[0]:
            want[j] = want[j] + weight(brute(name, False)[1][r, j], r2, power) * G[r]
    assert same(BS.values_grad(case.points, case.radius, case.ptr, G, power), want)
    got = BS.self_points_grad(case.points, case.radius, case.ptr, V, power, G, gw)
    assert same(got, brute_position(name, False, False, power, np.hstack([G, V]), np.hstack([V, G]), gw, gw))
    if name in BK.QUERY_CASES:
        q = len(case.queries)
        G, gw = rs.rand(q, 2) - 0.5, rs.rand(q) - 0.5
        kw = dict(queries=case.queries, query_ptr=case.query_ptr)
        got = BS.query_queries_grad(case.points, case.radius, case.ptr, V, power, G=G, gw=gw, **kw)
        assert same(got, brute_position(name, True, False, power, G, V, gw, None))
        got = BS.query_points_grad(case.points, case.radius, case.ptr, V, power, G=G, gw=gw, **kw)
        assert same(got, brute_position(name, True, True, power, V, G, None, gw))
        ok, d2 = brute(name, True)[:2]
        want = np.zeros((n, 2))
        for j in range(n):
            for r in np.nonzero(ok[:, j])[0]:
                want[j] = want[j] + weight(d2[r, j], r2, power) * G[r]
        assert same(BS.values_grad(case.points, case.radius, case.ptr, G, power, **kw), want)


# ---- what the cases claim

def test_triplets_differ_from_the_unbatched_result():
    """A kernel that ignores the offsets must fail: unbatched, every point has its two twins at d2 = 0."""
    case = BK.cases()["triplets"]
    batched = BS.pairs(case.points, case.radius, case.ptr)
    plain = pairs_spec.pairs(case.points, case.radius)
    assert int(plain[0][-1]) >= int(batched[0][-1]) + 2 * len(case.points)
    assert int((plain[2] == 0).sum()) == 2 * len(case.points) and int((batched[2] == 0).sum()) == 0
    for name in ("collisions", "boundaries", "queries"):                            # ... and so must it in the others
        case = BK.cases()[name]
        assert int(pairs_spec.pairs(case.points, case.radius)[0][-1]) > int(BS.pairs(case.points, case.radius, case.ptr)[0][-1])


def test_collisions_really_collide():
    """576 occupied (cell, cloud) keys, and in the table the count sizes for these 640 points two keys of DIFFERENT
    clouds share a bucket -- some of them even for the same cell's neighbourhood: the hash alone separates nothing."""
    from sand_crate_amd import _native as N
    case = BK.cases()["collisions"]
    n = len(case.points)
    buckets = N.pairs_buckets(n)
    assert buckets >= N.PAIRS_MIN_BUCKETS and buckets == 2048
    h = case.radius * N.PAIRS_CELL_FACTOR
    cells = np.floor(case.points / h).astype(np.int64)
    cloud = BS.cloud_of(case.ptr, n)
    keys = sorted({(int(cx), int(cy), int(b)) for (cx, cy), b in zip(cells, cloud)})
    assert len(keys) == 16 * BK.BOX * BK.BOX == 576
    by_bucket = {}
    for cx, cy, b in keys:
        by_bucket.setdefault(N.pairs_bucket(cx, cy, buckets, b), []).append((cx, cy, b))
    shared = [ks for ks in by_bucket.values() if len({b for _, _, b in ks}) > 1]
    assert len(shared) >= 10
    # cloud 0 hashes as an unbatched cell does
    assert all(N.pairs_bucket(cx, cy, buckets, 0) == N.pairs_bucket(cx, cy, buckets) for cx, cy, _ in keys)
    # a walk of cloud a over the nine cells around (cx, cy) meets members of cloud b in one of its buckets
    met = 0
    for cx, cy, a in keys:
        walk = {N.pairs_bucket(cx + ox, cy + oy, buckets, a) for ox in (-1, 0, 1) for oy in (-1, 0, 1)}
        met += any(b != a for bucket in walk for _, _, b in by_bucket.get(bucket, ()))
    assert met >= 100


def test_the_cases_hold_what_they_promise():
    cases = BK.cases()
    assert np.diff(cases["boundaries"].ptr).tolist() == [63, 64, 65, 1, 255, 257]
    assert np.diff(cases["empties"].ptr).tolist() == [0, 5, 0, 0, 1, 7, 1, 0]
    assert len(cases["single"].ptr) == 2 and len(cases["all_empty"].points) == 0 and len(cases["all_empty"].ptr) == 4
    assert int(BS.nearest(cases["boundaries"].points, BK.RADIUS, 64, cases["boundaries"].ptr)[2].max()) > 64
    odd = cases["nonfinite"]
    assert np.isnan(odd.points[30:60]).any() and np.isinf(odd.points[30:60]).any() and np.isfinite(odd.points[:30]).all()
    q = cases["queries"]
    psizes, qsizes = np.diff(q.ptr), np.diff(q.query_ptr)
    assert ((psizes == 0) & (qsizes > 0)).any() and ((psizes > 0) & (qsizes == 0)).any()
    assert {63, 64, 65} <= set(q.query_ptr.tolist())
    # queries of cloud 0 lie on points of cloud 3 -- and see none of them at d2 = 0 -- and on ten of their own
    on_other = (q.queries[:63, None, :] == q.points[None, q.ptr[3]:q.ptr[4], :]).all(axis=2).any(axis=1)
    assert int(on_other.sum()) == 40
    d2 = BS.nearest(q.points, q.radius, 1, q.ptr, q.queries, q.query_ptr)[1][:63, 0]
    assert int((d2 == 0).sum()) == 10 and not (d2[:40] == 0).any()
    assert int(BS.nearest(q.points, q.radius, 1, q.ptr, q.queries, q.query_ptr)[2][63]) == 0   # queries, no points
    for name in BK.SELF_CASES + BK.QUERY_CASES:
        assert len(cases[name].points) <= 720 and not cases[name].points.flags.writeable
    bad = BK.bad_offsets(q.ptr, len(q.points))
    assert set(bad) == {"first_is_1", "descent", "last_short", "last_long"}
    assert bad["first_is_1"][0] == 1 and (np.diff(bad["descent"]) < 0).any()
    assert bad["last_short"][-1] == len(q.points) - 1 and bad["last_long"][-1] == len(q.points) + 1


# ---- the binding

def test_header_exports_and_ctypes_name_the_setters():
    import ctypes as C
    from sand_crate_amd import _native as N, build
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sandcrate_hip.h").read_text(), flags=re.S)
    assert re.search(r"int sc_pairs_set_batch_device\(sc_ctx\* ctx, const int64_t\* dev_ptr, int64_t clouds\);", header)
    assert re.search(r"int sc_pairs_set_query_batch_device\(sc_ctx\* ctx, const int64_t\* dev_query_ptr\);", header)
    assert "#define SC_ABI_VERSION 5" in header
    assert N.SIGNATURES["sc_pairs_set_batch_device"] == (C.c_int, [N._P, N._P, C.c_int64])
    assert N.SIGNATURES["sc_pairs_set_query_batch_device"] == (C.c_int, [N._P, N._P])
    lib = C.CDLL(str(build.build()))
    assert hasattr(lib, "sc_pairs_set_batch_device") and hasattr(lib, "sc_pairs_set_query_batch_device")
    kernels = (ROOT / "sand_crate_amd" / "csrc" / "sc_pairs.h").read_text()
    assert int(re.search(r"kPairsHashCloud = (0x[0-9A-Fa-f]+)u", kernels).group(1), 16) == N.PAIRS_HASH_CLOUD
    assert re.search(r"kPairsStatusBatch = (-\d+)", kernels).group(1) == str(N.PAIRS_BATCH) == "-3"
    stub = (ROOT / "INTEGRATION.md").read_text()
    assert "sc_pairs_set_batch_device" in stub and "sc_pairs_set_query_batch_device" in stub
    for doc in ("README.md", "DESIGN.md"):
        assert "batch=" in (ROOT / doc).read_text()


def test_the_torch_helpers():
    import torch
    from sand_crate_amd import pairs
    ptr = pairs.batch_ptr([2, 0, 3])
    assert ptr.dtype == torch.int64 and ptr.tolist() == [0, 2, 2, 5]
    assert pairs.batch_index(ptr).tolist() == [0, 0, 2, 2, 2] and pairs.batch_index(ptr, 5).dtype == torch.int64
    assert pairs.batch_ptr(torch.tensor([4])).tolist() == [0, 4] and pairs.batch_index(pairs.batch_ptr([0, 0])).tolist() == []
    for name in BK.SELF_CASES:
        case = BK.cases()[name]
        ptr = pairs.batch_ptr(np.diff(case.ptr))
        assert ptr.tolist() == case.ptr.tolist()
        assert pairs.batch_index(ptr).tolist() == BS.cloud_of(case.ptr, len(case.points)).tolist()
    for bad in ([], [3, -1]):
        with pytest.raises(ValueError):
            pairs.batch_ptr(bad)
