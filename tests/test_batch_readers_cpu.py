"""CPU-side checks of the batched clusters, cluster sums, histograms, rays and ray paths: the binding, and that the cases
(tests/batch_readers_cases.py) hold what they promise -- for each, the per-cloud rule (tests/batch_readers_spec.py)
differs from the unbatched rule on the concatenated points and from the wrong twin it is named for.  Without that a
kernel that ignores the clouds could pass the GPU tests.  No GPU."""
import functools
import re
from pathlib import Path

import numpy as np

import batch_readers_cases as RK
import batch_readers_spec as RS
import batch_spec as BS
import cluster_spec
import cluster_sums_spec
import hist_spec
import pairs_spec
import ray_path_spec
import ray_spec

ROOT = Path(__file__).resolve().parent.parent
NEW_CALLS = ("sc_pairs_label_batch_device", "sc_pairs_hist_batch_device", "sc_pairs_rays_batch_device",
             "sc_pairs_ray_paths_batch_device")
EDGES = np.linspace(0.0, RK.RADIUS, 9)


@functools.lru_cache(maxsize=None)
def clusters_of(name):
    case = RK.cases()[name]
    return RS.clusters(case.points, case.radius, case.ptr), cluster_spec.clusters(case.points, case.radius)


# ---- the binding

def test_header_exports_and_ctypes_name_the_four_calls():
    import ctypes as C
    from sand_crate_amd import _native as N, build
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sandcrate_hip.h").read_text(), flags=re.S)
    lib = C.CDLL(str(build.build()))
    for name in NEW_CALLS:
        assert re.search(r"\bint " + name + r"\(sc_ctx\* ctx,", header), name
        assert name in N.SIGNATURES and N.SIGNATURES[name][0] is C.c_int, name
        assert hasattr(lib, name), name
        assert name in (ROOT / "INTEGRATION.md").read_text(), name
    # each takes its twin's arguments: the label's plus cluster_ptr, the histogram's plus room_clouds
    twin = lambda name: N.SIGNATURES[name.replace("_batch", "")][1]  # noqa: E731
    assert N.SIGNATURES[NEW_CALLS[0]][1] == twin(NEW_CALLS[0])[:-1] + [N._P] + twin(NEW_CALLS[0])[-1:]
    assert N.SIGNATURES[NEW_CALLS[1]][1] == twin(NEW_CALLS[1])[:-1] + [C.c_int64] + twin(NEW_CALLS[1])[-1:]
    assert N.SIGNATURES[NEW_CALLS[2]][1] == twin(NEW_CALLS[2]) and N.SIGNATURES[NEW_CALLS[3]][1] == twin(NEW_CALLS[3])
    assert "#define SC_ABI_VERSION 5" in header and lib.sc_abi_version() == 5
    assert int(eval(re.search(r"SC_HIST_BATCH_MAX_CELLS = ([^}]+?) }", header).group(1))) == N.HIST_BATCH_MAX_CELLS
    assert RK.HIST_BLOCK == N.HIST_BLOCK and set(N.HIST_SLOTS) <= set(RK.HIST_BINS) | {32}
    assert [N.hist_slots(b) for b in RK.HIST_BINS] == [16, 16, 32, 64]               # every NB step is met
    host = (ROOT / "sand_crate_amd" / "csrc" / "sc_host_state.h").read_text()
    for name in NEW_CALLS:                                                           # one body per pair: a wrapper each
        assert len(re.findall(r"^int " + name + r"\(", host, flags=re.M)) == 1


def test_the_torch_helpers():
    import torch
    from sand_crate_amd import pairs
    assert pairs.cluster_cloud(torch.tensor([0, 2, 2, 5])).tolist() == [0, 0, 2, 2, 2]
    assert pairs.cluster_cloud(torch.tensor([0, 0]), 0).tolist() == []
    edges = [0.0, 0.1, 0.2]
    total = torch.tensor([[4, 6], [0, 0], [2, 12]])
    g = pairs.radial_distribution(total, edges, [4, 0, 3], 2.0)
    assert g.shape == (3, 2) and bool(torch.isnan(g[1]).all())
    for b, n in ((0, 4), (2, 3)):
        assert torch.equal(g[b], pairs.radial_distribution(total[b], edges, n, 2.0))


# ---- every case separates the rule from the unbatched rule

def test_every_point_case_differs_from_the_unbatched_rule():
    for name in RK.POINT_CASES:
        case = RK.cases()[name]
        (labels, sizes, roots, cptr), (plain_labels, plain_sizes, _) = clusters_of(name)
        assert len(sizes) != len(plain_sizes) and not np.array_equal(labels, plain_labels), name
        assert cptr[0] == 0 and cptr[-1] == len(sizes) and (np.diff(cptr) >= 0).all()
        assert np.array_equal(BS.cloud_of(cptr, len(sizes)), BS.cloud_of(case.ptr, len(case.points))[roots]), name
        table, total = RS.histogram(case.points, EDGES, case.ptr)
        plain_table, plain_total = hist_spec.histogram(case.points, EDGES)
        assert total.shape == (len(case.ptr) - 1, len(EDGES) - 1) and not np.array_equal(table, plain_table), name
        assert int(total.sum()) < int(plain_total.sum()), name
        values = np.arange(len(case.points), dtype=np.float64).reshape(-1, 1)
        sums = RS.cluster_sums(case.points, case.radius, case.ptr, values, extrema=False)[3]
        plain_sums = cluster_sums_spec.cluster_sums(plain_labels, values, len(plain_sizes), False)[0]
        assert sums.shape != plain_sums.shape or not np.array_equal(sums, plain_sums), name
        assert len(case.points) <= 720 and not case.points.flags.writeable
    for name in RK.QUERY_CASES:
        case = RK.cases()[name]
        table = RS.histogram(case.points, EDGES, case.ptr, case.queries, case.query_ptr)[0]
        assert not np.array_equal(table, hist_spec.histogram(case.points, EDGES, case.queries)[0]), name


def test_every_ray_case_differs_from_the_unbatched_rule():
    for case in [RK.ray_cases()[name] for name in RK.RAY_CASES] + [RK.rays_of("collisions"), RK.rays_of("hist_blocks")]:
        args = (case.points, case.walls, case.origins, case.directions, case.rho, case.max_t)
        assert ray_spec.status(*args) == 0
        t, hit = RS.rays(*args, case.ptr, case.ray_ptr)
        plain_t, plain_hit = ray_spec.rays(*args)
        assert not np.array_equal(hit, plain_hit) and not np.array_equal(t, plain_t)
        for bounces in RK.BOUNCES:
            got = RS.paths(*args, bounces, case.ptr, case.ray_ptr)
            plain = ray_path_spec.paths(*args, bounces)
            assert got[1].shape == (len(case.origins), bounces + 1) and not np.array_equal(got[1], plain[1])
            assert np.array_equal(got[1][:, 0], hit) and got[0][:, 0].tobytes() == t.tobytes()     # leg 0 is the ray
    for name in RK.POINT_CASES:                                                      # the rays through the point cases are valid calls
        case = RK.rays_of(name)
        assert ray_spec.status(case.points, case.walls, case.origins, case.directions, case.rho, case.max_t) == 0, name
        assert len(case.walls) == 4 and np.diff(case.ray_ptr).tolist() == [5] * (len(case.ptr) - 1)


# ---- the named cases and their wrong twins

def test_bridge():
    case = RK.cases()["bridge"]
    r = case.radius
    d = np.linalg.norm(case.points[0] - case.points[1])
    assert r < d < 2 * r and np.linalg.norm(case.points[0] - case.points[2]) < r > np.linalg.norm(case.points[1] - case.points[2])
    (labels, sizes, roots, cptr), (plain_labels, plain_sizes, _) = clusters_of("bridge")
    assert plain_sizes.tolist() == [3] and plain_labels.tolist() == [0, 0, 0]
    assert labels.tolist() == [0, 1, 2] and sizes.tolist() == [1, 1, 1] and roots.tolist() == [0, 1, 2] and cptr.tolist() == [0, 2, 3]
    assert int(RS.histogram(case.points, EDGES, case.ptr)[1].sum()) == 0 < int(hist_spec.histogram(case.points, EDGES)[1].sum())
    values = np.array([1.0, 2.0, 4.0])
    assert RS.cluster_sums(case.points, r, case.ptr, values, False)[3].tolist() == [[1.0], [2.0], [4.0]]
    assert cluster_sums_spec.cluster_sums(plain_labels, values, 1, False)[0].tolist() == [[7.0]]


def test_neighbours_in_index():
    """The twin: a union over the partners j < i that does not ask for j >= ptr[b] -- the unbatched graph."""
    case = RK.cases()["neighbours_in_index"]
    (labels, _, _, _), (plain_labels, _, _) = clusters_of("neighbours_in_index")
    offsets, partners, _ = pairs_spec.pairs(case.points, case.radius)
    for at in case.ptr[1:-1]:
        assert at - 1 in partners[offsets[at]:offsets[at + 1]]                       # closer than r, and j < i
        assert labels[at] != labels[at - 1] and plain_labels[at] == plain_labels[at - 1]


def test_collisions_collide_under_the_hash():
    """test_batch_cpu.py::test_collisions_really_collide's mirror of pairs_bucket: rows of one cloud meet members of
    another in the buckets of their nine cells, so the clusters and the rays need the index test as the pair list does."""
    from sand_crate_amd import _native as N
    case = RK.cases()["collisions"]
    n = len(case.points)
    buckets = N.pairs_buckets(n)
    cells = np.floor(case.points / (case.radius * N.PAIRS_CELL_FACTOR)).astype(np.int64)
    cloud = BS.cloud_of(case.ptr, n)
    by_bucket = {}
    for i, ((cx, cy), b) in enumerate(zip(cells, cloud)):
        by_bucket.setdefault(N.pairs_bucket(int(cx), int(cy), buckets, int(b)), []).append(i)
    lower = 0                                                                        # ... with a SMALLER index: the union's j < i
    for i, ((cx, cy), b) in enumerate(zip(cells, cloud)):
        walk = {N.pairs_bucket(int(cx) + ox, int(cy) + oy, buckets, int(b)) for ox in (-1, 0, 1) for oy in (-1, 0, 1)}
        lower += any(cloud[j] != b and j < i for bucket in walk for j in by_bucket.get(bucket, ()))
    assert lower >= 100


def test_hist_blocks():
    """The twin: a workgroup's column sums credited to the cloud of its first row."""
    case = RK.cases()["hist_blocks"]
    W = RK.HIST_BLOCK
    for ptr, rows in ((case.ptr, case.points), (case.query_ptr, case.queries)):
        sizes = np.diff(ptr)
        assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any() and W in ptr.tolist()
        cloud = BS.cloud_of(ptr, len(rows))
        assert len(set(cloud[:W].tolist())) >= 3                                     # three clouds in the first workgroup
        assert any(ptr[b] // W != (ptr[b + 1] - 1) // W for b in range(len(sizes)) if sizes[b])   # a cloud over two
    for bins in RK.HIST_BINS:
        edges = np.linspace(0.0, case.radius, bins + 1)
        for queries, qptr in ((None, None), (case.queries, case.query_ptr)):
            table, total = RS.histogram(case.points, edges, case.ptr, queries, qptr)
            cloud = BS.cloud_of(case.ptr if qptr is None else qptr, len(table))
            twin = np.zeros_like(total)
            for base in range(0, len(table), W):
                twin[cloud[base]] += table[base:base + W].astype(np.int64).sum(axis=0)
            assert total.sum() == twin.sum() > 0 and not np.array_equal(total, twin), bins
            empty = np.diff(case.ptr if qptr is None else qptr) == 0
            assert not total[empty].any()


def test_dead_cloud():
    case = RK.cases()["dead_cloud"]
    assert not np.isfinite(case.points[case.ptr[1]:case.ptr[2]]).all(axis=1).any()
    (labels, sizes, roots, cptr), _ = clusters_of("dead_cloud")
    assert cptr[1] == cptr[2] and 0 < cptr[1] < cptr[3] and (labels[case.ptr[1]:case.ptr[2]] == -1).all()
    assert not RS.histogram(case.points, EDGES, case.ptr)[1][1].any()


def test_long_chain():
    case = RK.cases()["long_chain"]
    (labels, sizes, roots, cptr), _ = clusters_of("long_chain")
    chain = int(np.argmax(sizes))
    assert sizes[chain] == 70 > 64 and chain >= cptr[1] > 0 and roots[chain] == case.ptr[1] > 0
    assert cluster_sums_spec.levels(70) >= 2
    members = np.flatnonzero(labels == chain)
    assert members.min() == case.ptr[1] and not np.array_equal(case.points[members][:, 0], np.sort(case.points[members][:, 0]))


def test_occluder():
    case = RK.ray_cases()["occluder"]
    args = (case.points, case.walls, case.origins, case.directions, case.rho, case.max_t)
    t, hit = RS.rays(*args, case.ptr, case.ray_ptr)
    plain_t, plain_hit = ray_spec.rays(*args)
    near, far = 3, 4                                                                 # global rows: cloud 0's disc, cloud 1's
    assert case.ptr.tolist() == [0, 4, 5, 5] and case.ray_ptr.tolist() == [0, 2, 5, 7]
    assert hit[:2].tolist() == [near, near] and plain_hit[2:5].tolist() == [near, near, near]
    assert hit[2:5].tolist() == [far, far, far] and (t[2:5] > plain_t[2:5]).all()
    assert hit[5:].tolist() == [-2, -2] and plain_hit[5] == near                    # the empty cloud's rays: the wall alone


def wrong_skip(case, bounces):
    """The twin of path_skip: the disc a leg leaves out kept as a cloud-local index and compared with global ones."""
    out = []
    for b in range(len(case.ptr) - 1):
        lo = int(case.ptr[b])

        def search(o, d, m, pts, walls, rho, skip_wall, skip_disc, later, wrong, state, lo=lo):
            return ray_path_spec.brute(o, d, m, pts, walls, rho, skip_wall, skip_disc - lo if skip_disc >= lo else -1, later,
                                       wrong, state)
        rows = slice(case.ray_ptr[b], case.ray_ptr[b + 1])
        got = ray_path_spec.paths(case.points[lo:case.ptr[b + 1]], case.walls, case.origins[rows], case.directions[rows], case.rho,
                                  case.max_t, bounces, search=search)
        out.append(np.where(got[1] >= 0, got[1] + lo, got[1]))
    return np.concatenate(out)


def test_path_skip():
    case = RK.ray_cases()["path_skip"]
    lo = int(case.ptr[1])
    assert lo == 2
    for bounces in (1, 3):
        t, hit, P, n, end = RS.paths(case.points, case.walls, case.origins, case.directions, case.rho, case.max_t, bounces,
                                     case.ptr, case.ray_ptr)
        assert hit[1, :2].tolist() == [lo + 2, lo + 0] and lo + 2 >= lo > 0          # leg 1 leaves global disc 4, meets global 2
        assert abs(n[1, 0, 0] + np.sqrt(0.5)) < 1e-9 and abs(n[1, 0, 1] - np.sqrt(0.5)) < 1e-9
        twin = wrong_skip(case, bounces)
        assert twin[1, 0] == lo + 2 and twin[1, 1] != lo + 0 and not np.array_equal(twin, hit)
