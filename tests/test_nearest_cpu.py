"""CPU-side checks of the device nearest-k tables: the rule (tests/nearest_spec.py) against the pair list's rule, the
properties the cases of tests/nearest_cases.py are named for, the symbol in the header, the ctypes table and the built
library, the constants mirrored from the kernel's source, the torch helpers of sand_crate_amd/pairs.py, and the tensor
checks of `Engine.pairs_nearest`, which refuse before the library is touched.  No GPU."""
import functools
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import nearest_cases as NK
import nearest_spec as NS
import pairs_cases as K
import pairs_spec as S
from sand_crate_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sandcrate_hip.h"
KERNELS = ROOT / "sand_crate_amd" / "csrc" / "sc_nearest.h"
SELF_CASES = [name for name, case in NK.cases().items() if case[3] is None]
SMALL_SELF_CASES = [name for name in SELF_CASES if len(NK.cases()[name][0]) < 5000]   # (brute force twice: three_passes is left out)
QUERY_CASES = [name for name, case in NK.cases().items() if case[3] is not None]


@functools.lru_cache(maxsize=None)
def spec(name):
    return NS.nearest(*NK.cases()[name])


def check_table(neighbors, d2, partners, k):
    """What holds for every table: the shape, the padding, and rows ascending in (d2, j)."""
    rows = len(partners)
    assert neighbors.dtype == partners.dtype == np.int64 and d2.dtype == np.float64
    assert neighbors.shape == d2.shape == (rows, k) and partners.shape == (rows,)
    used = np.minimum(partners, k)
    place = np.arange(k)[None, :]
    pad = place >= used[:, None]
    assert (neighbors[pad] == -1).all() and np.isposinf(d2[pad]).all()
    assert (neighbors[~pad] >= 0).all() and np.isfinite(d2[~pad]).all()
    both = ~pad[:, 1:]
    a_d, b_d, a_j, b_j = d2[:, :-1][both], d2[:, 1:][both], neighbors[:, :-1][both], neighbors[:, 1:][both]
    assert ((a_d < b_d) | ((a_d == b_d) & (a_j < b_j))).all()


# ---- the rule

LINE = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.5, 0.0], [np.nan, 0.0], [0.0, 0.25], [0.0, np.inf], [0.0, -1.0]])


def test_spec_on_a_hand_made_set():
    neighbors, d2, partners = NS.nearest(LINE, 1.0, 3)
    check_table(neighbors, d2, partners, 3)
    assert partners.tolist() == [5, 2, 1, 3, 0, 2, 0, 1]
    assert neighbors[0].tolist() == [5, 3, 1] and d2[0].tolist() == [0.0625, 0.25, 1.0]     # 1, 2 and 7 tie at 1.0: 1 stays
    assert neighbors[2].tolist() == [0, -1, -1] and d2[2].tolist() == [1.0, np.inf, np.inf]
    assert neighbors[4].tolist() == [-1] * 3 and neighbors[6].tolist() == [-1] * 3
    neighbors, d2, partners = NS.nearest(LINE, 1.0, 5)
    assert neighbors[0].tolist() == [5, 3, 1, 2, 7]                                          # the tie in index order
    assert NS.nearest(LINE, 1.0, 1)[0][:, 0].tolist() == [5, 3, 0, 0, -1, 0, -1, 0]


def test_spec_with_queries():
    queries = np.array([[0.0, 0.0], [0.75, 0.0], [np.nan, 0.0], [5.0, 5.0], [0.0, -np.inf]])
    neighbors, d2, partners = NS.nearest(LINE, 1.0, 2, queries)
    check_table(neighbors, d2, partners, 2)
    assert partners.tolist() == [6, 4, 0, 0, 0]
    assert neighbors.tolist() == [[0, 5], [1, 3], [-1, -1], [-1, -1], [-1, -1]]              # a query on point 0 has it at d2 0
    assert d2[0].tolist() == [0.0, 0.0625] and d2[1].tolist() == [0.0625, 0.0625]            # ... and a tie decided by j
    empty = NS.nearest(np.zeros((0, 2)), 1.0, 2, queries)
    assert empty[0].shape == (5, 2) and (empty[0] == -1).all() and not empty[2].any()
    none = NS.nearest(LINE, 1.0, 2, np.zeros((0, 2)))
    assert none[0].shape == none[1].shape == (0, 2) and none[2].shape == (0,)
    assert [a.shape for a in NS.nearest(np.zeros((0, 2)), 1.0, 4)] == [(0, 4), (0, 4), (0,)]


def test_in_domain():
    pts = np.array([[0.0, 0.0], [np.inf, np.nan]])
    assert NS.in_domain(pts, 0.5) and NS.in_domain(pts, 0.5, np.array([[np.nextafter(2.0 ** 30, 0), -np.inf]]))
    assert not NS.in_domain(pts, 0.5, np.array([[0.0, -(2.0 ** 30)]]))
    assert not NS.in_domain(np.array([[2.0 ** 30, 0.0]]), 0.5, np.zeros((1, 2)))


@pytest.mark.parametrize("name", SMALL_SELF_CASES)
def test_self_form_is_the_pair_list_sorted_and_cut(name):
    points, radius, k, _ = NK.cases()[name]
    neighbors, d2, partners = spec(name)
    check_table(neighbors, d2, partners, k)
    offsets, js, ds = S.pairs(points, radius)
    assert np.array_equal(partners, np.diff(offsets))
    for r in range(len(points)):
        row_j, row_d = js[offsets[r]:offsets[r + 1]], ds[offsets[r]:offsets[r + 1]]
        order = np.argsort(row_d, kind="stable")[:k]                                         # (the row ascends in j)
        assert np.array_equal(neighbors[r, :len(order)], row_j[order])
        assert d2[r, :len(order)].tobytes() == row_d[order].tobytes()


@pytest.mark.parametrize("name", QUERY_CASES)
def test_query_form_is_the_row_of_the_query_appended_as_a_point(name):
    points, radius, k, queries = NK.cases()[name]
    neighbors, d2, partners = spec(name)
    check_table(neighbors, d2, partners, k)
    n = len(points)
    for r in range(0, len(queries), 7):
        offsets, js, ds = S.pairs(np.concatenate([points, queries[r:r + 1]]), radius)
        row_j, row_d = js[offsets[n]:offsets[n + 1]], ds[offsets[n]:offsets[n + 1]]
        assert partners[r] == len(row_j)
        order = np.argsort(row_d, kind="stable")[:k]
        assert np.array_equal(neighbors[r, :len(order)], row_j[order])
        assert d2[r, :len(order)].tobytes() == row_d[order].tobytes()


# ---- every case has the property it is named for

def test_cases_cover_the_pair_search_and_stay_small():
    cases = NK.cases()
    for name, (points, radius) in K.cases().items():
        found = [c for key, c in cases.items() if key.startswith(name + "_k_")]
        assert len(found) == 1 and found[0][0] is points and found[0][1] == radius
    assert {c[2] for c in cases.values()} >= set(NK.KS)
    for name, (points, radius, k, queries) in cases.items():
        assert len(points) <= 17000 and 1 <= k <= N.NEAREST_MAX_K and (queries is None or len(queries) <= 1000)
        assert NS.in_domain(points, radius, queries) == (name != NK.OUTSIDE)


@pytest.mark.parametrize("k", NK.KS)
def test_groups_have_rows_on_each_side_of_k(k):
    partners = spec(f"groups_k_{k}")[2]
    assert set(partners.tolist()) == {0, k - 1, k, k + 1}
    assert (partners > k).sum() == k + 2


@pytest.mark.parametrize("k", [2, 3])
def test_tie_at_the_cut(k):
    points, radius, _, _ = NK.cases()[f"tie_at_the_cut_k_{k}"]
    neighbors, d2, partners = spec(f"tie_at_the_cut_k_{k}")
    inner = np.nonzero(partners == 4)[0]
    assert len(inner) == 25
    for r in inner:
        offsets, js, ds = S.pairs(points, radius)
        row_j, row_d = js[offsets[r]:offsets[r + 1]], ds[offsets[r]:offsets[r + 1]]
        assert len(set(row_d.tobytes()[8 * s:8 * s + 8] for s in range(4))) == 1             # four bit-equal d2
        assert neighbors[r].tolist() == row_j[:k].tolist()                                   # j decides which stay


@pytest.mark.parametrize("k", [64, 5])
def test_pile(k):
    neighbors, d2, partners = spec(f"pile_70_k_{k}")
    assert (partners == 69).all() and 69 > N.NEAREST_MAX_K and not d2.any()
    for i in range(70):
        assert neighbors[i].tolist() == [j for j in range(70) if j != i][:k]


@pytest.mark.parametrize("descending", [True, False])
def test_arrival_order(descending):
    word = "descending" if descending else "ascending"
    points, radius, _, _ = NK.cases()[f"{word}_arrival_k_16"]
    assert NK.cases()[f"{word}_arrival_k_33"][0].tobytes() == points.tobytes()
    order = NK.arrival(points, radius, points[0], self_index=0)
    assert len(order) == 50 == spec(f"{word}_arrival_k_16")[2][0]                            # every partner of row 0, once
    assert len({K.cells_of(points[[j]], radius)[0] for j in order}) == 3                     # from three cells
    d = (points[0, 0] - points[order, 0]) ** 2 + (points[0, 1] - points[order, 1]) ** 2
    assert (np.diff(d) < 0).all() if descending else (np.diff(d) > 0).all()
    # the table is the end (the start) of the arrival order
    want = order[::-1][:16] if descending else order[:16]
    assert spec(f"{word}_arrival_k_16")[0][0].tolist() == want


def test_arrival_is_the_walk_of_every_partner():
    points, radius, _, _ = NK.cases()[next(name for name in NK.cases() if name.startswith("bucket_sharing"))]
    offsets, js, _ = S.pairs(points, radius)
    for r in range(len(points)):
        assert sorted(NK.arrival(points, radius, points[r], self_index=r)) == js[offsets[r]:offsets[r + 1]].tolist()


def test_nine_cells():
    points, radius, k, _ = NK.cases()["nine_cells_k_64"]
    neighbors, d2, partners = spec("nine_cells_k_64")
    assert k == 64 and partners[0] == 108
    cells = K.cells_of(points, radius)
    order = NK.arrival(points, radius, points[0], self_index=0)
    per_cell = {}
    for j in order:
        per_cell[cells[j]] = per_cell.get(cells[j], 0) + 1
    assert len(per_cell) == 9 and set(per_cell.values()) == {12}
    kept = {cells[j] for j in neighbors[0]}
    assert len(kept) >= 5 and (neighbors[0] >= 0).all()                                      # a full row, cut across the cells


def test_width_sizes():
    sizes = [63, 64, 65, 127, 128, 129]
    assert NK.width_sizes() == [(n, k) for k in (16, 17, 33) for n in sizes]
    assert [N.nearest_slots(k) for k in (16, 17, 33)] == [16, 32, 64]                         # one k per kernel
    for n, k in NK.width_sizes():
        points, _, case_k, _ = NK.cases()[f"width_n_{n}_k_{k}"]
        assert len(points) == n and case_k == k and n % N.nearest_width(k) in (63, 0, 1)
        partners = spec(f"width_n_{n}_k_{k}")[2]
        assert (partners > k).any() and (partners < k).any()


def test_query_cases():
    cases = NK.cases()
    assert len(cases["q_0"][3]) == 0 and len(cases["n_0_q_10"][0]) == 0 and len(cases["n_0_q_10"][3]) == 10
    assert not spec("n_0_q_10")[2].any()
    points, _, _, queries = cases["query_on_a_point"]
    neighbors, d2, _ = spec("query_on_a_point")
    for r in range(0, 40, 4):
        assert d2[r, 0] == 0.0 and points[neighbors[r, 0]].tobytes() == queries[r].tobytes()
    queries = cases["query_not_finite"][3]
    bad = ~np.isfinite(queries).all(axis=1)
    partners = spec("query_not_finite")[2]
    assert bad.sum() == 4 and not partners[bad].any() and partners[~bad].all()
    points, radius, _, queries = cases["query_in_empty_cells"]
    occupied = set(K.cells_of(points, radius))
    nine = lambda c: {(c[0] + dx, c[1] + dy) for dx in (-1, 0, 1) for dy in (-1, 0, 1)}  # noqa: E731
    lonely = [not (nine(c) & occupied) for c in K.cells_of(queries, radius)]
    assert sum(lonely) >= 4 and not all(lonely)
    assert not spec("query_in_empty_cells")[2][np.array(lonely)].any()
    points, radius, _, queries = cases[NK.OUTSIDE]
    assert S.in_domain(points, radius) and not S.in_domain(queries, radius)
    assert (np.abs(queries) / radius == 2.0 ** 31).sum() == 1
    assert NS.in_domain(*[cases["query_one_ulp_inside"][i] for i in (0, 1, 3)])
    points, radius, _, queries = cases["query_at_the_rim"]
    assert (np.abs(queries).max(axis=1) / radius > 2.0 ** 31 - 2).all() and spec("query_at_the_rim")[2].sum() >= 4


# ---- the boundary

def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert found, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in found.group(1).split(",")]


def test_symbol_is_declared_and_the_versions_stay():
    assert declaration("sc_pairs_nearest_device") == [
        "sc_ctx* ctx", "const double* dev_queries", "int64_t n_queries", "int32_t k", "int64_t* dev_neighbors",
        "double* dev_d2", "int64_t* dev_partners", "int64_t room_rows", "int64_t* dev_counts"]
    header = HEADER.read_text()
    assert re.search(r"#define SC_ABI_VERSION 5\b", header) and re.search(r"#define SC_NUM_KERNELS 12\b", header)
    assert re.search(r"enum \{ SC_NEAREST_MAX_K = 64 \};", header)
    assert N.NUM_KERNELS == 12


def test_ctypes_table_matches_the_header():
    import ctypes as C
    res, argtypes = N.SIGNATURES["sc_pairs_nearest_device"]
    kinds = {"sc_ctx*": C.c_void_p, "const double*": C.c_void_p, "double*": C.c_void_p, "int64_t*": C.c_void_p,
             "int64_t": C.c_int64, "int32_t": C.c_int32}                                    # (device addresses travel as void*)
    want = [kinds[a.rsplit(" ", 1)[0]] for a in declaration("sc_pairs_nearest_device")]
    assert res is C.c_int and len(argtypes) == 9 and argtypes == want


def test_constants_mirror_the_kernel_source():
    text = KERNELS.read_text()

    def const(name):
        return int(re.search(r"\b" + name + r"\s*=\s*(\d+)", text).group(1))

    assert const("kNearestMaxK") == N.NEAREST_MAX_K == 64
    assert const("kNearestBlock") == N.NEAREST_BLOCK == 64
    assert N.NEAREST_SLOTS == (const("kNearestFewK"), const("kNearestMidK"), const("kNearestMaxK"))
    assert [N.nearest_slots(k) for k in range(1, 65)] == [16] * 16 + [32] * 16 + [64] * 32
    assert {N.nearest_width(k) for k in range(1, 65)} == {64}
    for slots in N.NEAREST_SLOTS:                                                            # 12 bytes per place, padded lines
        assert 12 * slots * (N.NEAREST_BLOCK + const("kNearestPad")) <= 50 * 1024
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            N.nearest_width(k)
        with pytest.raises(ValueError):
            N.nearest_slots(k)


def test_kernels_are_included_once_after_the_pairs():
    text = (ROOT / "sand_crate_amd" / "csrc" / "sandcrate_hip.hip").read_text()
    assert text.count('#include "sc_nearest.h"') == 1
    assert text.index('#include "sc_clusters.h"') < text.index('#include "sc_nearest.h"')


def test_library_exports_the_call_and_refuses_a_null_context():
    import ctypes
    from sand_crate_amd import build
    lib = ctypes.CDLL(str(build.build()))
    fn = lib.sc_pairs_nearest_device
    fn.restype, fn.argtypes = N.SIGNATURES["sc_pairs_nearest_device"]
    lib.sc_last_error.restype = ctypes.c_char_p
    assert fn(None, None, 0, 1, None, None, None, 0, None) == N.ERR_ARG                      # before any HIP call: no GPU needed
    assert b"null context" in lib.sc_last_error()
    assert lib.sc_abi_version() == 5


def test_python_surface():
    from sand_crate_amd import Crate
    from sand_crate_amd.engine import Engine
    p = inspect.signature(Engine.pairs_nearest).parameters
    assert list(p) == ["self", "neighbors", "d2", "partners", "k", "queries", "counts", "room", "query_batch"]
    assert p["d2"].default is None and p["partners"].default is None and p["queries"].default is None
    assert all(p[name].kind is inspect.Parameter.KEYWORD_ONLY for name in ("k", "queries", "counts", "room"))
    p = inspect.signature(Crate.neighbor_tensors).parameters
    assert list(p) == ["self", "k", "radius", "points", "queries", "squared_distances", "partner_counts", "sync", "batch",
                       "query_batch"]
    assert p["radius"].default is None and p["sync"].default is True
    assert all(p[name].kind is inspect.Parameter.KEYWORD_ONLY for name in list(p)[3:])


# ---- the torch helpers

def test_neighbor_mask_and_edge_index():
    import torch
    from sand_crate_amd import pairs
    table = torch.from_numpy(NS.nearest(LINE, 1.0, 3)[0])
    mask = pairs.neighbor_mask(table)
    assert mask.dtype == torch.bool and mask.sum(dim=1).tolist() == [3, 2, 1, 3, 0, 2, 0, 1]
    edges = pairs.neighbor_edge_index(table)
    assert edges.dtype == torch.int64 and edges.shape == (2, 12)
    assert edges[0].tolist() == [0, 0, 0, 1, 1, 2, 3, 3, 3, 5, 5, 7]
    assert edges[1].tolist() == table[mask].tolist() and edges[1][:3].tolist() == [5, 3, 1]  # nearest first
    none = torch.full((4, 2), -1, dtype=torch.int64)
    assert pairs.neighbor_edge_index(none).shape == (2, 0) and not pairs.neighbor_mask(none).any()
    assert pairs.neighbor_edge_index(torch.zeros((0, 5), dtype=torch.int64)).shape == (2, 0)


# ---- tensors are checked before the library is touched

class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


class Fake:
    """What the checks look at of a CUDA tensor, without a GPU."""

    def __init__(self, shape, dtype="int64", contiguous=True, index=0):
        self.is_cuda = True
        self.shape = tuple(shape)
        self.dtype = f"torch.{dtype}"
        self._contiguous = contiguous
        self.device = type("Device", (), {"index": index})()

    def is_contiguous(self):
        return self._contiguous

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        raise AssertionError("the tensor's address was taken")


@pytest.fixture()
def engine():
    from sand_crate_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._lib = eng._ctx = Untouchable()
    eng.device, eng.capacity = 0, 64
    yield eng
    eng._ctx = None   # (nothing to close)


def good():
    return dict(neighbors=Fake((8, 4)), d2=Fake((8, 4), "float64"), partners=Fake((8,)), k=4, queries=Fake((8, 2), "float64"),
                counts=Fake((2,)))


def test_nearest_refuses_cpu_tensors(engine):
    import torch
    for name, shape, dtype in (("neighbors", (8, 4), torch.int64), ("d2", (8, 4), torch.float64), ("partners", (8,), torch.int64),
                               ("queries", (8, 2), torch.float64), ("counts", (2,), torch.int64)):
        args = good()
        args[name] = torch.zeros(shape, dtype=dtype)
        with pytest.raises(ValueError, match=name):
            engine.pairs_nearest(**args)
    for name in ("neighbors", "counts"):
        args = good()
        args[name] = None
        with pytest.raises(ValueError, match=name):
            engine.pairs_nearest(**args)
    with pytest.raises(ValueError, match="neighbors"):
        engine.pairs_nearest(np.zeros((8, 4), dtype=np.int64), k=4, counts=Fake((2,)))


@pytest.mark.parametrize("name,bad", [
    ("neighbors", Fake((8, 4), "int32")), ("neighbors", Fake((8,))), ("neighbors", Fake((8, 5))), ("neighbors", Fake((8, 4, 1))),
    ("neighbors", Fake((8, 4), contiguous=False)), ("neighbors", Fake((8, 4), index=1)), ("neighbors", Fake((8, 4), "float64")),
    ("d2", Fake((8, 4))), ("d2", Fake((7, 4), "float64")), ("d2", Fake((8, 3), "float64")), ("d2", Fake((8, 4), "float64", index=1)),
    ("d2", Fake((8, 4), "float32")), ("d2", Fake((8, 4), "float64", contiguous=False)),
    ("partners", Fake((7,))), ("partners", Fake((8, 1))), ("partners", Fake((8,), "int32")), ("partners", Fake((8,), index=1)),
    ("queries", Fake((8, 2))), ("queries", Fake((8, 3), "float64")), ("queries", Fake((16,), "float64")),
    ("queries", Fake((8, 2), "float64", contiguous=False)), ("queries", Fake((8, 2), "float64", index=1)),
    ("counts", Fake((1,))), ("counts", Fake((2,), "int32")), ("counts", Fake((2, 1))), ("counts", Fake(())),
    ("counts", Fake((2,), index=1)),
])
def test_nearest_refuses_wrong_dtypes_shapes_and_devices(engine, name, bad):
    args = good()
    args[name] = bad
    with pytest.raises(ValueError, match=name):
        engine.pairs_nearest(**args)


def test_nearest_refuses_k_and_rooms_beyond_the_tensors(engine):
    for k in (0, -1, 65):
        with pytest.raises(ValueError, match="k must be"):
            engine.pairs_nearest(**{**good(), "k": k})
    with pytest.raises(ValueError, match="room"):
        engine.pairs_nearest(**good(), room=9)


def test_neighbor_tensors_refuses_k_before_anything_is_launched():
    from sand_crate_amd import Crate
    crate = Crate.__new__(Crate)
    crate._engine = Untouchable()
    for k in (0, 65, -3):
        with pytest.raises(ValueError, match="k must be"):
            crate.neighbor_tensors(k)
