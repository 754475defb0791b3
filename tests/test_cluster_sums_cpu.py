"""CPU-side checks of the per-cluster sums: the rule (tests/cluster_sums_spec.py) against math.fsum and on hand-made
inputs, that the cases of tests/cluster_sums_cases.py have the properties they are named for, the observables' channel
table against tests/probe_spec.py, the symbol in the header, the ctypes table and the built library, the pinned parameter
lists, and the tensor checks of `Engine.pairs_cluster_sums`, which refuse before the library is touched.  No GPU."""
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import cluster_spec as CS
import cluster_sums_cases as SK
import cluster_sums_spec as SS
import probe_spec as PS
from test_clusters_cpu import Fake, Untouchable, declaration

ROOT = Path(__file__).resolve().parent.parent
SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 262145)


# ---- the rule

@pytest.mark.parametrize("n", SIZES)
def test_tree_stays_within_its_bound_of_fsum(n):
    rs = np.random.RandomState(n)
    for v in (rs.standard_normal(n), rs.standard_normal(n) * 10.0 ** rs.randint(-3, 4, size=n), SK.order_channel(n)):
        got, exact = SS.tree(v), math.fsum(v.tolist())
        assert abs(got - exact) <= SS.bound(v), (n, got, exact)


def test_tree_by_hand():
    assert SS.tree([1.5]) == 1.5 and SS.tree([1.0, 2.0, 3.0]) == 6.0
    assert math.copysign(1.0, SS.tree([-0.0])) == 1.0 and math.copysign(1.0, SS.tree([-0.0] * 65)) == 1.0   # the padding is +0.0
    assert math.copysign(1.0, -0.0 + -0.0) == -1.0                                  # ... which the terms alone would not give
    # pairs first: (1e16 + 1) + (-1e16 + 1) loses both ones; one after the other keeps the last
    assert SS.tree([1e16, 1.0, -1e16, 1.0]) == 0.0 and ((1e16 + 1.0) + -1e16) + 1.0 == 1.0
    # the 65th term is a group of its own: added last, after the 64 before it have met
    v = np.array([1e16] + [1.0] * 62 + [-1e16, 1.0])
    assert SS.tree(v) == SS.tree(v[:64]) + 1.0
    assert [SS.levels(n) for n in (1, 64, 65, 4096, 4097, 262144, 262145)] == [1, 1, 2, 2, 3, 3, 4]
    assert np.isnan(SS.tree([np.inf, -np.inf])) and SS.tree([np.inf, 1.0]) == np.inf


def test_cluster_sums_by_hand():
    labels = np.array([1, 0, -1, 1, 0, 1])
    values = np.array([[1.0, 10.0], [2.0, 20.0], [np.nan, np.nan], [3.0, -30.0], [4.0, 40.0], [5.0, 50.0]])
    sums, mins, maxs = SS.cluster_sums(labels, values)
    assert sums.tolist() == [[6.0, 60.0], [9.0, 30.0]] and mins.tolist() == [[2.0, 20.0], [1.0, -30.0]]
    assert maxs.tolist() == [[4.0, 40.0], [5.0, 50.0]]
    values[3, 0] = np.nan                                                           # a NaN member: sum, min and max
    sums, mins, maxs = SS.cluster_sums(labels, values)
    assert np.isnan(sums[1, 0]) and np.isnan(mins[1, 0]) and np.isnan(maxs[1, 0]) and sums[1, 1] == 30.0 and sums[0, 0] == 6.0
    assert [a.shape for a in SS.cluster_sums(np.zeros(0, dtype=np.int64), np.zeros((0, 3)))] == [(0, 3)] * 3
    assert SS.cluster_sums(labels, values[:, 1])[0].tolist() == [[60.0], [30.0]]    # (n,) is one channel
    assert SS.same(np.array([1.0, np.nan]), np.array([1.0, -np.nan])) and not SS.same(np.array([0.0]), np.array([-0.0]))
    assert not SS.same(np.array([1.0, np.nan]), np.array([np.nan, 1.0]))


# ---- the cases

def serial(v):
    total = 0.0
    for x in v.tolist():
        total += x
    return total


def members(labels, c):
    return np.flatnonzero(labels == c)


def test_ladder_has_its_sizes_and_interleaves():
    pts, values, labels, sizes, roots = SK.cases()["ladder"]
    assert sorted(sizes.tolist()) == list(SK.LADDER_SIZES) and len(pts) == sum(SK.LADDER_SIZES) and values.shape == (len(pts), 8)
    for g, w in zip(CS.clusters(pts, SK.RADIUS), (labels, sizes, roots)):
        assert g.tobytes() == w.tobytes()
    for c in np.flatnonzero(sizes >= 63):                                           # only a sort brings a cluster together
        m = members(labels, c)
        assert m[-1] - m[0] + 1 > 2 * len(m)


def test_ladder_values_tell_the_order():
    _, values, labels, sizes, _ = SK.cases()["ladder"]
    for c in np.flatnonzero(sizes >= 63):
        rows = values[members(labels, c)]
        want = [SS.tree(rows[:, f]) for f in range(8)]
        assert any(serial(rows[:, f]) != want[f] for f in range(8))                 # not a serial sum
        assert np.sum(rows[:, 3]) != want[3] or np.sum(rows[:, 4]) != want[4]       # not NumPy's
        swapped = rows.copy()
        swapped[[0, len(rows) - 1]] = swapped[[len(rows) - 1, 0]]                   # not with two members swapped
        assert any(SS.tree(swapped[:, f]) != want[f] for f in range(8))
    sums, mins, maxs = SS.cluster_sums(labels, values)
    assert np.isfinite(sums).all() and (mins <= maxs).all()


def test_chain4_reaches_the_fourth_level_by_a_construction_proved_short():
    pts, values, labels, sizes, roots = SK.cases()["chain4"]
    assert sizes.tolist() == [SK.CHAIN4] + [1] * SK.CHAIN4_SINGLETONS and SS.levels(SK.CHAIN4) == 4 and SS.levels(SK.CHAIN4 - 1) == 3
    assert roots.tolist() == [0] + [SK.CHAIN4 + k for k in range(SK.CHAIN4_SINGLETONS)] and len(pts) == SK.CHAIN4 + SK.CHAIN4_SINGLETONS
    short = SK.chain4(length=4097)                                                  # the same construction, where the spec scales
    for g, w in zip(CS.clusters(short[0], SK.RADIUS), short[2:]):
        assert g.tobytes() == w.tobytes()
    # the long one differs from it in the chain's length only: the same spacing, the same rows
    assert np.array_equal(pts[:4097], short[0][:4097]) and np.array_equal(pts[SK.CHAIN4:, 1], short[0][4097:, 1])
    assert np.array_equal(np.diff(pts[:SK.CHAIN4, 0]), np.full(SK.CHAIN4 - 1, 0.5)) and not pts[:SK.CHAIN4, 1].any()
    rows = values[:SK.CHAIN4]
    assert serial(rows[:, 0]) != SS.tree(rows[:, 0]) or serial(rows[:, 1]) != SS.tree(rows[:, 1])


def test_isolated_dead_rows_are_nan_and_in_no_cluster():
    pts, values, labels, sizes, roots = SK.cases()["isolated_dead"]
    for g, w in zip(CS.clusters(pts, SK.RADIUS), (labels, sizes, roots)):
        assert g.tobytes() == w.tobytes()
    dead = labels < 0
    assert dead.sum() == 90 and len(sizes) == 410 and (sizes == 1).all()
    assert np.isnan(values[dead]).all() and np.isfinite(values[~dead]).all()
    sums, mins, maxs = SS.cluster_sums(labels, values)
    assert np.isfinite(sums).all() and sums.tobytes() == values[~dead].tobytes() == mins.tobytes() == maxs.tobytes()


def test_special_values():
    pts, values, labels, sizes, roots = SK.cases()["special"]
    for g, w in zip(CS.clusters(pts, SK.RADIUS), (labels, sizes, roots)):
        assert g.tobytes() == w.tobytes()
    assert sizes.tolist() == [3, 5, 4, 1]
    sums, mins, maxs = SS.cluster_sums(labels, values)
    assert sums[0, 0] == 0.0 and math.copysign(1.0, sums[0, 0]) == 1.0 and math.copysign(1.0, mins[0, 0]) == -1.0
    assert np.isnan([sums[1, 0], mins[1, 0], maxs[1, 0]]).all()
    assert np.isnan(sums[2, 0]) and mins[2, 0] == -np.inf and maxs[2, 0] == np.inf
    assert sums[3, 0] == mins[3, 0] == maxs[3, 0] == -7.25 and np.isfinite(sums[:, 1]).all()


# ---- the observables

def test_channel_table_is_the_probes_terms():
    import torch
    from sand_crate_amd import pairs, probe
    rs = np.random.RandomState(5)
    xy, vxy, p = rs.rand(300, 2), rs.standard_normal((300, 2)) * 3.0, rs.standard_normal(300)
    want = SS.channels(xy, vxy, p)
    terms = PS.terms(xy, vxy, p)
    for k, name in enumerate(PS.SUMS):
        assert want[:, k].tobytes() == terms[name].tobytes()
    assert want[:, 6].tobytes() == (vxy[:, 0] * vxy[:, 0] + vxy[:, 1] * vxy[:, 1]).tobytes() and (want[:, 4] == 0.5 * want[:, 6]).all()
    assert want[:, 7].tolist() == (p > 0).astype(float).tolist()
    got = pairs.cluster_channels(torch.from_numpy(xy), torch.from_numpy(vxy), torch.from_numpy(p))
    assert got.dtype == torch.float64 and got.is_contiguous() and got.numpy().tobytes() == want.tobytes()
    assert pairs.CLUSTER_FIELDS == SS.FIELDS and pairs.CLUSTER_CHANNELS == SS.CHANNELS and len(pairs.CLUSTER_FIELDS) == 14
    assert all(name in probe.FIELDS for name in pairs.CLUSTER_FIELDS)
    labels = rs.randint(-1, 7, size=300)
    labels[:7] = np.arange(7)
    sizes = np.bincount(labels[labels >= 0])
    t = torch.from_numpy(SS.observables(labels, sizes, xy, vxy, p))
    assert t.shape == (7, 14) and t[:, 0].tolist() == sizes.tolist()
    assert torch.equal(pairs.cluster_centers(t), t[:, 1:3] / t[:, :1]) and pairs.cluster_centers(t).shape == (7, 2)
    assert torch.equal(pairs.cluster_mean_velocities(t), t[:, 3:5] / t[:, :1])
    c = 3
    assert abs(float(pairs.cluster_centers(t)[c, 0]) - xy[labels == c, 0].mean()) < 1e-12


# ---- the boundary

def test_symbol_is_declared_and_the_versions_stay():
    assert declaration("sc_pairs_cluster_sums_device") == [
        "sc_ctx* ctx", "const double* dev_values", "int64_t values_rows", "int32_t channels", "double* dev_sums",
        "double* dev_mins", "double* dev_maxs", "int64_t room_clusters", "int64_t* dev_counts"]
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    assert re.search(r"#define SC_ABI_VERSION 5\b", header) and re.search(r"#define SC_NUM_KERNELS 12\b", header)
    assert re.search(r"SC_CLUSTER_SUMS_MAX_CHANNELS = 8\b", header)


def test_ctypes_table_matches_the_header():
    import ctypes as C
    from sand_crate_amd import _native as N
    res, argtypes = N.SIGNATURES["sc_pairs_cluster_sums_device"]
    kinds = {"sc_ctx*": C.c_void_p, "const double*": C.c_void_p, "double*": C.c_void_p, "int64_t*": C.c_void_p,
             "int64_t": C.c_int64, "int32_t": C.c_int32}
    want = [kinds[a.rsplit(" ", 1)[0]] for a in declaration("sc_pairs_cluster_sums_device")]
    assert res is C.c_int and argtypes == want
    assert N.CLUSTER_SUMS_MAX_CHANNELS == 8 and N.CLUSTER_SUMS_GROUP == SS.GROUP
    assert (N.CLUSTER_SUMS_DOMAIN, N.CLUSTER_SUMS_VALUES_SHORT) == (-1, -2)


def test_kernels_are_included_once_after_the_clusters():
    text = (ROOT / "sand_crate_amd" / "csrc" / "sandcrate_hip.hip").read_text()
    assert text.count('#include "sc_cluster_sums.h"') == 1
    assert text.index('#include "sc_clusters.h"') < text.index('#include "sc_cluster_sums.h"')


def test_library_exports_the_call_and_refuses_before_any_hip_call():
    import ctypes
    from sand_crate_amd import _native as N, build
    lib = ctypes.CDLL(str(build.build()))
    fn = lib.sc_pairs_cluster_sums_device
    fn.restype, fn.argtypes = N.SIGNATURES["sc_pairs_cluster_sums_device"]
    lib.sc_last_error.restype = ctypes.c_char_p
    assert fn(None, None, 0, 1, None, None, None, 0, None) == N.ERR_ARG             # no GPU needed
    assert b"null context" in lib.sc_last_error()
    assert lib.sc_abi_version() == 5


def test_python_surface():
    from sand_crate_amd import Crate
    from sand_crate_amd.engine import Engine
    p = inspect.signature(Engine.pairs_cluster_sums).parameters
    assert list(p) == ["self", "values", "sums", "mins", "maxs", "counts", "room_clusters"]
    assert p["mins"].default is None and p["maxs"].default is None and p["room_clusters"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("counts", "room_clusters"))
    assert p["counts"].default is inspect.Parameter.empty
    p = inspect.signature(Crate.cluster_sums).parameters
    assert list(p) == ["self", "values", "radius", "points", "extrema", "max_clusters"]
    assert p["radius"].default is None and p["points"].default is None and p["extrema"].default is False and p["max_clusters"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("points", "extrema", "max_clusters"))
    p = inspect.signature(Crate.cluster_observables).parameters
    assert list(p) == ["self", "radius", "max_clusters"] and p["radius"].default is None
    assert p["max_clusters"].kind is inspect.Parameter.KEYWORD_ONLY and p["max_clusters"].default is None
    # ... and the label's lists are as they were
    assert list(inspect.signature(Engine.pairs_label).parameters) == ["self", "labels", "sizes", "roots", "counts", "room", "room_clusters"]
    assert list(inspect.signature(Crate.cluster_tensors).parameters) == ["self", "radius", "points", "max_clusters"]


# ---- tensors are checked before the library is touched

@pytest.fixture()
def engine():
    from sand_crate_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng._lib = eng._ctx = Untouchable()
    eng.device, eng.capacity = 0, 64
    yield eng
    eng._ctx = None   # (nothing to close)


def good(width=3):
    f64 = lambda *shape, **kw: Fake(shape, "float64", **kw)  # noqa: E731
    return dict(values=f64(8, width), sums=f64(5, width), mins=f64(5, width), maxs=f64(5, width), counts=Fake((2,)))


def test_sums_refuse_cpu_tensors(engine):
    import torch
    for name, shape in (("values", (8, 3)), ("sums", (5, 3)), ("mins", (5, 3)), ("maxs", (5, 3))):
        args = good()
        args[name] = torch.zeros(shape, dtype=torch.float64)
        with pytest.raises(ValueError, match=name):
            engine.pairs_cluster_sums(**args)
    args = good()
    args["counts"] = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="counts"):
        engine.pairs_cluster_sums(**args)
    for name in ("values", "sums", "counts"):
        args = good()
        args[name] = None
        with pytest.raises(ValueError, match=name):
            engine.pairs_cluster_sums(**args)


@pytest.mark.parametrize("name,bad", [
    ("values", Fake((8, 3), "float32")), ("values", Fake((8, 0), "float64")), ("values", Fake((8, 9), "float64")),
    ("values", Fake((8, 3, 1), "float64")), ("values", Fake((8, 3), "float64", contiguous=False)),
    ("values", Fake((8, 3), "float64", index=1)), ("values", Fake((8, 3), "int64")),
    ("sums", Fake((5, 2), "float64")), ("sums", Fake((5,), "float64")), ("sums", Fake((5, 3), "float32")),
    ("sums", Fake((5, 3), "float64", index=1)), ("sums", Fake((5, 3), "float64", contiguous=False)),
    ("mins", Fake((4, 3), "float64")), ("mins", Fake((5, 2), "float64")), ("mins", Fake((5, 3), "int64")),
    ("maxs", Fake((6, 3), "float64")), ("maxs", Fake((5, 3), "float64", index=1)),
    ("counts", Fake((1,))), ("counts", Fake((2,), "int32")), ("counts", Fake((2, 1))), ("counts", Fake((2,), index=1)),
])
def test_sums_refuse_wrong_dtypes_shapes_and_devices(engine, name, bad):
    args = good()
    args[name] = bad
    with pytest.raises(ValueError, match=name):
        engine.pairs_cluster_sums(**args)


def test_sums_refuse_a_room_beyond_the_tensors(engine):
    with pytest.raises(ValueError, match="room_clusters"):
        engine.pairs_cluster_sums(**good(), room_clusters=6)
    args = good(1)
    args["values"] = Fake((8,), "float64")                                          # the façade takes (V, F) only
    with pytest.raises(ValueError, match="values"):
        engine.pairs_cluster_sums(**args)
