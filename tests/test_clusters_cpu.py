"""CPU-side checks of the device cluster labelling: the rule (tests/cluster_spec.py) on hand-made inputs, the symbol in the
header, the ctypes table and the built library, the argument error that is checked before any HIP call, the torch helpers
of sand_crate_amd/pairs.py, and the tensor checks of `Engine.pairs_label`, which refuse before the library is touched.
No GPU."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest

import cluster_spec as CS
import pairs_spec as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sandcrate_hip.h"


# ---- the rule

LINE = np.array([[2.5, 0.0], [10.0, 0.0], [2.0, 0.0], [np.nan, 0.0], [1.0, 0.0], [0.0, 0.0], [10.5, np.inf], [10.5, 0.0]])


def test_spec_on_a_hand_made_line():
    labels, sizes, roots = CS.clusters(LINE, 1.0)
    assert labels.dtype == sizes.dtype == roots.dtype == np.int64
    assert labels.tolist() == [0, 1, 0, -1, 0, 0, -1, 1] and sizes.tolist() == [4, 2] and roots.tolist() == [0, 1]
    labels, sizes, roots = CS.clusters(LINE, 0.75)                                  # 2.5 - 2.0 and 10.5 - 10.0 only
    assert labels.tolist() == [0, 1, 0, -1, 2, 3, -1, 1] and sizes.tolist() == [2, 2, 1, 1] and roots.tolist() == [0, 1, 4, 5]


def test_spec_components_from_a_list_half_or_full():
    alive = np.isfinite(LINE).all(axis=1)
    want = CS.clusters(LINE, 1.0)
    for half in (False, True):
        offsets, partners, _ = S.pairs(LINE, 1.0, half)
        for g, w in zip(CS.components(len(LINE), offsets, partners, alive=alive), want):
            assert g.dtype == np.int64 and np.array_equal(g, w)
    # without `alive` every node is in a cluster: the two that are not finite are singletons
    offsets, partners, _ = S.pairs(LINE, 1.0)
    labels, sizes, roots = CS.components(len(LINE), offsets, partners)
    assert labels.tolist() == [0, 1, 0, 2, 0, 0, 3, 1] and sizes.tolist() == [4, 2, 1, 1] and roots.tolist() == [0, 1, 3, 6]


def test_spec_of_nothing_and_of_one():
    for got in (CS.clusters(np.zeros((0, 2)), 1.0), CS.components(0, np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64))):
        assert [a.shape for a in got] == [(0,)] * 3 and all(a.dtype == np.int64 for a in got)
    assert [a.tolist() for a in CS.clusters(np.array([[1.0, 2.0]]), 1.0)] == [[0], [1], [0]]
    assert [a.tolist() for a in CS.clusters(np.array([[1.0, -np.inf]]), 1.0)] == [[-1], [], []]


def test_spec_a_long_chain_in_the_worst_order():
    n = 3000
    k = np.arange(n)
    order = np.concatenate([k[::2], k[1::2][::-1]])                                 # neighbours on the line far apart in index
    pts = np.zeros((n, 2))
    pts[order, 0] = 0.5 * k
    labels, sizes, roots = CS.clusters(pts, 0.5)
    assert not labels.any() and sizes.tolist() == [n] and roots.tolist() == [0]
    offsets, partners, _ = S.pairs(pts, 0.5, half=True)
    assert offsets[-1] == n - 1
    assert [a.tolist() for a in CS.components(n, offsets, partners)] == [[0] * n, [n], [0]]


# ---- the boundary

def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert found, f"{name} is not declared in the header"
    return [" ".join(a.split()) for a in found.group(1).split(",")]


def test_symbol_is_declared_and_the_versions_stay():
    args = declaration("sc_pairs_label_device")
    assert args == ["sc_ctx* ctx", "int64_t* dev_labels", "int64_t room_rows", "int64_t* dev_sizes", "int64_t* dev_roots",
                    "int64_t room_clusters", "int64_t* dev_counts"]
    header = HEADER.read_text()
    assert re.search(r"#define SC_ABI_VERSION 5\b", header) and re.search(r"#define SC_NUM_KERNELS 12\b", header)
    from sand_crate_amd import _native as N
    assert N.NUM_KERNELS == 12


def test_ctypes_table_matches_the_header():
    import ctypes as C
    from sand_crate_amd import _native as N
    res, argtypes = N.SIGNATURES["sc_pairs_label_device"]
    kinds = {"sc_ctx*": C.c_void_p, "int64_t*": C.c_void_p, "int64_t": C.c_int64}  # (device addresses travel as void*)
    want = [kinds[a.rsplit(" ", 1)[0]] for a in declaration("sc_pairs_label_device")]
    assert res is C.c_int and argtypes == want


def test_kernels_are_included_once_after_the_pairs():
    text = (ROOT / "sand_crate_amd" / "csrc" / "sandcrate_hip.hip").read_text()
    assert text.count('#include "sc_clusters.h"') == 1
    assert text.index('#include "sc_pairs.h"') < text.index('#include "sc_clusters.h"')


def test_library_exports_the_call_and_refuses_a_null_context():
    import ctypes
    from sand_crate_amd import _native as N, build
    lib = ctypes.CDLL(str(build.build()))
    fn = lib.sc_pairs_label_device
    fn.restype, fn.argtypes = N.SIGNATURES["sc_pairs_label_device"]
    lib.sc_last_error.restype = ctypes.c_char_p
    assert fn(None, None, 0, None, None, 0, None) == N.ERR_ARG                      # before any HIP call: no GPU needed
    assert b"null context" in lib.sc_last_error()
    assert lib.sc_abi_version() == 5


def test_python_surface():
    from sand_crate_amd import Crate
    from sand_crate_amd.engine import Engine
    p = inspect.signature(Engine.pairs_label).parameters
    assert list(p) == ["self", "labels", "sizes", "roots", "counts", "room", "room_clusters"]
    assert p["sizes"].default is None and p["roots"].default is None and p["room"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("counts", "room", "room_clusters"))
    p = inspect.signature(Crate.cluster_tensors).parameters
    assert list(p) == ["self", "radius", "points", "max_clusters"] and p["radius"].default is None
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("points", "max_clusters"))


# ---- the torch helpers

def test_cluster_size_of_and_largest_cluster():
    import torch
    from sand_crate_amd import pairs
    labels, sizes, _ = (torch.from_numpy(a) for a in CS.clusters(LINE, 0.75))
    got = pairs.cluster_size_of(labels, sizes)
    assert got.dtype == torch.int64 and got.tolist() == [2, 2, 2, 0, 1, 1, 0, 2]
    assert pairs.largest_cluster(sizes) == (0, 2)                                   # the first of equals
    assert pairs.largest_cluster(torch.tensor([1, 7, 3])) == (1, 7)
    none = torch.zeros(0, dtype=torch.int64)
    assert pairs.largest_cluster(none) == (-1, 0)
    assert pairs.cluster_size_of(torch.tensor([-1, -1]), none).tolist() == [0, 0]
    assert pairs.cluster_size_of(none, none).shape == (0,)


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
    return dict(labels=Fake((8,)), sizes=Fake((5,)), roots=Fake((5,)), counts=Fake((2,)))


def test_label_refuses_cpu_tensors(engine):
    import torch
    for name, rows in (("labels", 8), ("sizes", 5), ("roots", 5), ("counts", 2)):
        args = good()
        args[name] = torch.zeros(rows, dtype=torch.int64)
        with pytest.raises(ValueError, match=name):
            engine.pairs_label(**args)
    for name in ("labels", "counts"):
        args = good()
        args[name] = None
        with pytest.raises(ValueError, match=name):
            engine.pairs_label(**args)
    with pytest.raises(ValueError, match="labels"):
        engine.pairs_label(np.zeros(8, dtype=np.int64), counts=Fake((2,)))


@pytest.mark.parametrize("name,bad", [
    ("labels", Fake((8,), "int32")), ("labels", Fake((8, 1))), ("labels", Fake((8,), "float64")),
    ("labels", Fake((8,), contiguous=False)), ("labels", Fake((8,), index=1)),
    ("sizes", Fake((5,), "int32")), ("sizes", Fake((5, 1))), ("sizes", Fake((5,), index=1)), ("sizes", Fake((5,), contiguous=False)),
    ("roots", Fake((4,))), ("roots", Fake((5,), "float64")), ("roots", Fake((5,), index=1)),
    ("counts", Fake((1,))), ("counts", Fake((2,), "int32")), ("counts", Fake((2, 1))), ("counts", Fake(())),
    ("counts", Fake((2,), index=1)),
])
def test_label_refuses_wrong_dtypes_shapes_and_devices(engine, name, bad):
    args = good()
    args[name] = bad
    with pytest.raises(ValueError, match=name):
        engine.pairs_label(**args)


def test_label_refuses_rooms_beyond_the_tensors(engine):
    with pytest.raises(ValueError, match="room"):
        engine.pairs_label(**good(), room=9)
    with pytest.raises(ValueError, match="room_clusters"):
        engine.pairs_label(**good(), room_clusters=6)
    with pytest.raises(ValueError, match="room_clusters"):
        engine.pairs_label(Fake((8,)), counts=Fake((2,)), room_clusters=1)          # no sizes, no roots: no room
