"""CPU-side checks of the device pair search: the rule (tests/pairs_spec.py) on hand-made inputs, the two symbols in the
header and the ctypes table, the torch helpers of sand_crate_amd/pairs.py, and the tensor checks of `Engine.pairs_count` /
`Engine.pairs_fill`, which refuse before the library is touched.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import pairs_spec as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sandcrate_hip.h"


# ---- the rule

def test_spec_on_a_hand_made_line():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [2.5, 0.0], [10.0, 0.0]])
    offsets, partners, d2 = S.pairs(pts, 1.0)
    assert offsets.dtype == partners.dtype == np.int64 and d2.dtype == np.float64
    assert offsets.tolist() == [0, 1, 3, 5, 6, 6]
    assert partners.tolist() == [1, 0, 2, 1, 3, 2]
    rows = [partners[offsets[i]:offsets[i + 1]].tolist() for i in range(5)]
    assert rows == [[1], [0, 2], [1, 3], [2], []]
    assert d2.tolist() == [1.0, 1.0, 1.0, 1.0, 0.25, 0.25]


def test_spec_half_keeps_j_above_i():
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [2.5, 0.0], [10.0, 0.0]])
    offsets, partners, d2 = S.pairs(pts, 1.5, half=True)
    rows = [partners[offsets[i]:offsets[i + 1]].tolist() for i in range(5)]
    assert rows == [[1], [2, 3], [3], [], []]
    assert d2.tolist() == [1.0, 1.0, 2.25, 0.25]
    full = S.pairs(pts, 1.5)
    assert full[0][-1] == 2 * offsets[-1]


def test_spec_coincident_and_non_finite_points():
    pts = np.array([[0.5, 0.5], [np.nan, 0.5], [0.5, 0.5], [0.5, np.inf], [-np.inf, np.nan], [0.5, 0.5]])
    offsets, partners, d2 = S.pairs(pts, 1e-3)
    rows = [partners[offsets[i]:offsets[i + 1]].tolist() for i in range(6)]
    assert rows == [[2, 5], [], [0, 5], [], [], [0, 2]]
    assert d2.tolist() == [0.0] * 6
    offsets, partners, d2 = S.pairs(np.zeros((0, 2)), 1.0)
    assert offsets.tolist() == [0] and partners.shape == d2.shape == (0,)
    assert S.pairs(np.array([[1.0, 2.0]]), 1.0)[0].tolist() == [0, 0]


def test_spec_row_blocks_do_not_show():
    rs = np.random.RandomState(1)
    pts = rs.rand(S.BLOCK + 37, 2)
    a = S.pairs(pts, 0.05)
    saved, S.BLOCK = S.BLOCK, 50
    try:
        b = S.pairs(pts, 0.05)
    finally:
        S.BLOCK = saved
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    j = a[1]
    i = np.repeat(np.arange(len(pts)), np.diff(a[0]))
    assert len(j) > 1000 and (i != j).all()
    assert set(zip(i.tolist(), j.tolist())) == set(zip(j.tolist(), i.tolist()))   # symmetric


def test_spec_domain():
    assert S.in_domain(np.array([[1.0, -2.0]]), 1e-9)
    assert not S.in_domain(np.array([[1.0, -2.0]]), 1e-10)
    assert not S.in_domain(np.array([[np.nan, 2.0 ** 31]]), 1.0)
    assert S.in_domain(np.array([[np.nan, np.nextafter(2.0 ** 31, 0)]]), 1.0)


# ---- the boundary

def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert found, f"{name} is not declared in the header"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("sc_pairs_count_device", 8), ("sc_pairs_fill_device", 4)])
def test_symbols_are_declared_and_bound(name, n_args):
    import ctypes as C
    from sand_crate_amd import _native as N
    args = declaration(name)
    assert len(args) == n_args and args[0].startswith("sc_ctx*")
    assert name in N.SIGNATURES
    res, argtypes = N.SIGNATURES[name]
    assert res is C.c_int and len(argtypes) == n_args
    if name == "sc_pairs_count_device":
        assert argtypes[2] is C.c_int64 and argtypes[3] is C.c_double and argtypes[4] is C.c_int32 and argtypes[6] is C.c_int64
    else:
        assert argtypes[3] is C.c_int64
    assert N.PAIRS_BLOCK > 0 and N.PAIRS_SORT_TILE > 0 and N.PAIRS_SCAN_BLOCK > 0 and N.PAIRS_HALF == 1


def test_constants_mirror_the_kernels():
    from sand_crate_amd import _native as N
    text = (ROOT / "sand_crate_amd" / "csrc" / "sc_pairs.h").read_text()

    def constant(name):
        return re.search(r"\b" + name + r"\s*=\s*([^,;]+)", text).group(1).strip()

    assert int(constant("kPairsLoad")) == N.PAIRS_LOAD and int(constant("kPairsMinBuckets")) == N.PAIRS_MIN_BUCKETS
    assert int(constant("kPairsHashX").rstrip("u"), 16) == N.PAIRS_HASH_X
    assert int(constant("kPairsHashY").rstrip("u"), 16) == N.PAIRS_HASH_Y
    assert int(constant("kPairsHashMix").rstrip("u"), 16) == N.PAIRS_HASH_MIX
    assert constant("kPairsCellFactor") == "1.0 + 1.0 / 1048576.0" and N.PAIRS_CELL_FACTOR == 1.0 + 1.0 / 1048576.0
    text = (ROOT / "sand_crate_amd" / "csrc" / "sc_radix.h").read_text()     # the sort both the export and the search run
    assert int(constant("kRadixTile")) == N.STATE_TILE == N.PAIRS_SORT_TILE
    header = HEADER.read_text()
    assert re.search(r"SC_PAIRS_HALF\s*=\s*1\b", header)
    assert re.search(r"#define SC_ABI_VERSION 5\b", header) and re.search(r"#define SC_NUM_KERNELS 12\b", header)


# ---- the torch helpers

def test_edge_index_and_row_lengths():
    import torch
    from sand_crate_amd import pairs
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0], [2.5, 0.0], [10.0, 0.0]])
    offsets, partners, _ = S.pairs(pts, 1.0)
    o, p = torch.from_numpy(offsets), torch.from_numpy(partners)
    assert pairs.row_lengths(o).tolist() == [1, 2, 2, 1, 0]
    e = pairs.edge_index(o, p)
    assert e.dtype == torch.int64 and e.shape == (2, 6)
    assert e.tolist() == [[0, 1, 1, 2, 2, 3], [1, 0, 2, 1, 3, 2]]
    assert pairs.edge_index(o, p[:4]).tolist() == [[0, 1, 1, 2], [1, 0, 2, 1]]          # a clipped list
    empty = pairs.edge_index(torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))
    assert empty.shape == (2, 0)


# ---- tensors are checked before the library is touched

class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"the library was touched ({name})")


class Fake:
    """What the checks look at of a CUDA tensor, without a GPU."""

    def __init__(self, shape, dtype="float64", contiguous=True, index=0):
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


def good_count():
    return dict(points=Fake((8, 2)), offsets=Fake((9,), "int64"), counts=Fake((2,), "int64"))


def good_fill():
    return dict(partners=Fake((30,), "int64"), d2=Fake((30,)))


def test_count_refuses_cpu_tensors(engine):
    import torch
    cpu = dict(points=torch.zeros((8, 2), dtype=torch.float64), offsets=torch.zeros(9, dtype=torch.int64),
               counts=torch.zeros(2, dtype=torch.int64))
    for name in cpu:
        args = good_count()
        args[name] = cpu[name]
        with pytest.raises(ValueError, match=name):
            engine.pairs_count(radius=0.1, **args)
    with pytest.raises(ValueError, match="points"):
        engine.pairs_count(np.zeros((8, 2)), radius=0.1, offsets=Fake((9,), "int64"), counts=Fake((2,), "int64"))
    with pytest.raises(ValueError, match="offsets"):
        engine.pairs_count(None, radius=0.1, offsets=None, counts=Fake((2,), "int64"))
    with pytest.raises(ValueError, match="counts"):
        engine.pairs_count(None, radius=0.1, offsets=Fake((9,), "int64"), counts=None)


@pytest.mark.parametrize("name,bad", [
    ("points", Fake((8, 2), "float32")), ("points", Fake((8, 3))), ("points", Fake((16,))),
    ("points", Fake((8, 2), contiguous=False)), ("points", Fake((8, 2), index=1)),
    ("offsets", Fake((9,), "int32")), ("offsets", Fake((9, 1), "int64")), ("offsets", Fake((9,), "float64")),
    ("offsets", Fake((0,), "int64")), ("offsets", Fake((9,), "int64", index=1)), ("offsets", Fake((9,), "int64", contiguous=False)),
    ("counts", Fake((1,), "int64")), ("counts", Fake((2,), "int32")), ("counts", Fake((2, 1), "int64")), ("counts", Fake((), "int64")),
    ("counts", Fake((2,), "int64", index=1)),
])
def test_count_refuses_wrong_dtypes_shapes_and_devices(engine, name, bad):
    args = good_count()
    args[name] = bad
    with pytest.raises(ValueError, match=name):
        engine.pairs_count(radius=0.1, **args)


def test_count_refuses_room_and_radius(engine):
    with pytest.raises(ValueError, match="room"):
        engine.pairs_count(radius=0.1, room=9, **good_count())
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="radius"):
            engine.pairs_count(radius=radius, **good_count())


def test_fill_refuses_cpu_tensors_wrong_dtypes_shapes_and_devices(engine):
    import torch
    cpu = dict(partners=torch.zeros(30, dtype=torch.int64), d2=torch.zeros(30, dtype=torch.float64))
    bad = [("partners", cpu["partners"]), ("d2", cpu["d2"]), ("partners", np.zeros(30, dtype=np.int64)),
           ("partners", Fake((30,), "int32")), ("partners", Fake((30, 1), "int64")), ("partners", Fake((30,), "int64", index=1)),
           ("partners", Fake((30,), "int64", contiguous=False)),
           ("d2", Fake((30,), "float32")), ("d2", Fake((29,))), ("d2", Fake((30, 1))), ("d2", Fake((30,), index=1)),
           ("d2", Fake((30,), "int64"))]
    for name, tensor in bad:
        args = good_fill()
        args[name] = tensor
        with pytest.raises(ValueError, match=name):
            engine.pairs_fill(**args)
    with pytest.raises(ValueError, match="room"):
        engine.pairs_fill(**good_fill(), room=31)
