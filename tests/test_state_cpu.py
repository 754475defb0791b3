"""CPU-side checks of the device state exchange: the export's rule (tests/state_spec.py) on hand-made storage arrays, the
two symbols in the header and the ctypes table, and the tensor checks of `Engine.export_state` / `Engine.import_state`,
which refuse before the library is touched.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import state_spec as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sandcrate_hip.h"


# ---- the rule

def test_spec_orders_by_id_over_gaps():
    x = np.array([0.5, 0.1, 0.9, 0.3, 0.7])
    y = x + 10
    vx, vy = x + 20, x + 30
    P = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    ids = np.array([40, 7, 1000, 0, 33])
    p, v, pr, i = S.export(x, y, vx, vy, P, ids, 5, 5, True)
    assert i.tolist() == [0, 7, 33, 40, 1000] and i.dtype == np.int64
    assert p.tolist() == [[0.3, 10.3], [0.1, 10.1], [0.7, 10.7], [0.5, 10.5], [0.9, 10.9]]
    assert v[:, 0].tolist() == [20.3, 20.1, 20.7, 20.5, 20.9] and v[:, 1].tolist() == [30.3, 30.1, 30.7, 30.5, 30.9]
    assert pr.tolist() == [4.0, 2.0, 5.0, 1.0, 3.0]
    # slots past n_stored are not the state
    p, v, pr, i = S.export(x, y, vx, vy, P, ids, 3, 3, True)
    assert i.tolist() == [7, 40, 1000] and pr.tolist() == [2.0, 1.0, 3.0]
    p, v, pr, i = S.export(x, y, vx, vy, P, ids, 0, 0, True)
    assert p.shape == v.shape == (0, 2) and pr.shape == i.shape == (0,)


def test_spec_skips_slots_whose_x_is_not_finite():
    x = np.array([0.5, np.inf, 0.9, np.nan, -np.inf, 0.2])
    y = np.array([1.0, 2.0, np.inf, 4.0, 5.0, np.nan])          # (only x decides)
    z = np.zeros(6)
    ids = np.array([5, 4, 3, 2, 1, 0])
    p, v, pr, i = S.export(x, y, z, z, z, ids, 6, 6, True)
    assert i.tolist() == [0, 3, 5]
    assert p[:, 0].tolist() == [0.2, 0.9, 0.5] and np.isnan(p[0, 1]) and np.isinf(p[1, 1])


def test_spec_pressure_is_valid_for_the_ticked_slots_only():
    x = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    z = np.zeros(5)
    P = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    ids = np.array([4, 3, 2, 1, 0])
    # the last tick left three slots live, two particles were appended since: their slots carry no pressure
    assert S.export(x, z, z, z, P, ids, 5, 3, True)[2].tolist() == [0.0, 0.0, 3.0, 2.0, 1.0]
    # ... the tick left more live than are stored now: the stored count bounds it
    assert S.export(x, z, z, z, P, ids, 4, 5, True)[2].tolist() == [4.0, 3.0, 2.0, 1.0]
    # ... after an upload no pressure is valid
    assert S.export(x, z, z, z, P, ids, 5, 5, False)[2].tolist() == [0.0] * 5
    # a pressure array shorter than the storage (the boundary lies inside it) is never read past the boundary
    assert S.export(x, z, z, z, P[:3], ids, 5, 3, True)[2].tolist() == [0.0, 0.0, 3.0, 2.0, 1.0]


# ---- the boundary

def declaration(name):
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    found = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert found, f"{name} is not declared in the header"
    return [a.strip() for a in found.group(1).split(",")]


@pytest.mark.parametrize("name,n_args", [("sc_export_state_device", 7), ("sc_import_state_device", 5)])
def test_symbols_are_declared_and_bound(name, n_args):
    import ctypes as C
    from sand_crate_amd import _native as N
    args = declaration(name)
    assert len(args) == n_args and args[0].startswith("sc_ctx*")
    assert name in N.SIGNATURES
    res, argtypes = N.SIGNATURES[name]
    assert res is C.c_int and len(argtypes) == n_args
    assert argtypes[-1 if name == "sc_import_state_device" else -2] is C.c_int64     # n / room
    assert N.STATE_TILE > 0 and N.STATE_SCAN_BLOCK > 0 and N.STATE_GATHER_BLOCK > 0


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


def good():
    return dict(particles=Fake((8, 2)), velocities=Fake((8, 2)), pressure=Fake((8,)), ids=Fake((8,), "int64"),
                count=Fake((1,), "int64"))


def test_export_refuses_cpu_tensors(engine):
    import torch
    cpu = dict(particles=torch.zeros((8, 2), dtype=torch.float64), velocities=torch.zeros((8, 2), dtype=torch.float64),
               pressure=torch.zeros(8, dtype=torch.float64), ids=torch.zeros(8, dtype=torch.int64),
               count=torch.zeros(1, dtype=torch.int64))
    for name in cpu:
        args = good()
        args[name] = cpu[name]
        with pytest.raises(ValueError, match=name):
            engine.export_state(**args)
    with pytest.raises(ValueError, match="count"):
        engine.export_state(Fake((8, 2)), count=None)
    with pytest.raises(ValueError):
        engine.export_state(np.zeros((8, 2)), count=Fake((1,), "int64"))


@pytest.mark.parametrize("name,bad", [
    ("particles", Fake((8, 2), "float32")), ("particles", Fake((8, 3))), ("particles", Fake((16,))),
    ("particles", Fake((8, 2), contiguous=False)), ("particles", Fake((8, 2), index=1)),
    ("velocities", Fake((7, 2))), ("velocities", Fake((8, 2), "int64")),
    ("pressure", Fake((8, 1))), ("pressure", Fake((9,))), ("pressure", Fake((8,), "float32")),
    ("ids", Fake((8,), "int32")), ("ids", Fake((8,), "float64")), ("ids", Fake((8, 2), "int64")),
    ("count", Fake((1,), "int32")), ("count", Fake((2,), "int64")), ("count", Fake((), "int64")), ("count", Fake((1, 1), "int64")),
])
def test_export_refuses_wrong_dtypes_and_shapes(engine, name, bad):
    args = good()
    args[name] = bad
    with pytest.raises(ValueError, match=name):
        engine.export_state(**args)


def test_export_refuses_more_room_than_rows(engine):
    with pytest.raises(ValueError, match="room"):
        engine.export_state(**good(), room=9)


def test_import_refuses_cpu_tensors_wrong_dtypes_and_shapes(engine):
    import torch
    p, v = Fake((8, 2)), Fake((8, 2))
    cpu = torch.zeros((8, 2), dtype=torch.float64)
    for args, name in (((cpu, v), "particles"), ((p, cpu), "velocities"), ((p, v, torch.zeros(8, dtype=torch.int64)), "ids"),
                       ((np.zeros((8, 2)), v), "particles"),
                       ((Fake((8, 2), "float32"), v), "particles"), ((Fake((8,)), v), "particles"), ((Fake((8, 3)), v), "particles"),
                       ((p, Fake((9, 2))), "velocities"), ((p, Fake((8, 2), contiguous=False)), "velocities"),
                       ((p, Fake((8, 2), index=1)), "velocities"),
                       ((p, v, Fake((8,), "int32")), "ids"), ((p, v, Fake((7,), "int64")), "ids"), ((p, v, Fake((8, 1), "int64")), "ids")):
        with pytest.raises(ValueError, match=name):
            engine.import_state(*args)
