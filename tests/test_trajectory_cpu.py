"""CPU checks of the trajectory log: the cases of tests/trajectory_cases.py have the properties they are named for, proved
from the spec alone; the spec (tests/trajectory_spec.py) against frames written by hand; the wrappers' argument errors and
the refusals of the C ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import state_spec
import trajectory_cases as K
import trajectory_spec as T


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the spec against frames written by hand
def test_fill_is_one_quiet_nan_and_numpy_keeps_its_bits():
    assert T.FILL_BITS == 0x7FF8000000000000 and np.isnan(T.FILL)
    assert (bits(T.filled((3, 4))) == T.FILL_BITS).all()
    a = np.zeros(2)
    a[1] = T.FILL                                                    # an assignment copies the payload
    assert bits(a).tolist() == [0, T.FILL_BITS]
    from sand_crate_amd import trajectory
    assert trajectory.FILL_BITS == T.FILL_BITS and trajectory.MAX_ID == T.MAX_ID


def test_a_frame_by_hand():
    """Five slots in storage order, four stored, one of them with a NaN x; the window [10, 14) holds ids 10 and 13."""
    x = np.array([0.1, 0.2, np.nan, 0.4, 0.9])
    y = np.array([1.1, -0.0, 1.3, np.inf, 1.9])
    vx = np.array([2.1, 2.2, 2.3, np.nan, 2.9])
    vy = np.array([3.1, 3.2, 3.3, 3.4, 3.9])
    P = np.array([0.5, 0.6, 0.7, 0.8, 0.9])
    ids = np.array([13, 9, 11, 10, 12])
    states, press, count, outside = T.frame(x, y, vx, vy, P, ids, 4, 3, True, 10, 4)
    assert (count, outside) == (3, 1)                                # ids 13, 9, 10 are live; 9 lies outside
    want = T.filled((4, 4))
    want[0] = [0.4, np.inf, np.nan, 3.4]                             # id 10, slot 3
    want[3] = [0.1, 1.1, 2.1, 3.1]                                   # id 13, slot 0
    assert bits(states).tolist() == bits(want).tolist()
    assert np.signbit(T.frame(x, y, vx, vy, P, ids, 4, 3, True, 9, 1)[0][0, 1])   # id 9: y = -0.0 keeps its sign
    want_p = T.filled((4,))
    want_p[0] = 0.0                                                  # slot 3: the last tick left three slots live
    want_p[3] = 0.5
    assert bits(press).tolist() == bits(want_p).tolist()
    assert T.present(states).tolist() == [True, False, False, True]
    # without a valid pressure every present row shows zero
    assert bits(T.frame(x, y, vx, vy, P, ids, 4, 3, False, 10, 4)[1]).tolist() == bits([0.0, T.FILL, T.FILL, 0.0]).tolist()
    # the slot beyond the stored count is nobody
    assert T.frame(x, y, vx, vy, P, ids, 4, 3, True, 12, 1)[2:] == (3, 3)


def test_a_lost_id0_or_a_row_one_off_would_show():
    xy, vxy, ids = K.edge_state(257, K.EDGE_ID0, 64)
    export = state_spec.export(xy[:, 0], xy[:, 1], vxy[:, 0], vxy[:, 1], np.zeros(257), ids, 257, 0, False)
    right = T.frame_of_export(*export, K.EDGE_ID0, 64)
    assert T.present(right[0])[[0, -1]].all()                        # the first and the last row are taken ...
    assert not T.present(right[0]).all()                             # ... and some row in between is not
    for wrong in (T.frame_of_export(*export, 0, 64), T.frame_of_export(*export, K.EDGE_ID0 + 1, 64),
                  T.frame_of_export(*export, K.EDGE_ID0 - 1, 64)):
        assert bits(wrong[0]).tolist() != bits(right[0]).tolist()
        assert wrong[3] != right[3] or (T.present(wrong[0]) != T.present(right[0])).any()


def test_the_log_by_hand():
    log = T.Log(3, 0, 2)
    one = (np.array([[0.1, 0.2]]), np.array([[0.3, 0.4]]), np.array([0.5]), np.array([1]))
    assert [T.due(t, 3) for t in range(7)] == [True, False, False, True, False, False, True]
    log.take(0, one)
    log.take(1, one, abandoned=True)                                 # no frame, and not counted as dropped
    log.take(2, one)
    log.take(3, one)
    first = {k: np.copy(v) for k, v in log.read().items()}
    log.take(4, one)
    log.take(5, one)
    got = log.read()
    assert got["dropped"] == 2 and got["ticks"].tolist() == [0, 2, 3] and log.cursor == 3
    for name in ("states", "pressure", "ticks", "counts", "outside"):
        assert got[name].tobytes() == first[name].tobytes()          # the dropped frames touched nothing
    assert bits(got["states"][1]).tolist() == bits([[T.FILL] * 4, [0.1, 0.2, 0.3, 0.4]]).tolist()
    log.restart()
    assert log.read()["ticks"].tolist() == [] and log.read()["dropped"] == 0


# ---------------------------------------------------------------- the cases have their properties
@pytest.mark.parametrize("rows", K.ROWS)
def test_edge_windows_cut_ids_off_on_both_sides(rows):
    id0 = K.EDGE_ID0
    assert {1, K.WAVE - 1, K.WAVE, K.WAVE + 1, K.BLOCK - 1, K.BLOCK, K.BLOCK + 1} == set(K.ROWS)
    xy, vxy, ids = K.edge_state(257, id0, rows)
    assert len(set(ids.tolist())) == 257 and {id0 - 1, id0, id0 + rows - 1, id0 + rows} <= set(ids.tolist())
    assert (ids < id0).any() and (ids >= id0 + rows).any()
    assert ids.tolist() != sorted(ids.tolist())                      # storage order is not id order
    one = K.edge_ids(1, id0, rows)
    assert one.tolist() == [id0]                                     # a single live particle sits in row 0
    states, _, count, outside = T.frame_of_export(xy, vxy, np.zeros(257), ids, id0, rows)
    assert count == 257 and 0 < outside < 257 and T.present(states).sum() == 257 - outside
    assert len(K.odd_values()[0]) < K.WAVE < 257                     # more than one workgroup, a partial last wave


def test_top_window_passes_int32():
    xy, vxy, ids, (lo, hi) = K.top_state()
    assert hi == 2 ** 31 - 1 and ids.max() == 2 ** 31 - 2 == T.MAX_ID and lo - 1 in ids and lo in ids
    assert hi > np.iinfo(np.int32).max - 1 and lo + (hi - lo) == 2 ** 31 - 1   # id0 + rows: INT_MAX, one more wraps
    states, _, count, outside = T.frame_of_export(xy, vxy, np.zeros(len(ids)), ids, lo, hi - lo)
    assert T.present(states)[[0, -1]].all() and (count, outside) == (len(ids), 5)
    # a window's end taken in 32 bits as id0 + rows + 1, or a row index as id - id0 + 1, would wrap: the largest id's row
    assert int(ids.max()) - lo == hi - lo - 1 and lo + (hi - lo) + 1 > np.iinfo(np.int32).max


def test_wave_windows_give_every_count_of_outsiders():
    _, _, ids = K.wave_state()
    assert len(ids) == K.WAVE_COUNT == 2 * K.WAVE + 2
    per_wave = {w: K.outsiders_per_wave(ids, w) for w in K.WAVE_WINDOWS}
    assert per_wave[(0, 64)] == [0, 64, 2] and per_wave[(1, 65)] == [1, 63, 2]
    assert per_wave[(0, 130)] == [0, 0, 0] and per_wave[(64, 128)] == [64, 0, 2]
    full = {n for counts in per_wave.values() for n in counts[:2]}
    assert {0, 1, 63, 64} <= full
    for w, counts in per_wave.items():
        xy, vxy, _ = K.wave_state()
        assert T.frame_of_export(xy, vxy, np.zeros(len(ids)), ids, w[0], w[1] - w[0])[3] == sum(counts)


def test_odd_values_are_what_they_are_named_for():
    xy, vxy, live = K.odd_values()
    n = len(xy)
    out = state_spec.export(xy[:, 0], xy[:, 1], vxy[:, 0], vxy[:, 1], np.zeros(n), np.arange(n), n, 0, False)
    assert out[3].tolist() == np.flatnonzero(live).tolist() and 0 < live.sum() < n
    states = T.frame_of_export(*out, 0, n)[0]
    assert T.present(states).tolist() == live.tolist()
    kept = states[live]
    assert np.signbit(kept[kept == 0.0]).any() and np.isinf(kept[:, 1:]).any() and np.isnan(kept[:, 1:]).any()
    assert np.isnan(xy[~live, 0]).any() and np.isinf(xy[~live, 0]).any()
    assert (bits(states[~live]) == T.FILL_BITS).all()


def test_the_run_has_gaps_and_ids_on_both_sides_of_its_window():
    ids = K.run_on_oracle(K.RUN_TICKS)
    lo, hi = K.RUN_WINDOW
    assert len(ids) == K.RUN_TICKS
    assert any((i < lo).any() for i in ids[:3]) and (ids[-1] >= hi).any() and ((ids[-1] >= lo) & (ids[-1] < hi)).any()
    last = ids[-1]
    assert len(last) < last.max() + 1                                # gaps: ids are no ranks
    assert len(set(ids[4].tolist()) - set(ids[-1].tolist())) > 0     # particles leave while others stay
    assert all(len(i) > 0 for i in ids)


# ---------------------------------------------------------------- the wrappers' argument errors
def test_window_and_log_arguments():
    from sand_crate_amd.trajectory import check_log, check_window
    assert check_window(None, 3000) == (0, 3000) and check_window((5, 9), 1) == (5, 4)
    assert check_window((2 ** 31 - 258, 2 ** 31 - 1), 1) == (2 ** 31 - 258, 257)
    for bad in ((-1, 4), (4, 4), (5, 4), (0, 2 ** 31), (2 ** 31 - 1, 2 ** 31)):
        with pytest.raises(ValueError):
            check_window(bad, 1)
    with pytest.raises(ValueError):
        check_window(None, 0)
    assert check_log(3, 1) == (3, 1)
    for bad in ((0, 1), (-2, 1), (3, 0), (3, -1)):
        with pytest.raises(ValueError):
            check_log(*bad)


def test_tensor_checks_come_before_the_library():
    """`Engine.traj_enable` on an engine that has no library and no context: every bad tensor is a ValueError."""
    import torch
    from sand_crate_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.device = 0
    f64, i64 = torch.float64, torch.int64
    good = dict(states=torch.zeros((3, 5, 4), dtype=f64), pressure=None, ticks=torch.zeros(3, dtype=i64),
                counts=torch.zeros(3, dtype=i64), outside=torch.zeros(3, dtype=i64), words=torch.zeros(4, dtype=i64))
    bad = [dict(good), dict(good, states=torch.zeros((3, 5, 3), dtype=f64)), dict(good, states=torch.zeros((0, 5, 4), dtype=f64)),
           dict(good, states=torch.zeros((3, 0, 4), dtype=f64)), dict(good, states=np.zeros((3, 5, 4))),
           dict(good, states=torch.zeros((3, 5, 4), dtype=torch.float32)), dict(good, ticks=torch.zeros(4, dtype=i64)),
           dict(good, words=torch.zeros(3, dtype=i64)), dict(good, pressure=torch.zeros((3, 4), dtype=f64))]
    for tensors in bad:                                              # (CPU tensors: the first one is refused as well)
        with pytest.raises(ValueError):
            eng.traj_enable(tensors["states"], tensors["pressure"], tensors["ticks"], tensors["counts"], tensors["outside"],
                            tensors["words"], id0=0)
    eng._ctx = None                                                  # (nothing to destroy)
    eng._lib = None


def test_a_stopped_recording_refuses_and_reads():
    import torch
    from sand_crate_amd.trajectory import Trajectory, complete_rows, present
    t = Trajectory.__new__(Trajectory)
    t._engine = None
    assert not t.recording
    for call in (t.capture, t.restart):
        with pytest.raises(RuntimeError):
            call()
    t.stop()                                                         # (stopped twice is fine)
    states = torch.tensor(np.stack([T.filled((3, 4)), T.filled((3, 4))]))
    states[0, 0] = torch.tensor([0.1, 0.2, 0.3, 0.4], dtype=torch.float64)
    states[1, 0] = torch.tensor([0.1, float("nan"), 0.3, float("inf")], dtype=torch.float64)
    states[1, 2] = 1.0
    assert present(states).tolist() == [[True, False, False], [True, False, True]]
    assert complete_rows(states).tolist() == [0]


# ---------------------------------------------------------------- the ABI's refusals that need no device
@pytest.fixture(scope="module")
def lib():
    from sand_crate_amd import _native as N, build
    build.build()
    return N.load()


def test_null_contexts_are_refused(lib):
    from sand_crate_amd import _native as N
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    assert lib.sc_traj_enable_device(None, p, None, p, p, p, p, 2, 0, 2, 1, 1) == N.ERR_ARG
    assert b"null context" in lib.sc_last_error()
    assert lib.sc_traj_capture(None) == N.ERR_ARG and lib.sc_traj_disable(None) == N.ERR_ARG


def test_driver_has_the_option():
    from sand_crate_amd.main import argument_parser
    ap = argument_parser()
    assert ap.parse_args(["c.yaml"]).trajectory == 0
    assert ap.parse_args(["c.yaml", "--trajectory"]).trajectory == 1
    assert ap.parse_args(["c.yaml", "--trajectory", "5"]).trajectory == 5
