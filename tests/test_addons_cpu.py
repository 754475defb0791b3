"""The add-ons of `Crate` (sand_crate_amd/addons.py) and the rule that moves them to the context a crate grows into --
`leave(old_engine)`, then `enter(new_engine)` -- by behaviour, against engines that write down what they are asked.  No
GPU.  (The overlay's half of the rule: tests/test_arrows_cpu.py, test_grow_forgets_what_was_sent.)"""
import numpy as np
import pytest

import track_spec
from sand_crate_amd import Crate, probe
from sand_crate_amd.addons import FRAMES, OBSERVABLES, AddOn, DeviceLog, Overlay, PendingCheckpoint
from sand_crate_amd.trajectory import Trajectory


def observables_log() -> DeviceLog:
    return DeviceLog(*OBSERVABLES)


def frame_log() -> DeviceLog:
    return DeviceLog(*FRAMES)


def frame(tick: int) -> bytes:
    return track_spec.pack(tick, np.full((2, 2), 0.5), np.zeros(2), np.arange(2), np.zeros((0, 2, 2)))


def rows(ticks, bins: int, dropped: int):
    """A chunk of `Engine.probe_read`: the rows of these ticks, profiles of `bins` bins, `dropped`."""
    r = np.zeros((len(ticks), len(probe.FIELDS)))
    r[:, 0] = ticks
    return r, np.full((len(ticks), bins), 7, dtype=np.int32), np.full((len(ticks), bins), 0.25), dropped


class Recorder:
    """An engine that writes down every call of the logs and of a checkpoint, and answers the reads from a script."""

    def __init__(self, probe_chunks=(), track_chunks=(), refuse=False):
        self.calls, self.refuse = [], refuse
        self.probe_chunks, self.track_chunks = list(probe_chunks), list(track_chunks)

    def _enable(self, name, settings):
        self.calls.append((name, *settings))
        if self.refuse:
            raise ValueError("refused")

    def probe_enable(self, *settings):
        self._enable("probe_enable", settings)

    def track_enable(self, *settings):
        self._enable("track_enable", settings)

    def probe_disable(self):
        self.calls.append(("probe_disable",))

    def track_disable(self):
        self.calls.append(("track_disable",))

    def probe_read(self):
        self.calls.append(("probe_read",))
        return self.probe_chunks.pop(0)

    def track_read(self):
        self.calls.append(("track_read",))
        frames, dropped = self.track_chunks.pop(0)
        return b"".join(frames), len(frames), dropped

    def checkpoint_finish(self):
        self.calls.append(("checkpoint_finish",))
        return {"tick": 5}


def move(addons, old, new):
    """The two loops of `Crate._grow`."""
    for addon in addons:
        addon.leave(old)
    for addon in addons:
        addon.enter(new)


def half_crate(engine):
    crate = object.__new__(Crate)  # (no GPU context: only what the logs touch)
    crate._engine, crate._observed, crate._tracked = engine, observables_log(), frame_log()
    return crate


def test_every_add_on_speaks_the_protocol():
    for kind in (Overlay, DeviceLog, PendingCheckpoint, Trajectory):
        assert callable(kind.leave) and callable(kind.enter)
    AddOn().leave(None)
    AddOn().enter(None)


def test_logs_that_are_on_move_with_their_settings_and_keep_what_the_old_context_held():
    old = Recorder([rows([1, 2], 3, dropped=2)], [([frame(2)], 1)])
    new = Recorder([rows([3], 3, dropped=1)], [([frame(4), frame(6)], 4)])
    crate = half_crate(old)
    crate.observe(capacity=8, bins=3, x_range=(0, 2))
    crate.track(every=2, capacity_bytes=4096)
    assert old.calls == [("probe_enable", 8, 3, 0.0, 2.0), ("track_enable", 2, 4096)]
    del old.calls[:]
    move([crate._observed, crate._tracked], old, new)
    crate._engine = new
    assert old.calls == [("probe_read",), ("track_read",)]       # each read once, and never switched off
    assert new.calls == [("probe_enable", 8, 3, 0.0, 2.0), ("track_enable", 2, 4096)]
    assert crate._observed.settings == (8, 3, 0.0, 2.0) and crate._tracked.settings == (2, 4096)
    got = crate.observations()
    assert got["tick"].tolist() == [1.0, 2.0, 3.0] and got["dropped"] == 3 and got["count"].shape == (3, 3)
    assert crate.tracked() == ([frame(2), frame(4), frame(6)], 5)
    assert old.calls == [("probe_read",), ("track_read",)] and new.calls[2:] == [("probe_read",), ("track_read",)]
    assert crate._observed.chunks == [] and crate._tracked.chunks == []


def test_take_returns_the_chunks_in_order_and_empties_the_log():
    old, new = Recorder([rows([1], 0, 2)]), Recorder([rows([2], 0, 1)])
    log = observables_log()
    log.switch(old, True, (4, 0, 0.0, 1.0))
    move([log], old, new)
    first, second = log.take(new)
    assert (first[0][:, 0].tolist(), first[3], second[0][:, 0].tolist(), second[3]) == ([1.0], 2, [2.0], 1)
    assert log.chunks == [] and log.settings == (4, 0, 0.0, 1.0)


def test_logs_that_are_off_touch_neither_engine():
    old, new = Recorder(), Recorder()
    crate = half_crate(old)
    move([crate._observed, crate._tracked], old, new)
    crate._engine = new
    assert crate.observations()["dropped"] == 0 and crate.tracked() == ([], 0)
    assert old.calls == [] and new.calls == []


def test_a_pending_checkpoint_collects_its_snapshot_from_the_old_context_once():
    old, new, newer = Recorder(), Recorder(), Recorder()
    pending = PendingCheckpoint()
    move([pending], old, new)                                    # none under way
    assert old.calls == [] and new.calls == []
    pending.meta = {"tick": 5}
    move([pending], old, new)
    assert old.calls == [("checkpoint_finish",)] and new.calls == [] and pending.snapshot == {"tick": 5}
    move([pending], new, newer)                                  # it has its snapshot: a second growth collects nothing
    assert old.calls == [("checkpoint_finish",)] and new.calls == [] and newer.calls == []
    assert pending.finish(newer) == ({"tick": 5}, {"tick": 5}) and newer.calls == []
    assert pending.meta is None and pending.snapshot is None
    pending.meta = {"tick": 6}                                   # without a growth the context that took it delivers
    assert pending.finish(newer) == ({"tick": 6}, {"tick": 5}) and newer.calls == [("checkpoint_finish",)]


@pytest.mark.parametrize("make, name, first, second", [(observables_log, "probe", (4, 0, 0.0, 1.0), (9, 2, 0.0, 0.5)),
                                                       (frame_log, "track", (1, 1024), (3, 2048))])
def test_switching_a_log(make, name, first, second):
    """The sequences `observe` and `track` document: on, on again with other settings, off, off again, and an enable
    that raises."""
    chunk = {"probe": rows([1], 0, 0), "track": ([frame(1)], 0)}[name]
    engine = Recorder([chunk] * 3, [chunk] * 3)
    enable, disable, read = f"{name}_enable", (f"{name}_disable",), (f"{name}_read",)
    log = make()
    log.switch(engine, True, first)
    assert engine.calls == [(enable, *first)] and log.settings == first and log.chunks == []
    log.switch(engine, True, second)                             # read, then on with the new settings: never off
    assert engine.calls[1:] == [read, (enable, *second)] and log.settings == second and len(log.chunks) == 1
    log.switch(engine, False)
    assert engine.calls[3:] == [read, disable] and log.settings is None and len(log.chunks) == 2
    log.switch(engine, False)                                    # off again: nothing
    assert len(engine.calls) == 5 and log.settings is None and len(log.chunks) == 2
    log.switch(engine, True, first)
    engine.refuse = True
    with pytest.raises(ValueError, match="refused"):
        log.switch(engine, True, second)
    assert engine.calls[5:] == [(enable, *first), read, (enable, *second)]
    assert log.settings is None and len(log.chunks) == 3         # what was logged is kept; the log counts as off
    assert len(log.take(engine)) == 3 and engine.calls[8:] == []  # ... so nothing more is read


def test_observations_of_chunks_with_other_bins_take_the_last_setting():
    engine = Recorder([rows([1], 3, 0), rows([2], 2, 1)])
    crate = half_crate(engine)
    crate.observe(bins=3)
    crate.observe(bins=2)
    got = crate.observations()
    assert got["tick"].tolist() == [1.0, 2.0] and got["dropped"] == 1
    assert got["count"].tolist() == [[0, 0], [7, 7]] and got["count"].dtype == np.int32
    assert got["top"].tolist() == [[np.inf, np.inf], [0.25, 0.25]]
    engine.probe_chunks.append(rows([3], 2, 0))
    crate.observe(False)                                         # off: the bins are those of the last chunk
    got = crate.observations()
    assert got["tick"].tolist() == [3.0] and got["count"].shape == (1, 2)
    calls = len(engine.calls)
    got = crate.observations()                                   # nothing was logged since: T = 0, no bins, no read
    assert got["tick"].shape == (0,) and "count" not in got and got["dropped"] == 0 and len(engine.calls) == calls
