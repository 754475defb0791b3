"""The rule of the trajectory log (sc_traj_enable_device; `Crate.record_trajectory`, sand_crate_amd/trajectory.py) in
NumPy: from the state as the device stores it to the frames the caller's tensors receive.

A recording has a window of ids [id0, id0 + M), F frames and `every` >= 1.  A frame is taken after every tick whose number
(ticks finished by the context) is a multiple of `every`, and on demand between ticks.  A frame is built on the export's
rule, `state_spec.export` -- which slots are live, which bits they deliver, which pressure belongs to them -- and only
says where the export's rows go: the particle with id i to row i - id0.  Every other row is FILL.  No device, no
reference."""
from __future__ import annotations

import numpy as np

import state_spec

FILL_BITS = 0x7FF8000000000000                       # an absent row: four of these (the pressure: one)
FILL = np.array([FILL_BITS], dtype=np.uint64).view(np.float64)[0]
MAX_ID = 2 ** 31 - 2                                 # ids reach this, so a window may end at MAX_ID + 1 = INT_MAX


def filled(shape):
    """float64 array of this shape with FILL's bits everywhere (np.full keeps a NaN's payload, but says so nowhere)."""
    return np.full(shape, FILL_BITS, dtype=np.uint64).view(np.float64)


def frame_of_export(xy, vxy, pressure, ids, id0, rows):
    """One frame from what the export (or `Engine.download()`, the same arrays) delivers: -> (states (M, 4), pressure (M,),
    count, outside).  Ids are unique; the rule says nothing about a state where they are not."""
    id0, rows = int(id0), int(rows)
    assert 0 <= id0 and rows >= 1 and id0 + rows <= MAX_ID + 1
    ids = np.asarray(ids, dtype=np.int64)
    assert len(np.unique(ids)) == len(ids)
    r = ids - id0
    inside = (r >= 0) & (r < rows)
    states, press = filled((rows, 4)), filled((rows,))
    states[r[inside], 0:2] = np.asarray(xy, dtype=np.float64).reshape(-1, 2)[inside]
    states[r[inside], 2:4] = np.asarray(vxy, dtype=np.float64).reshape(-1, 2)[inside]
    press[r[inside]] = np.asarray(pressure, dtype=np.float64)[inside]
    return states, press, len(ids), int((~inside).sum())


def frame(x, y, vx, vy, P, ids, n_stored, n_ticked, pressure_valid, id0, rows):
    """One frame from the storage arrays, through `state_spec.export`."""
    return frame_of_export(*state_spec.export(x, y, vx, vy, P, ids, n_stored, n_ticked, pressure_valid), id0, rows)


def present(states):
    """Which rows hold a particle: live means a finite x, and an absent row's x is FILL."""
    return np.isfinite(np.asarray(states)[..., 0])


def due(tick: int, every: int) -> bool:
    """Does the tick that brought the context's count of finished ticks to `tick` take a frame?"""
    return tick % every == 0


class Log:
    """The log and its two counters: `cursor` counts the frames written, `dropped` those that found the log full.
    `take(tick, export, abandoned)` is one frame that is due -- after a tick, or on demand (never abandoned); an abandoned
    tick leaves no frame and is not counted as dropped."""

    def __init__(self, frames: int, id0: int, rows: int, pressure: bool = True):
        self.frames, self.id0, self.rows = int(frames), int(id0), int(rows)
        self.states = np.zeros((self.frames, self.rows, 4))      # (rows beyond the cursor are whatever they were)
        self.pressure = np.zeros((self.frames, self.rows)) if pressure else None
        self.ticks = np.zeros(self.frames, dtype=np.int64)
        self.counts = np.zeros(self.frames, dtype=np.int64)
        self.outside = np.zeros(self.frames, dtype=np.int64)
        self.cursor = self.dropped = 0

    def restart(self):
        self.cursor = self.dropped = 0

    def take(self, tick, export, abandoned=False):
        if abandoned:
            return
        if self.cursor >= self.frames:
            self.dropped += 1
            return
        f = self.cursor
        self.cursor += 1
        states, press, count, outside = frame_of_export(*export, self.id0, self.rows)
        self.states[f] = states
        if self.pressure is not None:
            self.pressure[f] = press
        self.ticks[f], self.counts[f], self.outside[f] = tick, count, outside

    def read(self):
        t = self.cursor
        out = dict(states=self.states[:t], ticks=self.ticks[:t], counts=self.counts[:t], outside=self.outside[:t],
                   dropped=self.dropped)
        if self.pressure is not None:
            out["pressure"] = self.pressure[:t]
        return out
