"""`Trajectory`: a recording of the state at full precision, in torch tensors on the device, one row per particle id
(sc_traj_enable_device; the rule is tests/trajectory_spec.py on top of tests/state_spec.py).

`Crate.record_trajectory` makes one.  While it records, every tick whose number is a multiple of `every` -- and every
`capture()` -- writes one frame: ``states[t, r]`` is (x, y, vx, vy) of the live particle whose id is ``id0 + r``, the bits
`Crate.state_tensors` would deliver, and four NaNs where that id is not live.  Ids are unique and stable, so the id is the
row address: frames line up by particle without a sort, nothing is allocated per tick and nothing synchronises until
`read()`.  A log of `frames` frames that is full drops further frames and counts them.

The tensors are written on the library's stream, and the library's stream does not wait for torch's: read them after
`read()` / `synchronize()`, or run the crate on torch's stream (`engine.set_stream`) and everything torch enqueues
afterwards sees them."""
from __future__ import annotations

FILL_BITS = 0x7FF8000000000000  # the quiet NaN of an absent row (csrc/sc_traj.h: kTrajFillBits)
WORDS = 4                       # the log's words: cursor, dropped, the frame the last reserve chose, spare
MAX_ID = 2 ** 31 - 2            # the largest particle id


def check_window(ids, default_rows: int) -> tuple[int, int]:
    """-> (id0, rows) of the window `ids` = (lo, hi), or of (0, default_rows) for None.  ValueError unless
    0 <= lo < hi <= 2^31 - 1."""
    lo, hi = (0, int(default_rows)) if ids is None else (int(ids[0]), int(ids[1]))
    if not 0 <= lo < hi <= MAX_ID + 1:
        raise ValueError(f"ids=({lo}, {hi}): the window needs 0 <= lo < hi <= {MAX_ID + 1}")
    return lo, hi - lo


def check_log(frames, every) -> tuple[int, int]:
    frames, every = int(frames), int(every)
    if frames < 1:
        raise ValueError("frames must be at least 1")
    if every < 1:
        raise ValueError("every must be at least 1")
    return frames, every


def present(states):
    """Which rows of `states` (..., M, 4) hold a particle: x is finite exactly there."""
    import torch
    return torch.isfinite(states[..., 0])


def complete_rows(states):
    """The rows of `states` (T, M, 4) that hold a particle in every frame -- what a training window keeps: int64 indices
    into the window (add `id0` for the ids)."""
    import torch
    return torch.nonzero(present(states).all(dim=0)).reshape(-1)


class Trajectory:
    """The log of one recording: the tensors, and the engine that writes into them (`Crate._grow` moves it to the new
    one: `leave`, `enter`).  Made by `Crate.record_trajectory`."""

    def __init__(self, engine, frames: int, id0: int, rows: int, every: int = 1, pressure: bool = False):
        import torch
        frames, every = check_log(frames, every)
        id0, rows = check_window((id0, id0 + rows), 0)
        dev = torch.device("cuda", engine.device)
        self._engine = engine
        self._id0, self._rows, self._frames, self._every = id0, rows, frames, every
        self.states = torch.empty((frames, rows, 4), dtype=torch.float64, device=dev)
        self.pressure = torch.empty((frames, rows), dtype=torch.float64, device=dev) if pressure else None
        self.ticks = torch.zeros(frames, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(frames, dtype=torch.int64, device=dev)
        self.outside = torch.zeros(frames, dtype=torch.int64, device=dev)
        self.words = torch.zeros(WORDS, dtype=torch.int64, device=dev)
        torch.cuda.current_stream(dev).synchronize()  # (torch's fills are done before the library writes)
        self._enable(reset=True)

    id0 = property(lambda self: self._id0)
    rows = property(lambda self: self._rows)
    frames = property(lambda self: self._frames)
    every = property(lambda self: self._every)

    @property
    def recording(self) -> bool:
        return self._engine is not None

    def _enable(self, reset: bool) -> None:
        self._engine.traj_enable(self.states, self.pressure, self.ticks, self.counts, self.outside, self.words,
                                 id0=self._id0, every=self._every, reset=reset)

    def leave(self, old_engine) -> None:
        """An add-on of the crate (addons.py) whose log is torch's: nothing lives in the context that goes."""

    def enter(self, new_engine) -> None:
        """... and the recording goes on in the one that replaces it, where the words stand."""
        if self._engine is not None:
            self._engine = new_engine
            self._enable(reset=False)

    def _need_engine(self):
        if self._engine is None:
            raise RuntimeError("the recording was stopped")
        return self._engine

    def capture(self) -> None:
        """One frame of the state as it stands, now: the initial state, or one just loaded.  Enqueued only."""
        self._need_engine().traj_capture()

    def restart(self) -> None:
        """The log starts over: the words are zeroed on the library's stream, the window and `every` stay."""
        self._need_engine()
        self._enable(reset=True)

    def read(self) -> dict:
        """Synchronises the library's stream and reads the 32 bytes of the words.  -> `states` (T, M, 4), its views
        `positions` and `velocities` (T, M, 2), `pressure` (T, M) if recorded, `ticks`, `counts`, `outside` (T,) -- cut to
        the T frames recorded so far --, `dropped`, the frames that found the log full, and `ids`, the window's arange.
        The tensors are the log itself, not copies; reading does not restart it, recording continues behind T."""
        import torch
        if self._engine is not None:
            self._engine.synchronize()
        cursor, dropped = (int(w) for w in self.words[:2].cpu().tolist())
        t = max(0, min(cursor, self._frames))
        out = {"states": self.states[:t], "positions": self.states[:t, :, 0:2], "velocities": self.states[:t, :, 2:4],
               "ticks": self.ticks[:t], "counts": self.counts[:t], "outside": self.outside[:t], "dropped": dropped,
               "ids": torch.arange(self._id0, self._id0 + self._rows, dtype=torch.int64, device=self.states.device)}
        if self.pressure is not None:
            out["pressure"] = self.pressure[:t]
        return out

    def stop(self) -> None:
        """Stops recording and synchronises, so that nothing is queued against the tensors when torch may free them.
        What was recorded stays readable."""
        engine = self._engine
        if engine is not None:
            engine.traj_disable()
            self._engine = None
            engine.synchronize()

    present = staticmethod(present)
    complete_rows = staticmethod(complete_rows)
