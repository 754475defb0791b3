"""The add-ons of `Crate`: what is drawn over frames, the two switchable device logs, a recording at full precision
(`trajectory.Trajectory`) and a checkpoint under way.  Each keeps its state in an object of its own -- `Overlay`,
`DeviceLog`, `Trajectory`, `PendingCheckpoint` -- and its calls are a mixin `Crate` inherits: `_Frames`, `_Logs`,
`_Checkpoints`.

One rule moves the objects to the larger context a crate grows into (`Crate._grow`): ``leave(old_engine)`` saves what
lives only in the old context, ``enter(new_engine)`` sets the add-on up again in the new one.  A new add-on implements
the two and is listed in `Crate.__init__`; `_grow` names none of them.  Importing this module needs no GPU."""
from __future__ import annotations

import copy
import json

import numpy as np

from . import _native as N
from . import track as _track
from .engine import Engine
from .hud_font import default_placement
from .load_config import WorldConfig
from .probe import as_dict, concatenate
from .trajectory import Trajectory, check_log, check_window

_ARROWS = 'arrows must be None, a bool, "velocity" or an array-like K x 2 x 2 of (start, direction)'


class AddOn:
    def leave(self, old_engine) -> None:
        pass

    def enter(self, new_engine) -> None:
        pass


# ---------------------------------------------------------------------- frames (Playback.draw_scene, playback.py:75-85)
def arrow_ends(pairs) -> np.ndarray:
    """K x 2 x 2 (start, end) of the reference's debug arrows, an array-like K x 2 x 2 of (start, direction), as
    Playback.draw_debug_arrows draws them (playback.py:95-107): entries with a NaN are dropped (:97), the direction is
    compressed, d / (|d| + 0.001) ^ 0.3 (:99), and the arrow ends at start + that."""
    a = np.asarray(pairs, dtype=np.float64).reshape(-1, 2, 2)
    a = a[~np.isnan(a).any(axis=(1, 2))]
    start, d = a[:, 0], a[:, 1]
    with np.errstate(all="ignore"):
        norm = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        d = d / np.power(norm + 0.001, 0.3)[:, None]
        return np.stack([start, start + d], axis=1)


def hud_request(hud, default, width: int):
    """The `hud` argument of the render calls -> None: no text, or (bytes, x, y, scale).  True draws `default`, a str
    that string, None or False nothing; anything else is a TypeError.  The text goes at the reference's margin in the
    built-in bitmap font, scaled for a frame this wide (hud_font.default_placement); characters outside ASCII become
    ``?``, and an empty text is no text."""
    if hud is None or hud is False:
        return None
    text = default if hud is True else hud
    if not isinstance(text, str):
        raise TypeError("hud must be None, a bool or a str")
    data = text.encode("ascii", "replace")
    return (data, *default_placement(width)) if data else None


def arrows_request(arrows, debug_arrows, every: int, scale, dt):
    """The `arrows`, `arrow_every` and `arrow_scale` arguments of the render calls -> None: no arrows, ("list", the
    bytes of the K x 2 x 2 ends) or ("velocity", scale, every).  None or False draws none; True draws `debug_arrows`, the
    reference's list of (start, direction) in world units; an array-like K x 2 x 2 of (start, direction) is drawn the same
    way (`arrow_ends`), and none of them is no arrows; "velocity" asks the device for one arrow per `every`-th particle
    along velocity * `scale`, by default `dt`, the step the particle is about to take.  Anything else is a TypeError."""
    if arrows is None or arrows is False:
        return None
    if isinstance(arrows, str):
        if arrows != "velocity":
            raise TypeError(_ARROWS)
        return "velocity", float(dt if scale is None else scale), int(every)
    try:
        ends = arrow_ends(debug_arrows if arrows is True else arrows)
    except (TypeError, ValueError):
        raise TypeError(_ARROWS) from None
    return ("list", ends.tobytes()) if len(ends) else None


def _tell_arrows(engine, want) -> None:
    if want is None:
        engine.set_arrows(N.ARROWS_OFF)
    elif want[0] == "list":
        engine.set_arrows(N.ARROWS_LIST, np.frombuffer(want[1], dtype=np.float64))
    else:
        engine.set_arrows(N.ARROWS_VELOCITY, None, want[1], want[2])


class Overlay(AddOn):
    """What the engine was last told to draw on frames: `sent` maps "hud" to the request of `hud_request` and "arrows" to
    that of `arrows_request`; nothing -- None -- is also what a new context draws."""
    _TELL = {"hud": lambda engine, want: engine.set_hud(*(want or (None,))), "arrows": _tell_arrows}

    def __init__(self) -> None:
        self.sent = {}

    def send(self, engine, what: str, want) -> None:
        """The engine is told only when the request differs from the last one; if it refuses, nothing counts as sent."""
        if want != self.sent.get(what):
            self.sent[what] = None
            self._TELL[what](engine, want)
            self.sent[what] = want

    def enter(self, new_engine) -> None:
        """Forgets both requests: they are sent again with the next frame."""
        self.sent = {}


class _Frames:
    def _frame(self, width, height, zoom, center, segment_width, hud, arrows, arrow_every, arrow_scale):
        """-> (view, segments) of a frame, the engine told what to draw over it where that changed since the last frame:
        the text (`hud_request`; True is `debug_prints`) and the arrows (`arrows_request`; True is `debug_arrows`)."""
        view = Engine.view(width, height, self.particle_radius, zoom=zoom, center=center, segment_width=segment_width)
        segments = self.segments if self.rigid_bodies else np.zeros((0, 2, 2))
        self._overlay.send(self._engine, "hud", hud_request(hud, self.debug_prints if hud is True else None, width))
        self._overlay.send(self._engine, "arrows",
                           arrows_request(arrows, self.debug_arrows, arrow_every, arrow_scale, self.dt))
        return view, segments

    def render(self, width: int = 1000, height: int = 1000, *, zoom: float = 1.0, center=None, segment_width: int = 2,
               out=None, hud=None, arrows=None, arrow_every: int = 1, arrow_scale=None):
        """The frame the reference's viewer draws after `physics_tick()`, rendered on the GPU: every particle a disc of
        ``int(width * particle_radius) * zoom`` pixels coloured by its pressure (white at 0, blue at 1 and above), the
        walls (`segments`) on top in white, black elsewhere; ``height x width x 3`` uint8, row 0 at the top.

        It shows the device state as `sc_download_state` would return it: the pressure is that of the last finished
        tick, so right after the particles were set -- or after `from_checkpoint`, before the first tick -- every
        particle is white.  `center` is in screen pixels (default: the frame's centre).  With `out` a CUDA uint8 tensor
        of shape (height, width, 3) the frame is written there on the library's stream and the call returns without
        synchronising: the library's stream does not wait for torch's, so the tensor must be ready when this is called
        and read after `synchronize()` (or run the crate on torch's stream, `engine.set_stream`).  Otherwise it returns a
        NumPy array.  `hud=True` writes the HUD text (`debug_prints`) over the frame at the top left, `hud` a str that
        string (`hud_request`); telling the engine a new text synchronises.  `arrows` draws the viewer's debug arrows,
        green, between the walls and the text: True the list `debug_arrows`, an array of (start, direction) that,
        "velocity" one per `arrow_every`-th particle along its velocity times `arrow_scale` (`arrows_request`).
        The pixel rule, bit for bit: tests/render_spec.py, tests/arrow_spec.py for the arrows and tests/text_spec.py for
        the text."""
        view, segments = self._frame(width, height, zoom, center, segment_width, hud, arrows, arrow_every, arrow_scale)
        return self._engine.render(view, segments, out)

    def render_jpeg(self, width: int = 1000, height: int = 1000, *, quality: int = 95, zoom: float = 1.0, center=None,
                    segment_width: int = 2, hud=None, arrows=None, arrow_every: int = 1, arrow_scale=None) -> bytes:
        """`render`'s frame as a JPEG file, encoded on the GPU: only the compressed bytes leave it.  Baseline JPEG, 4:4:4,
        the standard tables at `quality` (1..100; 95 is cv2's default, what the reference's AVI writer uses).  `hud`,
        `arrows`, `arrow_every` and `arrow_scale` as in `render`: text and arrows are on the frame before it is encoded.
        The bitstream, byte for byte: tests/jpeg_spec.py applied to `render`'s frame."""
        view, segments = self._frame(width, height, zoom, center, segment_width, hud, arrows, arrow_every, arrow_scale)
        return self._engine.render_jpeg(view, segments, quality)

    def render_gif(self, width: int = 1000, height: int = 1000, *, zoom: float = 1.0, center=None,
                   segment_width: int = 2, hud=None, arrows=None, arrow_every: int = 1, arrow_scale=None) -> bytes:
        """`render`'s frame as the image data of one GIF frame, compressed on the GPU: only the LZW bytes leave it;
        `gif.GifWriter` strings such frames into ``video.gif``.  The frame has a GIF's worth of colours by construction
        -- black and (c, c, 255) -- so nothing is quantised: palette entry 0 is black, entry k is (k, k, 255).  The one
        loss: (0, 0, 255), a pressure of 1 and above, is stored as entry 1, (1, 1, 255).  `hud` as in `render`: the text
        is white like the walls, entry 255.  `arrows`, `arrow_every` and `arrow_scale` as in `render`: a frame with arrows
        keeps entry 1 for them -- (0, 255, 0) in `gif.palette(arrows=True)` -- and stores a disc of colour byte c as
        max(c, 2), so there (0, 0, 255) and (1, 1, 255) both become (2, 2, 255).
        The bitstream, byte for byte: tests/gif_spec.py (`image_data(indices(frame))`) applied to `render`'s frame."""
        view, segments = self._frame(width, height, zoom, center, segment_width, hud, arrows, arrow_every, arrow_scale)
        return self._engine.render_gif(view, segments)


# ---------------------------------------------------------------------- logs
class DeviceLog(AddOn):
    """A log in device memory that can be switched: `settings`, the arguments it is on with, or None: off; and `chunks`,
    what was read from a context that is gone, or before the log was switched.  enable(engine, *settings),
    disable(engine) and read(engine) -> a chunk are the engine's calls of the log."""

    def __init__(self, enable, disable, read) -> None:
        self._enable, self._disable, self._read = enable, disable, read
        self.settings = None
        self.chunks = []

    def leave(self, old_engine) -> None:
        if self.settings is not None:
            self.chunks.append(self._read(old_engine))

    def enter(self, new_engine) -> None:
        if self.settings is not None:
            self._enable(new_engine, *self.settings)

    def switch(self, engine, on: bool, settings=()) -> None:
        """What was logged so far is read and kept; then the log is on with `settings`, or off (also if enable raises)."""
        self.leave(engine)
        was, self.settings = self.settings, None
        if on:
            self._enable(engine, *settings)
            self.settings = tuple(settings)
        elif was is not None:
            self._disable(engine)

    def take(self, engine) -> list:  # -> every chunk since the last call, oldest first
        self.leave(engine)
        chunks, self.chunks = self.chunks, []
        return chunks


def _read_frames(engine):
    blob, _, dropped = engine.track_read()
    return _track.split(blob), dropped


# the two logs, as `DeviceLog` takes them: of `observe`, settings (capacity, bins, x0, x1) and chunks (rows, counts, tops,
# dropped); of `track`, settings (every, capacity_bytes) and chunks (frames, dropped)
OBSERVABLES = (lambda e, *s: e.probe_enable(*s), lambda e: e.probe_disable(), lambda e: e.probe_read())
FRAMES = (lambda e, *s: e.track_enable(*s), lambda e: e.track_disable(), _read_frames)


class _Logs:
    # ------------------------------------------------------------------ observables (sc_probe_*; tests/probe_spec.py)
    def measure(self, bins: int = 0, x_range=(0.0, 1.0)) -> dict:
        """The state as it stands, reduced on the device to the sixteen numbers of `probe.FIELDS` -- {name: value} -- and,
        with `bins`, the profile of the free surface over `x_range`: `count` (bins,) int32 particles per column and
        `top` (bins,) the smallest y in each (gravity points to +y), +inf where a column is empty.  Nothing but these
        numbers is downloaded; synchronises.  The simulation is left alone."""
        row, counts, tops = self._engine.probe_now(bins, float(x_range[0]), float(x_range[1]))
        return as_dict(row, counts, tops)

    def observe(self, on: bool = True, *, capacity: int = 4096, bins: int = 0, x_range=(0.0, 1.0)) -> None:
        """Switch the device log: while on, every tick (`physics_tick` and each tick of `run`) appends what `measure`
        would return to a log of `capacity` rows in device memory, with no synchronisation and no download until
        `observations()` reads it.  A tick that finds the log full is dropped and counted.  Switching the log (on again
        with other settings, or off) keeps what was logged so far for the next `observations()`."""
        self._observed.switch(self._engine, on, (int(capacity), int(bins), float(x_range[0]), float(x_range[1])))

    def observations(self) -> dict:
        """What was logged since the last call, oldest first: a T-long float64 array per name of `probe.FIELDS`, `count`
        (T x bins, int32) and `top` (T x bins) when the log has bins, and `dropped`, the ticks that found the log
        full.  T = 0 when nothing was logged.  Synchronises.  (`tick` counts the ticks of the GPU context, and goes on
        counting when the crate had to grow into a larger one: `_grow`.)"""
        chunks, on = self._observed.take(self._engine), self._observed.settings
        bins = on[1] if on is not None else (chunks[-1][1].shape[1] if chunks else 0)
        # (the bins changed between reads: the profiles of the last setting, empty ones for the chunks of another)
        chunks = [c if c[1].shape[1] == bins else (c[0], np.zeros((len(c[0]), bins), dtype=np.int32),
                                                  np.full((len(c[0]), bins), np.inf), c[3]) for c in chunks]
        return concatenate([as_dict(*c) for c in chunks], bins)

    # ------------------------------------------------------------------ packed frames (sc_track_*; tests/track_spec.py)
    def capture_frame(self) -> bytes:
        """The state as it stands as one packed frame (`track.parse` reads it, `track.Player` draws it): nine bytes per
        particle -- id, position on a 16-bit grid over [-0.25, 1.25], the colour byte `render` would give it -- behind the
        tick number and the walls as they stand.  Packed on the device; only the frame is downloaded.  Synchronises; the
        simulation is left alone."""
        self._send_tick_inputs()  # (the walls as they stand: before the first tick the engine has seen none)
        return self._engine.track_capture()

    def track(self, on: bool = True, *, every: int = 1, capacity_bytes: int = 1 << 26) -> None:
        """Switch the device log of frames: while on, every tick whose number is a multiple of `every` (`physics_tick`
        and each tick of `run`) appends what `capture_frame` would return to a log of `capacity_bytes` in device memory,
        with no synchronisation and no download until `tracked()` reads it.  A frame that does not fit is dropped whole
        and counted.  Switching the log (on again with other settings, or off) keeps what was logged so far for the next
        `tracked()`."""
        self._tracked.switch(self._engine, on, (int(every), int(capacity_bytes)))

    def tracked(self) -> tuple[list[bytes], int]:
        """-> (the frames logged since the last call, oldest first; how many were dropped because the log was full).
        Synchronises.  (A frame's tick counts the ticks of the GPU context, and goes on counting when the crate had to
        grow into a larger one: `_grow`.)"""
        chunks = self._tracked.take(self._engine)
        return [f for c in chunks for f in c[0]], sum(c[1] for c in chunks)

    # ------------------------------------------------------------------ trajectories (sc_traj_*; tests/trajectory_spec.py)
    def record_trajectory(self, frames: int, *, ids=None, every: int = 1, pressure: bool = False,
                          initial: bool = True) -> Trajectory:
        """Record the run at full precision into torch CUDA tensors, one row per particle id: while the returned
        `Trajectory` records, every tick whose number is a multiple of `every` (`physics_tick` and each tick of `run`)
        writes one frame -- ``states[t, r]`` is (x, y, vx, vy) of the live particle with id ``lo + r``, exactly what
        `state_tensors` would deliver for it, and NaN where that id is not live; with `pressure` its pressure too -- into
        a log of `frames` frames, with no sort, no allocation and no synchronisation until `Trajectory.read()`.  A frame
        that finds the log full is dropped and counted.  `ids` = (lo, hi) is the window of ids that get a row; the default
        is (0, `max_particles` of the world's configuration) -- not the capacity: a run does not depend on it -- and live
        particles outside it are counted per frame, not recorded.  `initial` captures the state as it stands as the first
        frame.  One recording at a time: a second call stops the first, whose tensors stay readable.

        The log is written on the library's stream, and the library's stream does not wait for torch's: read it after
        `Trajectory.read()` or `synchronize()` -- or run the crate on torch's stream, `engine.set_stream`, and everything
        torch enqueues afterwards sees it."""
        frames, every = check_log(frames, every)
        id0, rows = check_window(ids, int(self.world_config.coefficients["max_particles"]))
        self.stop_trajectory()
        self._trajectory = Trajectory(self._engine, frames, id0, rows, every, bool(pressure))
        self._addons.append(self._trajectory)
        if initial:
            self._trajectory.capture()
        return self._trajectory

    def stop_trajectory(self) -> None:
        """Stops the recording `record_trajectory` started, if any, and synchronises: nothing is queued against its
        tensors afterwards."""
        traj, self._trajectory = self._trajectory, None
        if traj is not None:
            self._addons.remove(traj)
            traj.stop()


# ---------------------------------------------------------------------- checkpoints (playback.py:109-118, grown up)
class PendingCheckpoint(AddOn):
    """A checkpoint under way: `meta`, what `begin_checkpoint` wrote down on the host, or None: none is; `snapshot`,
    the capture, once it was collected from the context that took it."""

    def __init__(self) -> None:
        self.meta = self.snapshot = None

    def leave(self, old_engine) -> None:  # (the capture lives in the context that took it)
        if self.meta is not None and self.snapshot is None:
            self.snapshot = old_engine.checkpoint_finish()

    def finish(self, engine):
        """-> (meta, snapshot); nothing is under way from here on, whether or not the engine delivers."""
        meta, snapshot = self.meta, self.snapshot
        self.meta = self.snapshot = None
        return meta, engine.checkpoint_finish() if snapshot is None else snapshot


class _Checkpoints:
    def begin_checkpoint(self) -> None:
        """Capture the whole simulation state as of now.  Returns at once: the particle state is copied on the device
        and travels to pinned host memory on a side stream while later ticks run; `finish_checkpoint` collects it."""
        if self._checkpoint.meta is not None:
            raise RuntimeError("a checkpoint is already under way")
        self._engine.checkpoint_begin()
        bodies = [{"segments": body.segments.tolist(), "position": [float(x) for x in body.position],
                   "center_velocity": np.asarray(body.center_velocity, dtype=np.float64).tolist(),
                   "angular_clockwise_velocity": float(body.angular_clockwise_velocity),
                   "time_from_start": float(getattr(body, "time_from_start", 0.0))} for body in self.rigid_bodies]
        host_rng = None
        if self._noise != "host":  # the host owns the global stream (the device's copy travels with the particles)
            _, key, pos, has_gauss, cached = np.random.get_state()
            host_rng = {"key": key.tolist(), "pos": int(pos), "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}
        wc = self.world_config
        self._checkpoint.meta = {
            "format": 1, "tick": int(self.tick), "noise": self._noise, "noise_seed": int(self._noise_seed),
            "world_config": {"rigid_bodies": copy.deepcopy(wc.rigid_bodies), "particle_sources": copy.deepcopy(wc.particle_sources),
                             "coefficients": self._coefficients()},
            "bodies": bodies, "host_rng": host_rng, "pressure": self._cache[2] if self._cache is not None else None}

    def finish_checkpoint(self, path) -> None:
        """Wait for the transfer `begin_checkpoint` started (not for later ticks) and write the .npz file."""
        if self._checkpoint.meta is None:
            raise RuntimeError("begin_checkpoint first")
        meta, snap = self._checkpoint.finish(self._engine)
        pressure = meta.pop("pressure")
        meta["next_id"] = int(snap["next_id"])
        meta["engine_tick"] = int(snap["tick"])
        arrays = {"particles": snap["particles"], "velocities": snap["velocities"], "ids": snap["ids"]}
        if pressure is not None and len(pressure) == len(snap["ids"]):
            arrays["pressure"] = pressure
        # the stream to restore is the one the run draws from: the device's in noise mode "host", else the host's (a crate
        # that fell back from "host" to "host-sync" still has a -- stale -- device state: it is not written)
        if snap["rng"] is not None and meta["noise"] == "host":
            arrays["rng_key"] = snap["rng"][0]
            meta["rng_pos"] = int(snap["rng"][1])
        np.savez(path, meta=np.array(json.dumps(meta)), **arrays)

    def save_checkpoint(self, path) -> None:
        self.begin_checkpoint()
        self.finish_checkpoint(path)

    @classmethod
    def from_checkpoint(cls, path, *, device: int = 0, capacity: int | None = None) -> "Crate":
        """A crate that continues the run `save_checkpoint` captured: same particles (and ids), velocities, tick,
        wall positions and motor clocks, coefficients as edited, and the random stream where it stood."""
        with np.load(path, allow_pickle=False) as z:
            meta = json.loads(str(z["meta"]))
            arrays = {k: z[k] for k in z.files if k != "meta"}
        wc = meta["world_config"]
        crate = cls(WorldConfig(rigid_bodies=wc["rigid_bodies"], particle_sources=wc["particle_sources"],
                                coefficients=wc["coefficients"]),
                    device=device, noise=meta["noise"], noise_seed=meta["noise_seed"], capacity=capacity)
        for body, saved in zip(crate.rigid_bodies, meta["bodies"]):
            body.segments = np.array(saved["segments"], dtype=np.float64)
            body.position = list(saved["position"])
            body.center_velocity = np.array(saved["center_velocity"], dtype=np.float64)
            body.angular_clockwise_velocity = saved["angular_clockwise_velocity"]
            if hasattr(body, "time_from_start"):
                body.time_from_start = saved["time_from_start"]
        n = len(arrays["ids"])
        if n > crate._engine.capacity:
            crate._grow(n)
        eng = crate._engine
        eng.upload_with_ids(arrays["particles"], arrays["velocities"], arrays["ids"])
        eng.restore_counters(meta["engine_tick"], meta["next_id"])
        crate.tick = meta["tick"]
        crate._state_changed(n, (arrays["particles"], arrays["velocities"], arrays.get("pressure", np.zeros(n))))
        if meta["noise"] == "host" and "rng_key" in arrays:
            eng.rng_set_state(arrays["rng_key"], meta["rng_pos"])
        elif meta["host_rng"] is not None:
            h = meta["host_rng"]
            np.random.set_state(("MT19937", np.array(h["key"], dtype=np.uint32), h["pos"], h["has_gauss"], h["cached_gaussian"]))
        return crate
