"""`Crate`: the reference's simulation object (``src/crate/crate.py:19-371``) with the per-timestep
particle update running on an MI355X.

Drop-in surface: ``Crate(world_config)``, ``physics_tick()``, and the
attributes the viewer reads or writes between ticks -- ``particles``, ``particle_velocities``,
``particles_pressure``, ``particle_radius``, ``segments``, ``gravity``, every YAML coefficient by
name, ``editable_coefficients()``, ``debug_arrows``, ``debug_prints``, ``tick``,
``particle_count``, ``diameter``, ``rigid_bodies``, ``particle_sources``.

What runs where
---------------
host   rigid-body motion (rigid_body.py) and pad_segments: O(S) per tick.  The particle sources: on the DEVICE
       (sc_emit_particles, below) with noise="host", where the device holds NumPy's stream; on the host
       (particle_source.py: `_create_new_particles`) in the modes that leave ``np.random`` to the host --
       "counter", "none" and "host-sync".
GPU    everything per particle: removal, wall contacts + hard wall fix, strip sort and neighbor
       lists, pressure / tension / gravity / viscosity / wall bounce / continuous collision,
       integration (sand_crate_amd/csrc/sc_kernels.h).  State stays on the device; the
       ``particles`` / ``particle_velocities`` / ``particles_pressure`` attributes download
       lazily, once per tick, when read.

Collider noise (crate.py:169) and particle sources (particle_source.py:17-24) draw from NumPy's global MT19937
stream in the reference.  Modes:
``"host"``    (default) that very stream, bit for bit, generated ON THE DEVICE: `Crate.__init__` seeds
              ``np.random`` like the reference (crate.py:22) and hands the state to the library
              (sc_rng_set_state); sources and noise are then drawn by kernels (sc_rng.h) and a tick costs no
              readback, no host draw and no upload.  `sync_host_rng()` returns the stream to ``np.random``
              for callers that draw from it themselves between ticks.  (Both branches of NumPy's legacy binomial are
              on the device -- inversion up to flow * dt = 30, BTPE beyond; only dt > 0.5 makes the crate fall back to
              the next mode.)
``"host-sync"`` the same numbers drawn by the host: one device->host count and one upload per tick;
``"counter"`` a counter-based hash on the device keyed by (seed, tick, particle id, slot): same
              distribution, different numbers, no host round trip (used for throughput runs);
``"none"``    no noise (what ``collider_noise_level = 0`` computes).

There is no CPU implementation behind this class: without libsandcrate_hip.so and a GPU it raises.
"""
from __future__ import annotations

import copy
import json
import time

import numpy as np
import yaml

from . import _native as N
from .engine import Engine
from .hud_font import default_placement
from .load_config import WorldConfig
from .neighbourhood import _Neighbourhood
from .particle_source import build_particle_sources
from .probe import FIELDS, as_dict
from . import track as _track
from .trajectory import Trajectory, check_log, check_window
from .rigid_body import build_rigid_bodies
from .utils.geometry_utils import pad_segments

_NOISE_MODES = {"none": N.NOISE_NONE, "host": N.NOISE_HOST, "host-sync": N.NOISE_HOST, "counter": N.NOISE_COUNTER}
FORCE_PHASES = ("tension", "gravity", "pressure", "viscosity", "wall_bounce", "continuous_collision")  # crate.py:110-123
_TICK_COEFFICIENTS = ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
                      "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure")


def tick_geometry(rigid_bodies, particle_radius, cache):
    """-> (segments S x 2 x 2, padded 2S x 2 x 2, [(position, center_velocity, omega, n_segments)]) of one
    tick: `Crate.segments` (crate.py:69-71) and `pad_segments` of it (geometry_utils.py:146-172).  Padding
    is per segment, so bodies that did not move reuse their padded halves from `cache`."""
    if not rigid_bodies:
        return np.zeros((0, 2, 2)), np.zeros((0, 2, 2)), []
    plus, minus = [], []
    for body in rigid_bodies:
        hit = cache.get(id(body))
        # (a body that moves gets a new `segments` array every tick -- rigid_body.py: apply_velocity -- so the identity of
        # the array says whether the cached halves still belong to it; the contents are compared only for the same array,
        # which somebody may have edited in place)
        if hit is None or hit[0] != particle_radius or hit[1] is not body.segments or hit[2].tobytes() != body.segments.tobytes():
            pad = pad_segments(body.segments, particle_radius)
            hit = (particle_radius, body.segments, body.segments.copy(), pad[: len(body)], pad[len(body):])
            cache[id(body)] = hit
        plus.append(hit[3])
        minus.append(hit[4])
    seg = np.concatenate([body.segments for body in rigid_bodies])
    bodies = [(b.position, b.center_velocity, b.angular_clockwise_velocity, len(b)) for b in rigid_bodies]
    return seg, np.concatenate(plus + minus), bodies


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


class Crate(_Neighbourhood):
    def __init__(self, world_config: WorldConfig, *, device: int = 0, noise: str = "host", noise_seed: int = 0,
                 capacity: int | None = None) -> None:
        if noise not in _NOISE_MODES:
            raise ValueError(f"noise must be one of {sorted(_NOISE_MODES)}")
        np.random.seed(0)  # the reference seeds the global legacy RNG here (crate.py:22)
        self.tick: int = 0
        self.debug_arrows: list = []
        self._debug_prints: str | None = ""
        self.world_config = world_config
        self.rigid_bodies = build_rigid_bodies(world_config.rigid_bodies)
        self.particle_sources = build_particle_sources(world_config.particle_sources)
        for name in self.editable_coefficients():
            setattr(self, name, world_config.coefficients[name])
        self.gravity = np.array(world_config.coefficients["gravity"])

        cap = capacity if capacity is not None else int(self.max_particles) + 1024
        self._engine = Engine(max(int(cap), 1), device=device)
        self._noise = noise
        self._noise_seed = noise_seed
        self._engine.set_noise_mode(_NOISE_MODES[noise], noise_seed)
        if noise == "host":        # the device takes over the global stream the reference draws from
            self._hand_rng_to_device()
        self._count = 0            # particles on the device after the last tick / upload
        self._count_known = True
        self._cache = None         # (particles, velocities, pressure) downloaded for this tick
        self._empty()
        self._tick_seconds = 0.0   # EMA of wall time per tick, for debug_prints
        self._pad_cache = {}
        self._hud_kernels = False
        self._kernel_seconds = {}
        self._hud_forces = False
        self._force_ema = {}
        self._pending_checkpoint = None
        self._hud_sent = None      # (text bytes, x, y, scale) the engine draws on frames, or None: no HUD
        self._arrows_sent = None   # ("list", bytes of the K x 2 x 2 ends) or ("velocity", scale, every), or None: no arrows
        self._observe = None       # (capacity, bins, x0, x1) of the device log of observables, or None: not logging
        self._observed = []        # rows read from an engine that is gone, or before the log was switched off
        self._track = None         # (every, capacity_bytes) of the device log of packed frames, or None: not tracking
        self._tracked = []         # (frames, dropped) read from an engine that is gone, or before the log was switched off
        self._trajectory = None    # the `Trajectory` that records, or None
        self.last_stats = None

    # ------------------------------------------------------------------ reference accessors
    def editable_coefficients(self) -> list[str]:
        return list(self.world_config.coefficients.keys())

    @property
    def diameter(self) -> float:
        return self.particle_radius * 2

    @property
    def segments(self) -> np.ndarray:
        return np.vstack([body.segments for body in self.rigid_bodies])

    @property
    def particle_count(self) -> int:
        if not self._count_known:
            self._count = self._engine.count()
            self._count_known = True
        return self._count

    # ------------------------------------------------------------------ state attributes
    def _empty(self) -> None:
        self._cache = (np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0,)))

    def _state(self):
        if self._cache is None:
            p, v, pr, _ = self._engine.download()
            self._cache = (p, v, pr)
            self._count, self._count_known = len(p), True
        return self._cache

    @property
    def particles(self) -> np.ndarray:
        return self._state()[0]

    @particles.setter
    def particles(self, value) -> None:
        value = np.array(value, dtype=np.float64).reshape(-1, 2)
        vel = self._state()[1]
        if len(vel) != len(value):
            vel = np.zeros_like(value)
        self._set_state(value, vel)

    @property
    def particle_velocities(self) -> np.ndarray:
        return self._state()[1]

    @particle_velocities.setter
    def particle_velocities(self, value) -> None:
        value = np.array(value, dtype=np.float64).reshape(-1, 2)
        pos = self._state()[0]
        if len(pos) != len(value):
            raise ValueError("set particles before particle_velocities when the particle count changes")
        self._set_state(pos, value)

    @property
    def particles_pressure(self) -> np.ndarray:
        return self._state()[2]

    def _set_state(self, particles: np.ndarray, velocities: np.ndarray) -> None:
        if len(particles) > self._engine.capacity:
            self._grow(len(particles))
        self._engine.upload(particles, velocities)
        self._cache = (particles, velocities, np.zeros(len(particles)))
        self._count, self._count_known = len(particles), True

    def state_tensors(self, *, pressure: bool = True, ids: bool = False, sync: bool = True):
        """The state as torch CUDA tensors on the crate's device, without crossing to the host: ``(particles,
        velocities[, pressure][, ids])`` -- float64 (n, 2) twice, float64 (n,), int64 (n,) -- holding exactly what the
        `particles`, `particle_velocities` and `particles_pressure` attributes hold, in the same particle-index order,
        ranked and gathered on the GPU (sc_export_state_device).

        `sync=True` synchronises, reads the 8-byte count and returns views cut to n.  `sync=False` returns tensors of the
        context's capacity plus, last, the one-element int64 count tensor, and does not synchronise: rows from the count
        on are uninitialised.  The tensors are written on the library's stream, and the library's stream does not wait
        for torch's: read them after `synchronize()` -- or run the crate on torch's stream, `engine.set_stream`, and
        everything torch enqueues afterwards sees them."""
        import torch
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        room = eng.capacity
        out = [torch.empty((room, 2), dtype=torch.float64, device=dev), torch.empty((room, 2), dtype=torch.float64, device=dev),
               torch.empty(room, dtype=torch.float64, device=dev) if pressure else None,
               torch.empty(room, dtype=torch.int64, device=dev) if ids else None]
        count = torch.empty(1, dtype=torch.int64, device=dev)  # (always written; nothing of torch's touches the new tensors)
        if sync:  # (... unless their memory was freed with work still queued on torch's stream)
            torch.cuda.current_stream(dev).synchronize()
        eng.export_state(*out, count=count)
        if not sync:
            return (*(t for t in out if t is not None), count)
        eng.synchronize()
        n = int(count.item())
        self._count, self._count_known = n, True
        return tuple(t[:n] for t in out if t is not None)

    def load_state_tensors(self, particles, velocities, ids=None) -> None:
        """The device form of the `particles` / `particle_velocities` setters: float64 (n, 2) CUDA tensors -- and `ids`,
        int64 (n,), for particles that keep their identity, e.g. what `state_tensors(ids=True)` returned -- become the
        crate's state without crossing to the host (sc_import_state_device).  Pressures are zero until the next tick.
        The tensors are read on the library's stream, which does not wait for torch's: they must be ready when this is
        called (`torch.cuda.current_stream().synchronize()`, or run the crate on torch's stream, `engine.set_stream`)."""
        n = int(particles.shape[0]) if getattr(particles, "is_cuda", False) and particles.dim() == 2 else 0
        if n > self._engine.capacity:
            self._grow(n)
        self._engine.import_state(particles, velocities, ids)
        self._cache = None
        self._count, self._count_known = int(particles.shape[0]), True

    def _hand_rng_to_device(self) -> None:
        name, key, pos, _, _ = np.random.get_state()
        if name != "MT19937":
            raise RuntimeError("np.random is not the legacy MT19937 generator")
        self._engine.rng_set_state(key, pos)

    def sync_host_rng(self) -> None:
        """noise="host": bring ``np.random`` to where the device stream stands (synchronises).  The device keeps
        drawing from its own copy afterwards: call this before host code draws from the global generator, and
        `_hand_rng_to_device()` happens again on the next tick if the host state moved."""
        if self._noise == "host":
            key, pos = self._engine.rng_get_state()
            np.random.set_state(("MT19937", key, pos, 0, 0.0))
            self._host_rng_mark = (key.copy(), pos)

    def _fall_back_to_host_stream(self) -> None:
        """A particle source whose time step exceeds one half (binomial(n, p) with p > 0.5) is outside what the device
        draws of NumPy's legacy binomial (sc_rng.h: inversion and BTPE for 0 < p <= 0.5): from here on the host draws the
        stream -- same numbers, but two synchronisations per tick.  Said out loud, once."""
        import warnings
        warnings.warn("sand_crate_amd: a particle source draws binomial(n, p) with p > 0.5 -- not on the device; "
                      "physics_tick() falls back to noise='host-sync' (identical results, two host synchronisations per "
                      "tick) for the rest of this run", RuntimeWarning, stacklevel=3)
        self.sync_host_rng()
        self._noise = "host-sync"

    def _grow(self, needed: int) -> None:
        """A larger context takes the place of the one the state has outgrown, and the run goes on as if the crate had
        had the room from the start: a run does not depend on the capacity.  The state goes over through the old
        context's snapshot (sc_checkpoint_begin / sc_checkpoint_finish) -- particles and velocities with their ids, the
        tick number, the next id to hand out, the device's generator -- so counter noise, exported ids, the logs' tick
        numbers and the phase of `track(every=)` continue; noise mode and seed, the logs, and what the old engine was
        told (`Engine.adopt_settings`: stream, scan patience, timing, force monitor) are set again; HUD text and arrows
        are sent again with the next frame.  Pressures are not part of a snapshot: as after any upload they are zero
        until the next tick -- the callers grow right before one, or replace the state anyway.  `engine.timing()` counts
        the launches of the context that is there.  Costs a synchronisation and a copy of the state through the host."""
        old = self._engine
        pending = getattr(self, "_pending_checkpoint", None)
        if pending is not None and "snapshot" not in pending:  # begin_checkpoint's capture lives in the old context
            pending["snapshot"] = old.checkpoint_finish()
        old.checkpoint_begin()
        snap = old.checkpoint_finish()
        self._engine = Engine(int(needed * 1.5) + 1024, device=old.device)
        self._engine.set_noise_mode(_NOISE_MODES[self._noise], self._noise_seed)
        self._engine.adopt_settings(old)
        self._hud_sent = None  # (a new context has no HUD)
        self._arrows_sent = None  # (... and no arrows)
        if self._noise == "host" and snap["rng"] is not None:
            self._engine.rng_set_state(*snap["rng"])
        if getattr(self, "_observe", None) is not None:  # the log moves on: what the old context holds is kept
            self._observed.append(old.probe_read())
            self._engine.probe_enable(*self._observe)
        if getattr(self, "_track", None) is not None:  # ... and so does the log of frames
            self._tracked.append(self._read_track(old))
            self._engine.track_enable(*self._track)
        if getattr(self, "_trajectory", None) is not None:  # ... and the trajectory: same tensors, the words as they stand
            self._trajectory._move_to(self._engine)
        old.close()
        if len(snap["ids"]):
            self._engine.upload_with_ids(snap["particles"], snap["velocities"], snap["ids"])
        self._engine.restore_counters(snap["tick"], snap["next_id"])
        self._count, self._count_known = len(snap["ids"]), True
        self._cache = None

    # ------------------------------------------------------------------ the tick
    def physics_tick(self) -> None:
        t0 = time.perf_counter()
        self._create_new_particles()
        self.debug_arrows = []
        for body in self.rigid_bodies:  # crate.py:363-365
            body.apply_velocity(self.dt)
        eng = self._engine
        if self._noise == "host":    # the stream lives on the device: nothing comes back, nothing goes up --
            eng.tick(self._pack_tick_inputs())  # ... and the whole tick is one library call
            self._count_known = False
            self.last_stats = None
        elif self._noise == "host-sync":
            self._send_tick_inputs()
            eng.step_begin()
            stats = eng.step_stats()
            self.last_stats = stats
            if stats.flags & N.FLAG_SCAN_TIMEOUT:
                # the tick is abandoned (sc_step_stats): it has no lists, so nothing is drawn for it -- np.random stays
                # where it stands -- and the count is the one the crate had
                eng.set_noise_host(np.zeros((0, 2)))
                eng.step_finish()
            else:
                # crate.py:165-170 draws rand(C_i, 2) particle by particle; one block is the same stream
                eng.set_noise_host(np.random.rand(stats.neighbor_slots, 2))
                eng.step_finish()
                self._count, self._count_known = stats.particles, True
        else:
            eng.tick(self._pack_tick_inputs())
            self._count_known = False
        self._accelerate_free_bodies()
        self._cache = None
        self.tick += 1
        if self._hud_kernels:  # the HUD's phase split (timer.py:37-48), from HIP events; synchronises the tick
            eng.synchronize()
            for name, (ms, launches) in eng.timing().items():
                if launches:
                    self._kernel_seconds[name] = 0.9 * self._kernel_seconds.get(name, 0.0) + 0.1 * ms / 1000.0
            eng.reset_timing()
        if self._hud_forces:  # force_monitor.py:27-33: EMA (0.80) of the mean |dv| of each force phase
            sums, count = eng.force_monitor()
            if count:
                for name, total in zip(FORCE_PHASES, sums):
                    self._force_ema[name] = 0.8 * self._force_ema.get(name, 0.0) + 0.2 * total / count
        dt_wall = time.perf_counter() - t0
        self._tick_seconds = 0.9 * self._tick_seconds + 0.1 * dt_wall
        self._debug_prints = None  # crate.py:129 formats the HUD text every tick; here it is formatted when read

    def show_kernel_times(self, on: bool = True) -> None:
        """The reference's HUD splits the frame into its Python phases (crate.py:93-125 under
        `debug_timer`, reported by timer.py:37-48).  The phases are fused into kernels here; with this on,
        `physics_tick` brackets every launch with HIP events and `debug_prints` shows the same
        `Timing: {name: "x ms (y%)"}` block per kernel.  Costs one synchronisation per tick."""
        self._hud_kernels = bool(on)
        self._kernel_seconds = {}
        self._engine.reset_timing()
        self._engine.enable_timing(self._hud_kernels)

    def show_forces(self, on: bool = True) -> None:
        """The `Forces` block of the reference's HUD (force_monitor.py:35-37, printed at crate.py:135): mean |dv| of
        tension, gravity, pressure, viscosity, wall_bounce and continuous_collision, EMA 0.80, times 1000.  The force
        kernel sums |dv| per phase on the side (results unchanged); costs one synchronisation per tick."""
        self._hud_forces = bool(on)
        self._force_ema = {}
        self._engine.enable_force_monitor(self._hud_forces)

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
        if self._observe is not None:
            self._observed.append(self._engine.probe_read())
        if on:
            want = (int(capacity), int(bins), float(x_range[0]), float(x_range[1]))
            self._observe = None
            self._engine.probe_enable(*want)
            self._observe = want
        elif self._observe is not None:
            self._observe = None
            self._engine.probe_disable()

    def observations(self) -> dict:
        """What was logged since the last call, oldest first: a T-long float64 array per name of `probe.FIELDS`, `count`
        (T x bins, int32) and `top` (T x bins) when the log has bins, and `dropped`, the ticks that found the log
        full.  T = 0 when nothing was logged.  Synchronises.  (`tick` counts the ticks of the GPU context, and goes on
        counting when the crate had to grow into a larger one: `_grow`.)"""
        chunks, self._observed = self._observed, []
        if self._observe is not None:
            chunks.append(self._engine.probe_read())
        bins = self._observe[1] if self._observe is not None else (chunks[-1][1].shape[1] if chunks else 0)
        if any(c[1].shape[1] != bins for c in chunks):  # the bins changed between reads: the profiles of the last setting
            chunks = [c if c[1].shape[1] == bins else (c[0], np.zeros((len(c[0]), bins), dtype=np.int32),
                                                      np.full((len(c[0]), bins), np.inf), c[3]) for c in chunks]
        rows = np.concatenate([c[0] for c in chunks]) if chunks else np.zeros((0, len(FIELDS)))
        counts = np.concatenate([c[1] for c in chunks]) if chunks else np.zeros((0, bins), dtype=np.int32)
        tops = np.concatenate([c[2] for c in chunks]) if chunks else np.zeros((0, bins))
        return as_dict(rows, counts, tops, dropped=sum(c[3] for c in chunks))

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
        if self._track is not None:
            self._tracked.append(self._read_track(self._engine))
        if on:
            want = (int(every), int(capacity_bytes))
            self._track = None
            self._engine.track_enable(*want)
            self._track = want
        elif self._track is not None:
            self._track = None
            self._engine.track_disable()

    @staticmethod
    def _read_track(engine):
        blob, _, dropped = engine.track_read()
        return _track.split(blob), dropped

    def tracked(self) -> tuple[list[bytes], int]:
        """-> (the frames logged since the last call, oldest first; how many were dropped because the log was full).
        Synchronises.  (A frame's tick counts the ticks of the GPU context, and goes on counting when the crate had to
        grow into a larger one: `_grow`.)"""
        chunks, self._tracked = self._tracked, []
        if self._track is not None:
            chunks.append(self._read_track(self._engine))
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
        if initial:
            self._trajectory.capture()
        return self._trajectory

    def stop_trajectory(self) -> None:
        """Stops the recording `record_trajectory` started, if any, and synchronises: nothing is queued against its
        tensors afterwards."""
        traj, self._trajectory = getattr(self, "_trajectory", None), None
        if traj is not None:
            traj.stop()

    def close(self) -> None:
        """Stops a recording into torch's memory, then frees the GPU context."""
        try:
            self.stop_trajectory()
        finally:
            self._engine.close()

    # ------------------------------------------------------------------ frames (Playback.draw_scene, playback.py:75-85)
    def _set_hud(self, hud, width: int) -> None:
        """The `hud` argument of `render`, `render_jpeg` and `render_gif`: True draws `debug_prints` (what
        Playback.draw_debug_text shows, playback.py:215-219), a str draws that string, None or False nothing.  The text
        goes at the reference's margin in the built-in bitmap font, scaled for a frame this wide
        (hud_font.default_placement); characters outside ASCII become ``?``.  The engine is told only when the text or
        its placement changed since the last frame."""
        want = None
        if hud is not None and hud is not False:
            text = self.debug_prints if hud is True else hud
            if not isinstance(text, str):
                raise TypeError("hud must be None, a bool or a str")
            data = text.encode("ascii", "replace")
            if data:
                want = (data, *default_placement(width))
        if want != self._hud_sent:
            self._hud_sent = None
            if want is None:
                self._engine.set_hud(None)
            else:
                self._engine.set_hud(*want)
            self._hud_sent = want

    def _set_arrows(self, arrows, every: int, scale) -> None:
        """The `arrows`, `arrow_every` and `arrow_scale` arguments of `render`, `render_jpeg` and `render_gif`: the debug
        arrows of Playback.draw_debug_arrows (playback.py:95-107), green, over the walls and under the HUD text.  None or
        False draws none; True draws `debug_arrows`, the reference's list of (start, direction) in world units; an
        array-like K x 2 x 2 of (start, direction) is drawn the same way (`arrow_ends`: NaN entries dropped, the
        direction compressed on the host); "velocity" draws, without downloading anything, one arrow for every particle
        whose index is a multiple of `every`, along velocity * `scale` compressed the same way on the device -- `scale`
        defaults to `dt`, the step the particle is about to take.  Anything else is a TypeError.  The engine is told only
        when the request changed since the last frame."""
        want = None
        if arrows is None or arrows is False:
            pass
        elif isinstance(arrows, str):
            if arrows != "velocity":
                raise TypeError('arrows must be None, a bool, "velocity" or an array-like K x 2 x 2 of (start, direction)')
            want = ("velocity", float(self.dt if scale is None else scale), int(every))
        else:
            try:
                ends = arrow_ends(self.debug_arrows if arrows is True else arrows)
            except (TypeError, ValueError):
                raise TypeError('arrows must be None, a bool, "velocity" or an array-like K x 2 x 2 of (start, direction)') \
                    from None
            if len(ends):
                want = ("list", ends.tobytes())
        if want != getattr(self, "_arrows_sent", None):
            self._arrows_sent = None
            if want is None:
                self._engine.set_arrows(N.ARROWS_OFF)
            elif want[0] == "list":
                self._engine.set_arrows(N.ARROWS_LIST, np.frombuffer(want[1], dtype=np.float64))
            else:
                self._engine.set_arrows(N.ARROWS_VELOCITY, None, want[1], want[2])
            self._arrows_sent = want

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
        string (`_set_hud`); telling the engine a new text synchronises.  `arrows` draws the viewer's debug arrows
        between the walls and the text: True the list `debug_arrows`, an array of (start, direction) that, "velocity" one
        per `arrow_every`-th particle along its velocity times `arrow_scale` (`_set_arrows`).
        The pixel rule, bit for bit: tests/render_spec.py, tests/arrow_spec.py for the arrows and tests/text_spec.py for
        the text."""
        view = Engine.view(width, height, self.particle_radius, zoom=zoom, center=center, segment_width=segment_width)
        segments = self.segments if self.rigid_bodies else np.zeros((0, 2, 2))
        self._set_hud(hud, width)
        self._set_arrows(arrows, arrow_every, arrow_scale)
        return self._engine.render(view, segments, out)

    def render_jpeg(self, width: int = 1000, height: int = 1000, *, quality: int = 95, zoom: float = 1.0, center=None,
                    segment_width: int = 2, hud=None, arrows=None, arrow_every: int = 1, arrow_scale=None) -> bytes:
        """`render`'s frame as a JPEG file, encoded on the GPU: only the compressed bytes leave it.  Baseline JPEG, 4:4:4,
        the standard tables at `quality` (1..100; 95 is cv2's default, what the reference's AVI writer uses).  `hud`,
        `arrows`, `arrow_every` and `arrow_scale` as in `render`: text and arrows are on the frame before it is encoded.
        The bitstream, byte for byte: tests/jpeg_spec.py applied to `render`'s frame."""
        view = Engine.view(width, height, self.particle_radius, zoom=zoom, center=center, segment_width=segment_width)
        segments = self.segments if self.rigid_bodies else np.zeros((0, 2, 2))
        self._set_hud(hud, width)
        self._set_arrows(arrows, arrow_every, arrow_scale)
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
        view = Engine.view(width, height, self.particle_radius, zoom=zoom, center=center, segment_width=segment_width)
        segments = self.segments if self.rigid_bodies else np.zeros((0, 2, 2))
        self._set_hud(hud, width)
        self._set_arrows(arrows, arrow_every, arrow_scale)
        return self._engine.render_gif(view, segments)

    # ------------------------------------------------------------------ checkpoint (the reference's commented zarr dump,
    # playback.py:109-118, grown into something a run can resume from)
    def begin_checkpoint(self) -> None:
        """Capture the whole simulation state as of now.  Returns at once: the particle state is copied on the device
        and travels to pinned host memory on a side stream while later ticks run; `finish_checkpoint` collects it."""
        if self._pending_checkpoint is not None:
            raise RuntimeError("a checkpoint is already under way")
        self._engine.checkpoint_begin()
        bodies = []
        for body in self.rigid_bodies:
            bodies.append({"segments": body.segments.tolist(), "position": [float(x) for x in body.position],
                           "center_velocity": np.asarray(body.center_velocity, dtype=np.float64).tolist(),
                           "angular_clockwise_velocity": float(body.angular_clockwise_velocity),
                           "time_from_start": float(getattr(body, "time_from_start", 0.0))})
        coefficients = {}
        for name in self.editable_coefficients():
            value = getattr(self, name)
            coefficients[name] = value.tolist() if isinstance(value, np.ndarray) else value
        host_rng = None
        if self._noise != "host":  # the host owns the global stream (the device's copy travels with the particles)
            _, key, pos, has_gauss, cached = np.random.get_state()
            host_rng = {"key": key.tolist(), "pos": int(pos), "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}
        wc = self.world_config
        self._pending_checkpoint = {
            "format": 1, "tick": int(self.tick), "noise": self._noise, "noise_seed": int(self._noise_seed),
            "world_config": {"rigid_bodies": copy.deepcopy(wc.rigid_bodies), "particle_sources": copy.deepcopy(wc.particle_sources),
                             "coefficients": coefficients},
            "bodies": bodies, "host_rng": host_rng, "pressure": self._cache[2] if self._cache is not None else None}

    def finish_checkpoint(self, path) -> None:
        """Wait for the transfer `begin_checkpoint` started (not for later ticks) and write the .npz file."""
        if self._pending_checkpoint is None:
            raise RuntimeError("begin_checkpoint first")
        meta, self._pending_checkpoint = self._pending_checkpoint, None
        snap = meta.pop("snapshot", None)  # (collected already when the crate grew out of the context that took it)
        if snap is None:
            snap = self._engine.checkpoint_finish()
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
        crate._count, crate._count_known = n, True
        crate._cache = (arrays["particles"], arrays["velocities"], arrays.get("pressure", np.zeros(n)))
        if meta["noise"] == "host" and "rng_key" in arrays:
            eng.rng_set_state(arrays["rng_key"], meta["rng_pos"])
        elif meta["host_rng"] is not None:
            h = meta["host_rng"]
            np.random.set_state(("MT19937", np.array(h["key"], dtype=np.uint32), h["pos"], h["has_gauss"], h["cached_gaussian"]))
        return crate

    def run(self, n_ticks: int) -> None:
        """`n_ticks` ticks back to back without touching the host state in between (no sources
        may be active, noise must not be "host"): the throughput path bench.py measures."""
        if self._noise in ("host", "host-sync"):
            raise RuntimeError("Crate.run needs noise='counter' or 'none'")
        if any(src.active_ticks > self.tick for src in self.particle_sources):
            raise RuntimeError("Crate.run cannot interleave particle sources; use physics_tick()")
        if n_ticks <= 0:
            return
        eng = self._engine
        # One library call per tick (sc_tick).  Nobody can edit coefficients inside run(), so every tick
        # also promises the next tick's inputs and its removal / wall pass rides on this tick's force
        # kernel (sc_set_next_inputs); each tick's inputs are computed and packed once.
        for body in self.rigid_bodies:
            body.apply_velocity(self.dt)
        now = self._pack_tick_inputs()
        for k in range(n_ticks):
            nxt = None
            self._accelerate_free_bodies()  # this tick's gravity step on free bodies precedes the next tick's motion
            if k + 1 < n_ticks:
                for body in self.rigid_bodies:
                    body.apply_velocity(self.dt)
                nxt = self._pack_tick_inputs()
            eng.tick(now, nxt)
            self.tick += 1
            now = nxt
        self._cache = None
        self._count_known = False

    def _accelerate_free_bodies(self) -> None:
        """crate.py:311-314: gravity accelerates bodies that are neither fixed nor motored.  (Each body owns its
        velocity here; the reference's default `center_velocity` is one array shared by all bodies,
        rigid_body.py:21 -- INTEGRATION.md, deviations.)"""
        for body in self.rigid_bodies:
            if body.moves and not body.driven:
                body.center_velocity = body.center_velocity + self.dt * self.gravity

    def synchronize(self) -> None:
        self._engine.synchronize()

    def _create_new_particles(self) -> None:
        """crate.py:138-147: sources append in order, each seeing the count the previous left."""
        if self._noise == "host":
            active = [s for s in self.particle_sources if s.active_ticks > self.tick]
            if not active:
                return
            mark = getattr(self, "_host_rng_mark", None)
            if mark is not None:  # sync_host_rng() was used: has the host drawn from the stream since?
                _, key, pos, _, _ = np.random.get_state()
                if pos != mark[1] or not np.array_equal(key, mark[0]):
                    self._hand_rng_to_device()
                self._host_rng_mark = None
            try:
                self._engine.emit_particles(active, self.dt, int(self.max_particles))
                self._cache = None
                self._count_known = False
                return
            except N.NativeError as err:
                # (sc_emit_particles takes any number of sources: ERR_CAPACITY is the context's capacity)
                if err.code == N.ERR_CAPACITY:
                    self._grow(max(self._engine.capacity, int(self.max_particles)) + 1024)
                    self._engine.emit_particles(active, self.dt, int(self.max_particles))
                    self._cache = None
                    self._count_known = False
                    return
                if err.code != N.ERR_DOMAIN:
                    raise
                self._fall_back_to_host_stream()  # binomial(n, p) with p > 0.5: the host draws from here on
        for source in self.particle_sources:
            if source.active_ticks <= self.tick:
                continue
            new_p, new_v = source.generate_particles(dt=self.dt, max_particles=self.max_particles - self.particle_count)
            if new_p is not None:
                if self._count + len(new_p) > self._engine.capacity:
                    self._grow(self._count + len(new_p))
                self._engine.append(new_p, new_v)
                self._count += len(new_p)
                self._cache = None

    def _pack_tick_inputs(self):
        coef = {name: getattr(self, name) for name in _TICK_COEFFICIENTS}
        seg, pad, bodies = tick_geometry(self.rigid_bodies, self.particle_radius, self._pad_cache)
        return self._engine.pack_inputs(coef, self.gravity, seg, pad, bodies)

    def _send_tick_inputs(self) -> None:
        coef = {name: getattr(self, name) for name in _TICK_COEFFICIENTS}
        self._engine.set_params(gravity=self.gravity, **coef)
        bodies = self.rigid_bodies
        if bodies:
            seg = self.segments
            self._engine.set_segments(
                seg, pad_segments(seg, self.particle_radius),
                [(b.position, b.center_velocity, b.angular_clockwise_velocity, len(b)) for b in bodies])
        else:
            self._engine.set_segments(np.zeros((0, 2, 2)), np.zeros((0, 2, 2)), [])

    # ------------------------------------------------------------------ HUD text (crate.py:131-136)
    @property
    def debug_prints(self) -> str:
        """The HUD text the viewer draws every frame (playback.py:81).  Two YAML dumps: formatted on first read after a
        tick rather than in every tick, which is most of a small scene's tick time."""
        if self._debug_prints is None:
            self.set_debug_prints()
        return self._debug_prints

    @debug_prints.setter
    def debug_prints(self, text: str) -> None:
        self._debug_prints = text

    def set_debug_prints(self) -> None:
        count = self._count if self._count_known else "?"
        self.debug_prints = f"Tick: {self.tick}\nParticles: {count}\n"
        frame = self._tick_seconds
        timing = {"tick (host wall, EMA)": f"{1000 * frame:.2f} ms"}
        if self._hud_kernels and frame > 0:
            for name, seconds in self._kernel_seconds.items():
                timing[name] = f"{1000 * seconds:.3f} ms ({100 * seconds / frame:.0f}%)"
        self.debug_prints += yaml.dump({"Timing": timing,
                                        "FPS": f"{int(1 / frame) if frame > 0 else 0} ({1000 * frame:.0f} ms)"})
        if self._hud_forces:  # force_monitor.py:35-37, in the place crate.py:135 gives it
            rounded = {name: float(f"{1000 * value:.1f}") for name, value in self._force_ema.items()}
            self.debug_prints += f"\n\n{yaml.dump({'Forces': rounded})}"
        self.debug_prints += f"\n\n{self.get_coefficient_debug()}"

    def get_coefficient_debug(self) -> str:
        rows = []
        for name in self.editable_coefficients():
            val = getattr(self, name)
            rows.append({name: val.tolist() if isinstance(val, np.ndarray) else val})
        return yaml.dump(rows)

    def kernel_timing(self):
        return self._engine.timing()

    @property
    def engine(self) -> Engine:
        return self._engine
