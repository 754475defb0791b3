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
import functools
import json
import time

import numpy as np
import yaml

from . import _native as N
from .engine import Engine
from .hud_font import default_placement
from .load_config import WorldConfig
from .particle_source import build_particle_sources
from .probe import FIELDS, as_dict
from . import track as _track
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


def _point_rows(points) -> int:
    """The rows of a caller's (n, 2) tensor of points; what is no such tensor is left to the engine's check (0 rows)."""
    return int(points.shape[0]) if getattr(points, "is_cuda", False) and len(points.shape) == 2 else 0


_BATCH_ORDER = "batch offsets must start at 0, not descend and end at the number of points"


def _check_batch(who: str, device: int, points, queries, batch, query_batch) -> None:
    """The `batch=` / `query_batch=` arguments of a neighbourhood call: ValueError before anything is enqueued."""
    from .engine import _batch_tensor
    if batch is None:
        if query_batch is not None:
            raise ValueError(f"{who}: query_batch without batch")
        return
    if points is None:
        raise ValueError(f"{who}: batch needs points, the state is one cloud")
    entries = _batch_tensor(batch, "batch", device)
    if queries is None:
        if query_batch is not None:
            raise ValueError(f"{who}: query_batch without queries")
    elif query_batch is None:
        raise ValueError(f"{who}: queries of a batched call need query_batch, their clouds")
    else:
        _batch_tensor(query_batch, "query_batch", device, entries)


def _batch_keywords(method):
    """`batch=` and `query_batch=` for a method whose own parameter list stays as it is (`neighbor_tensors`: its list is
    part of the tested surface): the two keywords are taken here and wait in `self._batch_args` for the method, which
    reads them; `inspect.signature` shows the method's own list."""
    @functools.wraps(method)
    def call(self, *args, batch=None, query_batch=None, **kw):
        self._batch_args = (batch, query_batch)
        try:
            return method(self, *args, **kw)
        finally:
            self._batch_args = (None, None)
    return call


class Crate:
    _batch_args = (None, None)

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

    def pair_tensors(self, radius: float | None = None, *, points=None, half: bool = False, squared_distances: bool = False,
                     max_pairs: int | None = None, batch=None):
        """Which particles lie within `radius` (default: `diameter`) of which, as a CSR edge list in torch CUDA tensors on
        the crate's device, searched on the GPU (sc_pairs_count_device / sc_pairs_fill_device): ``(offsets, partners[, d2])``
        -- int64 (n + 1,), int64 (E,), float64 (E,).  Row i's partners are ``partners[offsets[i]:offsets[i + 1]]``, ascending;
        i and j are rows of `state_tensors()` at the same point of the stream, not ids.  (i, j) is a pair iff i != j and
        dx*dx + dy*dy <= radius*radius in separately rounded float64 (tests/pairs_spec.py); `half` keeps j > i only;
        `squared_distances` adds the number that was compared, per pair.  A particle with a coordinate that is not finite
        has no partners.  `points`, a float64 (n, 2) CUDA tensor, is searched instead of the state.  No cap on a row's
        length; `sand_crate_amd.pairs.edge_index` turns the result into a (2, E) tensor.

        By default the call synchronises once between counting and filling, reads n and E (16 bytes) and returns tensors
        cut to them; a coordinate with |c| / radius >= 2^31 raises ValueError.  With `max_pairs=K` nothing synchronises:
        `offsets` comes at capacity + 1 entries (n + 1 with `points`), `partners` and `d2` at K entries, and last the int64
        `counts` tensor (n, E): entries of `offsets` past n and of `partners` past min(E, K) are uninitialised, E > K means
        the list was clipped at K entries, E = -1 is the domain error (nothing else was written).  The tensors are written
        on the library's stream, and the library's stream does not wait for torch's: read them after `synchronize()`, and
        have `points` ready before the call -- or run the crate on torch's stream, `engine.set_stream`, and everything
        torch enqueues afterwards sees them.

        `batch`, an int64 CUDA tensor of B + 1 ascending offsets from 0 to n (`sand_crate_amd.pairs.batch_ptr` makes one
        from the clouds' sizes), makes `points` B disjoint clouds in one call -- the frames of a minibatch, which may
        overlap in space completely: cloud b is ``points[batch[b]:batch[b + 1]]``, a pair never crosses clouds, indices are
        global, and the result is, bit for bit, the per-cloud results concatenated with the partners shifted by
        ``batch[b]`` (tests/batch_spec.py).  Offsets that are not in order raise ValueError at the synchronisation
        (E = -3 with `max_pairs`)."""
        import torch
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(self.diameter if radius is None else radius)
        _check_batch("pair_tensors", eng.device, points, None, batch, None)
        rows = eng.capacity if points is None else _point_rows(points)
        offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        counts = torch.empty(2, dtype=torch.int64, device=dev)
        sync = max_pairs is None
        if sync:  # (nothing of torch's touches the new tensors, unless their memory was freed with work still queued)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=half, batch=batch)
        if sync:
            eng.synchronize()
            n, total = (int(v) for v in counts.cpu())
            if total == N.PAIRS_BATCH:
                raise ValueError(f"pair_tensors: {_BATCH_ORDER}")
            if total < 0:
                raise ValueError(f"pair_tensors: a coordinate lies outside the domain |c| / radius < 2^31 (radius {radius!r})")
            if points is None:
                self._count, self._count_known = n, True
        else:
            total = int(max_pairs)
            if total < 0:
                raise ValueError("max_pairs must not be negative")
        partners = torch.empty(total, dtype=torch.int64, device=dev)
        d2 = torch.empty(total, dtype=torch.float64, device=dev) if squared_distances else None
        eng.pairs_fill(partners, d2)
        if sync:
            eng.synchronize()
            return (offsets[:n + 1], partners) + ((d2,) if squared_distances else ())
        return (offsets, partners) + ((d2,) if squared_distances else ()) + (counts,)

    def cluster_tensors(self, radius: float | None = None, *, points=None, max_clusters: int | None = None):
        """What hangs together: the connected components of the graph `pair_tensors` defines at the same `radius` (default:
        `diameter`), labelled on the GPU from the pair search's grid (sc_pairs_count_device, then sc_pairs_label_device),
        as torch CUDA tensors on the crate's device: ``(labels, sizes, roots)`` -- int64 (n,), (C,), (C,).  ``labels[i]``
        is the cluster of row i of `state_tensors()` at the same point of the stream, or -1 for a particle with a
        coordinate that is not finite: it is in no cluster and bridges none.  Clusters are numbered 0..C-1 in ascending
        order of their smallest member, ``roots[c]``; ``sizes[c]`` is the member count (tests/cluster_spec.py is the
        rule; `sand_crate_amd.pairs.largest_cluster` and `cluster_size_of` read the result).  `points`, a float64 (n, 2)
        CUDA tensor, is labelled instead of the state.

        By default the call synchronises once, reads n and C (16 bytes) and returns tensors cut to them; a coordinate with
        |c| / radius >= 2^31 raises ValueError.  With `max_clusters=K` nothing synchronises: `labels` comes at capacity
        entries (n with `points`), `sizes` and `roots` at K entries, and last the int64 `counts` tensor (n, C): entries of
        `labels` past n and of `sizes` and `roots` past min(C, K) are uninitialised, C > K means that the clusters from K
        on were not written (`labels` is whole all the same), C = -1 is the domain error (nothing else was written).  The
        tensors are written on the library's stream, and the library's stream does not wait for torch's: read them after
        `synchronize()`, and have `points` ready before the call -- or run the crate on torch's stream,
        `engine.set_stream`, and everything torch enqueues afterwards sees them."""
        import torch
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(self.diameter if radius is None else radius)
        rows = eng.capacity if points is None else _point_rows(points)
        sync = max_clusters is None
        room = rows if sync else int(max_clusters)
        if room < 0:
            raise ValueError("max_clusters must not be negative")
        offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)  # (a temporary: the label reads the workspace)
        counts = torch.empty(2, dtype=torch.int64, device=dev)          # (n, E) of the count, then (n, C)
        labels = torch.empty(rows, dtype=torch.int64, device=dev)
        sizes = torch.empty(room, dtype=torch.int64, device=dev)
        roots = torch.empty(room, dtype=torch.int64, device=dev)
        if sync:  # (nothing of torch's touches the new tensors, unless their memory was freed with work still queued)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True)
        eng.pairs_label(labels, sizes, roots, counts=counts)
        if not sync:
            self._cluster_offsets = offsets  # (held until the next call: the count that writes it is still queued)
            return labels, sizes, roots, counts
        eng.synchronize()
        n, total = (int(v) for v in counts.cpu())
        if total < 0:
            raise ValueError(f"cluster_tensors: a coordinate lies outside the domain |c| / radius < 2^31 (radius {radius!r})")
        if points is None:
            self._count, self._count_known = n, True
        return labels[:n], sizes[:total], roots[:total]

    def cluster_sums(self, values, radius: float | None = None, *, points=None, extrema: bool = False,
                     max_clusters: int | None = None):
        """What each cluster carries: `cluster_tensors` at the same `radius` and `points`, and per cluster the sums --
        with `extrema` also the minima and maxima -- of `values` over its members, reduced on the GPU in one call (count,
        label, sc_pairs_cluster_sums_device): ``(labels, sizes, roots, sums[, mins, maxs])``, the last float64 (C, F).
        `values` is a float64 (n, F) or (n,) CUDA tensor, F 1 .. 8, whose rows are in the order of `state_tensors()` -- or
        of `points`; (n,) is one channel and still gives (C, 1).  A cluster's sum adds its members' values in ascending
        index, pairwise in groups of 64 and groups of groups, every add rounded on its own
        (tests/cluster_sums_spec.py is the rule): a pure function of the cluster's own members, the same bits on every
        call, no floating-point atomics anywhere.  A row with label -1 is never read, whatever its values are; a NaN among
        a cluster's values is that cluster's sum, minimum and maximum.  `sand_crate_amd.pairs.cluster_centers` and
        `cluster_mean_velocities` read the table of `cluster_observables`.

        Synchronisation and `max_clusters` are exactly those of `cluster_tensors`: by default one synchronisation, tensors
        cut to n and C, ValueError for a coordinate outside the domain and for `values` with fewer rows than there are
        points; with `max_clusters=K` nothing synchronises, the per-cluster tensors come at K rows and last the int64
        `counts` tensor (n, C): C > K means that the clusters from K on were not written, C = -1 is the domain error and
        C = -2 the short `values` (nothing else was written by the reduction).  `values` must be ready when this is
        called, as `points` must."""
        import torch
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(self.diameter if radius is None else radius)
        if not getattr(values, "is_cuda", False) or values.dtype != torch.float64 or values.dim() not in (1, 2):
            raise ValueError("values must be a CUDA float64 tensor of shape (n, F) or (n,)")
        values = (values.unsqueeze(1) if values.dim() == 1 else values).contiguous()
        width = int(values.shape[1])
        if not 1 <= width <= N.CLUSTER_SUMS_MAX_CHANNELS:
            raise ValueError(f"values must have 1 .. {N.CLUSTER_SUMS_MAX_CHANNELS} columns")
        rows = eng.capacity if points is None else _point_rows(points)
        sync = max_clusters is None
        room = rows if sync else int(max_clusters)
        if room < 0:
            raise ValueError("max_clusters must not be negative")
        offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)  # (a temporary: the label reads the workspace)
        counts = torch.empty(2, dtype=torch.int64, device=dev)          # (n, E) of the count, then (n, C) twice
        labels = torch.empty(rows, dtype=torch.int64, device=dev)
        sizes = torch.empty(room, dtype=torch.int64, device=dev)
        roots = torch.empty(room, dtype=torch.int64, device=dev)
        tables = tuple(torch.empty((room, width), dtype=torch.float64, device=dev) for _ in range(3 if extrema else 1))
        if sync:  # (what torch was asked for above is done, and nothing of torch's touches the new tensors)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True)
        eng.pairs_label(labels, sizes, roots, counts=counts)
        eng.pairs_cluster_sums(values, *tables, counts=counts)
        if not sync:
            self._cluster_sums_temporaries = (offsets, values)  # (held until the next call: still queued)
            return (labels, sizes, roots, *tables, counts)
        eng.synchronize()
        n, total = (int(v) for v in counts.cpu())
        if total == N.CLUSTER_SUMS_VALUES_SHORT:
            raise ValueError(f"cluster_sums: values has {values.shape[0]} rows, fewer than there are points")
        if total < 0:
            raise ValueError(f"cluster_sums: a coordinate lies outside the domain |c| / radius < 2^31 (radius {radius!r})")
        if points is None:
            self._count, self._count_known = n, True
        return (labels[:n], sizes[:total], roots[:total], *(t[:total] for t in tables))

    def cluster_observables(self, radius: float | None = None, *, max_clusters: int | None = None):
        """The probe's observables per droplet: ``(labels, roots, table)``, `table` float64 (C, 14) with the columns
        `sand_crate_amd.pairs.CLUSTER_FIELDS` -- n, sum_x, sum_y, sum_vx, sum_vy, sum_ke, sum_p, min_x, max_x, min_y,
        max_y, max_speed2, max_p, n_pressed, named as `probe.FIELDS` names them -- for every cluster of the state at
        `radius` (default: `diameter`).  The channels are built with torch from `state_tensors()` as the probe builds them,
        each operation rounded on its own and ``vx*vx + vy*vy`` evaluated once, so `max_speed2` and the kinetic energy
        agree; one `cluster_sums(..., extrema=True)` reduces them, with its synchronisation and `max_clusters` semantics
        (then `counts` comes last, and the table's rows from min(C, K) on are uninitialised).  Runs on torch's current
        stream and the crate's: with `max_clusters` the crate must be on torch's stream (`engine.set_stream`)."""
        import torch
        from .pairs import CLUSTER_FIELDS, cluster_channels
        if max_clusters is None:
            xy, vv, p = self.state_tensors()
        else:
            xy, vv, p, _ = self.state_tensors(sync=False)
        values = cluster_channels(xy, vv, p)
        out = self.cluster_sums(values, radius, extrema=True, max_clusters=max_clusters)
        labels, sizes, roots, sums, mins, maxs = out[:6]
        table = torch.empty((sums.shape[0], len(CLUSTER_FIELDS)), dtype=torch.float64, device=sums.device)
        table[:, 0] = sizes
        table[:, 1:7] = sums[:, 0:6]
        table[:, 7], table[:, 8], table[:, 9], table[:, 10] = mins[:, 0], maxs[:, 0], mins[:, 1], maxs[:, 1]
        table[:, 11], table[:, 12], table[:, 13] = maxs[:, 6], maxs[:, 5], sums[:, 7]
        return (labels, roots, table) + tuple(out[6:])

    @_batch_keywords
    def neighbor_tensors(self, k: int, radius: float | None = None, *, points=None, queries=None,
                         squared_distances: bool = False, partner_counts: bool = False, sync: bool = True):
        """The k nearest particles within `radius` (default: `diameter`) of every particle, as a table of fixed shape in
        torch CUDA tensors on the crate's device, selected on the GPU from the pair search's grid (sc_pairs_count_device,
        then sc_pairs_nearest_device): ``(neighbors[, d2][, partners])`` -- int64 (n, k), float64 (n, k), int64 (n,).
        ``neighbors[i]`` holds the partners of row i of `state_tensors()` at the same point of the stream -- the row of
        `pair_tensors` -- in ascending order of (squared distance, index), the nearest k of them, and -1 in the places
        behind (tests/nearest_spec.py is the rule; `sand_crate_amd.pairs.neighbor_mask` and `neighbor_edge_index` read the
        result).  `squared_distances` adds the numbers that were compared, +inf in the padding; `partner_counts` every
        row's number of partners without the cap, the row length of `pair_tensors`.  `points`, a float64 (n, 2) CUDA
        tensor, is searched instead of the state.  With `queries`, a float64 (q, 2) CUDA tensor, the rows are those points
        instead -- probes, sensors, the cursor: they need not be particles, and one that lies on a particle has it as a
        partner at distance 0 -- and the tensors have q rows.  `k` is 1 .. 64.

        The shape is known before anything runs, so nothing synchronises between counting and selecting.  `sync=True`
        synchronises once at the end, reads 16 bytes and returns tensors cut to the row count; a coordinate of a particle
        or a query with |c| / radius >= 2^31 raises ValueError.  `sync=False` synchronises nothing: the tensors come at
        capacity rows (n with `points`, q with `queries`) and last the int64 `counts` tensor (rows, cut): rows from the
        row count on are uninitialised, cut is the number of rows that had more than k partners, cut = -1 is the domain
        error (nothing else was written).  The tensors are written on the library's stream, and the library's stream does
        not wait for torch's: read them after `synchronize()`, and have `points` and `queries` ready before the call -- or
        run the crate on torch's stream, `engine.set_stream`, and everything torch enqueues afterwards sees them.

        `batch=` (a keyword of the wrapper around this method, `_batch_keywords`, as is `query_batch=`) makes `points` B
        disjoint clouds in one call, as in `pair_tensors`; with `queries` comes `query_batch`,
        also B + 1 offsets, from 0 to q: query rows ``query_batch[b]:query_batch[b + 1]`` see only the points of cloud b
        (a cloud may have points and no queries, or queries and no points).  Offsets that are not in order raise
        ValueError at the synchronisation (cut = -3 with `sync=False`)."""
        import torch
        k = int(k)
        if not 1 <= k <= N.NEAREST_MAX_K:
            raise ValueError(f"k must be 1 .. {N.NEAREST_MAX_K}")
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(self.diameter if radius is None else radius)
        batch, query_batch = self._batch_args
        _check_batch("neighbor_tensors", eng.device, points, queries, batch, query_batch)
        bound = eng.capacity if points is None else _point_rows(points)
        rows = bound if queries is None else _point_rows(queries)
        offsets = torch.empty(bound + 1, dtype=torch.int64, device=dev)  # (a temporary: the table reads the workspace)
        counts = torch.empty(2, dtype=torch.int64, device=dev)           # (n, E) of the count, then (rows, cut)
        neighbors = torch.empty((rows, k), dtype=torch.int64, device=dev)
        d2 = torch.empty((rows, k), dtype=torch.float64, device=dev) if squared_distances else None
        partners = torch.empty(rows, dtype=torch.int64, device=dev) if partner_counts else None
        out = tuple(t for t in (neighbors, d2, partners) if t is not None)
        if sync:  # (nothing of torch's touches the new tensors, unless their memory was freed with work still queued)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True, batch=batch)
        count_counts = counts
        if queries is not None:  # (the count's n stays readable: with queries the table's row count is q)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
        if query_batch is not None:
            eng.pairs_set_query_batch(query_batch)
        eng.pairs_nearest(neighbors, d2, partners, k=k, queries=queries, counts=counts)
        if not sync:
            self._neighbor_temporaries = (offsets, count_counts)  # (held until the next call: the count is still queued)
            return (*out, counts)
        eng.synchronize()
        n, cut = (int(v) for v in counts.cpu())
        if cut == N.PAIRS_BATCH:
            raise ValueError(f"neighbor_tensors: {_BATCH_ORDER} (of queries for query_batch)")
        if cut < 0:
            raise ValueError(f"neighbor_tensors: a coordinate of a point or a query lies outside the domain "
                             f"|c| / radius < 2^31 (radius {radius!r})")
        if points is None:
            self._count, self._count_known = (n if queries is None else int(count_counts[0])), True
        return tuple(t[:n] for t in out)

    def field_tensors(self, values=None, radius: float | None = None, *, power: int = 3, include_self: bool = True,
                      points=None, queries=None, weight_sums: bool = False, sync: bool = True, batch=None, query_batch=None):
        """What is there within `radius` (default: `diameter`) of every particle: the weighted sums of an SPH
        interpolation, as torch CUDA tensors on the crate's device, summed on the GPU over the pair search's grid
        (sc_pairs_count_device, then sc_pairs_sum_device): ``(sums[, wsum])`` -- float64 (n, C) and (n,).
        ``sums[i] = sum_j w_ij * values[j]`` over the partners j of row i of `state_tensors()` at the same point of the
        stream -- the row of `pair_tensors`, and with `include_self` particle i itself --, ``wsum[i] = sum_j w_ij``, with
        ``w = (1 - d2 / radius**2) ** power``, `power` 0 .. 3 (3: the poly6 shape; 0: w = 1, `wsum` counts the partners).
        The sums are added in ascending j, every operation rounded on its own: a pure function of the state, the same
        bits on every call (tests/field_spec.py is the rule; `sand_crate_amd.pairs.normalized` divides the two,
        `grid_queries` makes a raster of probes).  `values` is a float64 (n, C) or (n,) CUDA tensor whose rows are in the
        order of `state_tensors()` -- or of `points`, a float64 (n, 2) CUDA tensor that is searched instead of the state;
        it is made contiguous, any C is served, eight columns per launch against the same count, and (n,) gives sums of
        shape (n,).  With ``values=None`` only ``(wsum,)`` comes back: the density.  With `queries`, a float64 (q, 2) CUDA
        tensor, the rows are those points instead -- probes, sensors, the cell centres of an image: they need not be
        particles, a particle one lies on is a partner at distance 0, `include_self` means nothing -- and the tensors
        have q rows.  A particle or query with a coordinate that is not finite gives and gets nothing.

        The shape is known before anything runs, so nothing synchronises between counting and summing.  `sync=True`
        synchronises once at the end, reads 16 bytes and returns tensors cut to the row count; ValueError when a
        coordinate of a particle or a query has |c| / radius >= 2^31, and when `values` has fewer rows than there are
        particles.  `sync=False` synchronises nothing: the tensors come at capacity rows (n with `points`, q with
        `queries`) and last the int64 `counts` tensor (rows, status): rows from the row count on are uninitialised, status
        -1 is the domain error and -2 the short `values` (nothing else was written).  The tensors are written on the
        library's stream, and the library's stream does not wait for torch's: read them after `synchronize()`, and have
        `values`, `points` and `queries` ready before the call -- or run the crate on torch's stream, `engine.set_stream`,
        and everything torch enqueues afterwards sees them.  What the wrapper itself asks of torch -- the contiguous copy,
        the split into eights of more than 8 columns and their concatenation -- runs on torch's stream: with `sync=False`
        those need the crate on torch's stream.

        `batch` and `query_batch` make `points` (and `queries`) B disjoint clouds in one call, as in `neighbor_tensors`:
        the rows of `values` are global, a sum never crosses clouds.  Offsets that are not in order raise ValueError at the
        synchronisation (status -3 with `sync=False`)."""
        import torch
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(self.diameter if radius is None else radius)
        power = int(power)
        if not 0 <= power <= 3:
            raise ValueError("power must be 0 .. 3")
        _check_batch("field_tensors", eng.device, points, queries, batch, query_batch)
        flat = False
        if values is not None:
            if not getattr(values, "is_cuda", False) or values.dtype != torch.float64 or values.dim() not in (1, 2):
                raise ValueError("values must be a CUDA float64 tensor of shape (n, C) or (n,)")
            flat = values.dim() == 1
            values = (values.unsqueeze(1) if flat else values).contiguous()
            if values.shape[1] < 1:
                raise ValueError("values must have at least one column")
        step = N.FIELDS_MAX_CHANNELS
        width = 0 if values is None else int(values.shape[1])
        chunks = [values] if width <= step else [values[:, at:at + step].contiguous() for at in range(0, width, step)]
        bound = eng.capacity if points is None else _point_rows(points)
        rows = bound if queries is None else _point_rows(queries)
        offsets = torch.empty(bound + 1, dtype=torch.int64, device=dev)  # (a temporary: the sum reads the workspace)
        counts = torch.empty(2, dtype=torch.int64, device=dev)           # (n, E) of the count, then (rows, status)
        want_wsum = weight_sums or values is None
        wsum = torch.empty(rows, dtype=torch.float64, device=dev) if want_wsum else None
        parts = [None if v is None else torch.empty((rows, v.shape[1]), dtype=torch.float64, device=dev) for v in chunks]
        if sync:  # (what torch was asked for above is done, and nothing of torch's touches the new tensors)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True, batch=batch)
        count_counts = counts
        if queries is not None:  # (the count's n stays readable: with queries the sums' row count is q)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
        for at, (v, part) in enumerate(zip(chunks, parts)):  # (every launch consumes the query offsets: given each time)
            eng.pairs_sum(v, part, wsum if at == 0 else None, power=power, include_self=include_self, queries=queries,
                          counts=counts, query_batch=query_batch)
        if not sync:
            self._field_temporaries = (offsets, count_counts, chunks, parts)  # (held until the next call: still queued)
        else:
            eng.synchronize()
            n, status = (int(v) for v in counts.cpu())
            if status == N.PAIRS_BATCH:
                raise ValueError(f"field_tensors: {_BATCH_ORDER} (of queries for query_batch)")
            if status == N.FIELDS_DOMAIN:
                raise ValueError(f"field_tensors: a coordinate of a point or a query lies outside the domain "
                                 f"|c| / radius < 2^31 (radius {radius!r})")
            if status == N.FIELDS_VALUES_SHORT:
                raise ValueError(f"field_tensors: values has {values.shape[0]} rows, fewer than there are points")
            if points is None:
                self._count, self._count_known = (n if queries is None else int(count_counts[0])), True
        out = ()
        if values is not None:
            sums = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
            out = (sums.view(-1) if flat else sums,)
        if want_wsum:
            out += (wsum,)
        return (*out, counts) if not sync else tuple(t[:n] for t in out)

    def field_function(self, values=None, radius: float | None = None, *, power: int = 3, include_self: bool = True,
                       points=None, queries=None, weight_sums: bool = False, batch=None, query_batch=None):
        """`field_tensors(..., sync=True)` under torch autograd: the same arguments, the same results bit for bit, attached
        to the graph when `values`, `points` or `queries` requires grad -- `backward()` then gives their gradients from
        the same grid kernels (sc_pairs_sum_device with rows and partners swapped for the values,
        sc_pairs_sum_grad_device for the positions; tests/field_grad_spec.py is the rule).  When nothing requires grad it
        is `field_tensors` and nothing more.  Once differentiable; no gradient with respect to `radius`, no `sync=False`
        form; `batch` and `query_batch` as in `field_tensors`, and the backward passes them on:
        `sand_crate_amd.fields.field_function` has the details."""
        from .fields import field_function
        return field_function(self, values, radius, power=power, include_self=include_self, points=points, queries=queries,
                              weight_sums=weight_sums, batch=batch, query_batch=query_batch)

    def distance_histogram(self, edges, *, points=None, queries=None, per_row: bool = False, totals: bool = True,
                           sync: bool = True):
        """How far apart the particles are: the histogram of the pair distances over the bins `edges` delimits, as torch
        CUDA tensors on the crate's device, counted on the GPU over the pair search's grid (sc_pairs_count_device at the
        radius ``edges[-1]``, then sc_pairs_hist_device): ``([table, ]total)`` -- int32 (n, B) with `per_row`, int64 (B,)
        with `totals`.  `edges` is a host sequence or NumPy array of B + 1 float64 distances, B 1 .. 64, ``0 <= edges[0]
        < edges[1] < ...`` (`sand_crate_amd.pairs.shell_edges` makes equal-width ones).  ``table[i, b]`` is the number of
        partners j != i of row i of `state_tensors()` at the same point of the stream with ``edges[b]**2 <= d2 <
        edges[b + 1]**2``, the last bin closed on top, d2 the separately rounded float64 dx*dx + dy*dy of `pair_tensors`:
        the squares are compared, no square root is taken (tests/hist_spec.py is the rule).  ``total[b]`` is the sum of
        the column: it counts ORDERED pairs, each unordered pair twice (`sand_crate_amd.pairs.radial_distribution` turns
        it into g(r)).  Only integers are added: the same result on every call.  `points`, a float64 (n, 2) CUDA tensor,
        is searched instead of the state.  With `queries`, a float64 (q, 2) CUDA tensor, the rows are those points
        instead -- probes, sensors: they need not be particles, a particle one lies on is a partner at distance 0 --
        and the table has q rows.  A particle or query with a coordinate that is not finite gives and gets nothing.

        The shape is known before anything runs, so nothing synchronises between counting and binning.  `sync=True`
        synchronises once at the end, reads 16 bytes and returns the table cut to the row count; ValueError when a
        coordinate of a particle or a query has |c| / edges[-1] >= 2^31.  `sync=False` synchronises nothing: the table
        comes at capacity rows (n with `points`, q with `queries`) and last the int64 `counts` tensor (rows, status):
        rows from the row count on are uninitialised, status -1 is the domain error (nothing else was written).  The
        tensors are written on the library's stream, and the library's stream does not wait for torch's: read them
        after `synchronize()`, and have `points` and `queries` ready before the call -- or run the crate on torch's
        stream, `engine.set_stream`, and everything torch enqueues afterwards sees them."""
        import torch
        if not per_row and not totals:
            raise ValueError("neither per_row nor totals: nothing to return")
        e = np.array(edges, dtype=np.float64)
        bins = len(N.hist_squared_edges(e)) - 1
        if not e[-1] > 0:  # (never: the edges ascend from 0 or more)
            raise ValueError("the last edge must be positive")
        eng = self._engine
        dev = torch.device("cuda", eng.device)
        radius = float(e[-1])
        bound = eng.capacity if points is None else _point_rows(points)
        rows = bound if queries is None else _point_rows(queries)
        offsets = torch.empty(bound + 1, dtype=torch.int64, device=dev)  # (a temporary: the histogram reads the workspace)
        counts = torch.empty(2, dtype=torch.int64, device=dev)           # (n, E) of the count, then (rows, status)
        table = torch.empty((rows, bins), dtype=torch.int32, device=dev) if per_row else None
        total = torch.empty(bins, dtype=torch.int64, device=dev) if totals else None
        if sync:  # (nothing of torch's touches the new tensors, unless their memory was freed with work still queued)
            torch.cuda.current_stream(dev).synchronize()
        eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True)
        count_counts = counts
        if queries is not None:  # (the count's n stays readable: with queries the table's row count is q)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
        eng.pairs_hist(table, total, edges=e, queries=queries, counts=counts)
        if not sync:
            self._hist_temporaries = (offsets, count_counts)  # (held until the next call: the count is still queued)
            return (*(t for t in (table, total) if t is not None), counts)
        eng.synchronize()
        n, status = (int(v) for v in counts.cpu())
        if status == N.HIST_DOMAIN:
            raise ValueError(f"distance_histogram: a coordinate of a point or a query lies outside the domain "
                             f"|c| / radius < 2^31 (radius {radius!r})")
        if points is None:
            self._count, self._count_known = (n if queries is None else int(count_counts[0])), True
        return (() if table is None else (table[:n],)) + (() if total is None else (total,))

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
