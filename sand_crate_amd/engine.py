"""`Engine`: one GPU context of libsandcrate_hip.so with NumPy in/out.

This is the thinnest Python layer over the C ABI (include/sandcrate_hip.h); `Crate` (crate.py)
builds the reference's `Crate.physics_tick()` surface on top of it.  Device state stays resident
between ticks; nothing is copied back unless asked for.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass

import numpy as np

from . import _native as N


@dataclass
class StepStats:
    particles: int
    neighbor_slots: int
    max_neighbors: int
    wall_particles: int
    flags: int


_COEF_ORDER = ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
               "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure")


_BODY_FMT, _BODY_SIZE = "<5dii", C.sizeof(N.Body)
_PARAMS_FMT = f"<{len(_COEF_ORDER) + 2}d"
assert struct.calcsize(_BODY_FMT) == _BODY_SIZE and struct.calcsize(_PARAMS_FMT) == C.sizeof(N.Params)
assert N.TickInputs.params.offset == 0


def _pack_bodies(bodies):
    """-> (the sc_body array of `bodies`, an iterable of (position, center_velocity, omega, n_segments); how many)."""
    bodies = list(bodies)
    arr = (N.Body * max(len(bodies), 1))()
    # (packed straight into the C structs: this runs every tick, and a ctypes constructor per body and field costs
    # the host more than the GPU spends on a small scene's kernel)
    for k, (pos, vel, omega, nseg) in enumerate(bodies):
        struct.pack_into(_BODY_FMT, arr, _BODY_SIZE * k, pos[0], pos[1], vel[0], vel[1], omega, nseg, 0)
    return arr, len(bodies)


def _pack_params(coef, gravity, into=None) -> N.Params:
    """sc_params of the nine coefficients `coef` maps by name and the gravity, at the start of `into` or in a new one."""
    p = N.Params() if into is None else into
    struct.pack_into(_PARAMS_FMT, p, 0, *[coef[k] for k in _COEF_ORDER], gravity[0], gravity[1])
    return p


class PackedInputs:
    """sc_tick_inputs plus the NumPy buffers it points into (kept alive with it)."""

    __slots__ = ("struct", "ref", "_seg", "_pad", "_bodies")

    def __init__(self, coef, gravity, segments, padded, bodies):
        seg = N.f64(segments).reshape(-1, 2, 2)
        pad = N.f64(padded).reshape(-1, 2, 2)
        if len(pad) != 2 * len(seg):
            raise ValueError("padded must hold two segments per wall segment")
        t = N.TickInputs()
        _pack_params(coef, gravity, t)  # (params is the struct's first member)
        t.segments = N.dptr(seg)
        t.padded = N.dptr(pad)
        arr, t.n_bodies = _pack_bodies(bodies)
        t.bodies = arr
        t.n_segments = len(seg)
        self.struct, self.ref, self._seg, self._pad, self._bodies = t, C.byref(t), seg, pad, arr


def _state_tensor(t, name: str, dtype: str, tail: tuple, device: int, rows: int | None = None) -> int:
    """The number of rows of `t` once it is what the device state calls take: a contiguous CUDA tensor on `device` of
    this dtype and shape (rows, *tail).  ValueError otherwise -- before the library is touched, as `render(out=)` does."""
    want = f"{name} must be a contiguous CUDA {dtype} tensor of shape ({'N' if rows is None else rows}{''.join(f', {k}' for k in tail)}) on cuda:{device}"
    if not getattr(t, "is_cuda", False) or str(getattr(t, "dtype", None)) != f"torch.{dtype}" or not t.is_contiguous():
        raise ValueError(want)
    shape = tuple(t.shape)
    if len(shape) != 1 + len(tail) or shape[1:] != tuple(tail) or (rows is not None and shape[0] != rows):
        raise ValueError(want)
    if t.device.index != device:
        raise ValueError(want)
    return int(shape[0])


def _addresses(spare, *tensors) -> list:
    """The addresses of `tensors` for the library; None for None, which asks for the state or the self form, or says that
    an array is absent.  An empty tensor has no address: nothing is read or written there, so any address serves --
    `spare`'s."""
    return [None if t is None else N._P(t.data_ptr() if t.shape[0] else spare.data_ptr()) for t in tensors]


def _room(room, held: int, whose: str, unit: str = "rows") -> int:
    """`room` of a reader, by default all the `held` rows of its tensors; ValueError for more than they hold."""
    room = held if room is None else int(room)
    if room > held:
        raise ValueError(f"room {room} exceeds {whose} {held} {unit}")
    return room


def _ray_numbers(disc_radius, max_t, segments):
    """The host's numbers of `pairs_rays` and `pairs_ray_paths`, checked first -- they need no device --:
    -> (disc_radius, max_t, segments as float64 (S, 2, 2)).  ValueError otherwise."""
    disc_radius, max_t = float(disc_radius), float(max_t)
    if not (0 <= disc_radius < float("inf")):
        raise ValueError("disc_radius must be finite and not negative")
    if not (0 <= max_t < float("inf")):
        raise ValueError("max_t must be finite and not negative")
    seg = np.zeros((0, 2, 2)) if segments is None else np.ascontiguousarray(segments, dtype=np.float64)
    if seg.ndim != 3 or seg.shape[1:] != (2, 2) or len(seg) > N.MAX_SEGMENTS:
        raise ValueError(f"segments must be (S, 2, 2) with S at most {N.MAX_SEGMENTS}")
    return disc_radius, max_t, seg


def _counts_tensor(counts, device: int) -> None:
    _state_tensor(counts, "counts", "int64", (), device, 2)


def _query_rows(queries, device: int) -> int:
    """The rows of `queries`, float64 (q, 2), or 0 for None: the self form."""
    return 0 if queries is None else _state_tensor(queries, "queries", "float64", (2,), device)


def _batch_tensor(t, name: str, device: int, entries: int | None = None) -> int:
    """The entries of the offsets of a batched call, `batch` or `query_batch`: a contiguous 1-D int64 CUDA tensor on
    `device` of B + 1 >= 2 entries (`entries` of them when given).  ValueError otherwise, before the library is touched."""
    held = _state_tensor(t, name, "int64", (), device)
    if held < 2:
        raise ValueError(f"{name} must hold B + 1 offsets, B at least 1")
    if entries is not None and held != entries:
        raise ValueError(f"{name} has {held} entries, batch has {entries}: both count the same clouds")
    return held


class Engine:
    def __init__(self, capacity: int, device: int = 0):
        self._lib = N.load()
        self._ctx = N._P()
        N.check(self._lib.sc_create(int(device), int(capacity), C.byref(self._ctx)))
        self.capacity = int(capacity)
        self.device = int(device)
        # the settings a context is given and cannot be asked for: kept here, so that a context that replaces this one
        # can be given the same (`adopt_settings`; Crate._grow)
        self.stream = None            # the hipStream_t handed to `set_stream`, or None: the context's own stream
        self.scan_patience = None     # what `set_scan_patience` was given, or None: the library's default
        self.timing_on = False
        self.force_monitor_on = False
        # set on use: the host buffer `_fetch_bytes` keeps; (capacity, bins) of the log of observables while it is on; the
        # tensors of a recording while it runs and, stopped, until the next `synchronize()`
        self._fetch_buf = self._probe_log = self._traj_log = self._traj_retired = None

    def adopt_settings(self, other: "Engine") -> None:
        """The settings `other` was given become this context's: the stream, the scan's patience, timing and the force
        monitor.  (Noise mode, generator, HUD, arrows and the logs belong to their owner: crate.py.)"""
        if other.stream is not None:
            self.set_stream(other.stream)
        if other.scan_patience is not None:
            self.set_scan_patience(other.scan_patience)
        if other.timing_on:
            self.enable_timing(True)
        if other.force_monitor_on:
            self.enable_force_monitor(True)

    # -- lifetime
    def close(self) -> None:
        if self._ctx:
            self._lib.sc_destroy(self._ctx)
            self._ctx = N._P()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int) -> None:
        """Enqueue on this hipStream_t (0 = HIP's default stream), e.g. torch's current stream."""
        N.check(self._lib.sc_set_stream(self._ctx, N._P(int(stream_handle))))
        self.stream = int(stream_handle)

    def use_own_stream(self) -> None:
        N.check(self._lib.sc_use_own_stream(self._ctx))
        self.stream = None

    # -- state
    def upload(self, particles, velocities) -> None:
        p, v = N.f64(particles).reshape(-1, 2), N.f64(velocities).reshape(-1, 2)
        if p.shape != v.shape:
            raise ValueError("particles and velocities must both be P x 2")
        N.check(self._lib.sc_upload_state(self._ctx, N.dptr(p), N.dptr(v), len(p)))

    def upload_with_ids(self, particles, velocities, ids) -> None:
        """Slab mode: the particles this GPU owns, carrying their global ids."""
        p, v = N.f64(particles).reshape(-1, 2), N.f64(velocities).reshape(-1, 2)
        i = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if not (len(p) == len(v) == len(i)):
            raise ValueError("particles, velocities and ids must have one row per particle")
        N.check(self._lib.sc_upload_state_ids(self._ctx, N.dptr(p), N.dptr(v), N.i64ptr(i), len(p)))

    def append_with_ids(self, particles, velocities, ids) -> None:
        p, v = N.f64(particles).reshape(-1, 2), N.f64(velocities).reshape(-1, 2)
        i = np.ascontiguousarray(ids, dtype=np.int64).reshape(-1)
        if not (len(p) == len(v) == len(i)):
            raise ValueError("particles, velocities and ids must have one row per particle")
        N.check(self._lib.sc_append_particles_ids(self._ctx, N.dptr(p), N.dptr(v), N.i64ptr(i), len(p)))

    def append(self, particles, velocities) -> None:
        p, v = N.f64(particles).reshape(-1, 2), N.f64(velocities).reshape(-1, 2)
        N.check(self._lib.sc_append_particles(self._ctx, N.dptr(p), N.dptr(v), len(p)))

    def count(self) -> int:
        n = C.c_int64(0)
        N.check(self._lib.sc_count(self._ctx, C.byref(n)))
        return n.value

    def download(self, room: int | None = None):
        """-> particles (P,2), velocities (P,2), pressure (P,), ids (P,) in particle-index order."""
        room = self.capacity if room is None else int(room)
        xy = np.empty((room, 2))
        vxy = np.empty((room, 2))
        pr = np.empty(room)
        ids = np.empty(room, dtype=np.int64)
        n = C.c_int64(0)
        N.check(self._lib.sc_download_state(self._ctx, N.dptr(xy), N.dptr(vxy), N.dptr(pr), N.i64ptr(ids), room, C.byref(n)))
        k = n.value
        return xy[:k].copy(), vxy[:k].copy(), pr[:k].copy(), ids[:k].copy()

    # -- the state in torch's memory (sc_export_state_device / sc_import_state_device; the rule is tests/state_spec.py)
    def export_state(self, particles=None, velocities=None, pressure=None, ids=None, *, count, room: int | None = None):
        """`download()` into CUDA tensors, without the host: `particles` and `velocities` float64 (R, 2), `pressure`
        float64 (R,), `ids` int64 (R,) -- any of them None -- and `count`, int64 (1,), which receives n.  Rows 0..n-1 are
        written in particle-index order, the rest is left alone.  `room` defaults to R, the tensors' common row count (0
        without tensors).  Enqueued on the context's stream, no synchronisation: the library's stream does not wait for
        torch's, so the tensors must not be in use when this is called and are read after `synchronize()` (or run the
        engine on torch's stream, `set_stream`).  Returns `count`."""
        rows = None
        for t, name, dtype, tail in ((particles, "particles", "float64", (2,)), (velocities, "velocities", "float64", (2,)),
                                     (pressure, "pressure", "float64", ()), (ids, "ids", "int64", ())):
            if t is not None:
                rows = _state_tensor(t, name, dtype, tail, self.device, rows)
        _state_tensor(count, "count", "int64", (), self.device, 1)
        room = (rows or 0) if room is None else int(room)
        if rows is not None and room > rows:
            raise ValueError(f"room {room} exceeds the tensors' {rows} rows")
        ptr = lambda t: None if t is None else N._P(t.data_ptr())  # noqa: E731
        N.check(self._lib.sc_export_state_device(self._ctx, ptr(particles), ptr(velocities), ptr(pressure), ptr(ids), room,
                                                 ptr(count)))
        return count

    def import_state(self, particles, velocities, ids=None) -> None:
        """`upload` (ids None: particle i gets id i) or `upload_with_ids` from CUDA tensors, without the host: float64
        (n, 2) twice and int64 (n,).  The tensors are read on the context's stream, which does not wait for torch's:
        they must be ready when this is called.  With ids it synchronises once (the largest id comes back)."""
        n = _state_tensor(particles, "particles", "float64", (2,), self.device)
        _state_tensor(velocities, "velocities", "float64", (2,), self.device, n)
        if ids is not None:
            _state_tensor(ids, "ids", "int64", (), self.device, n)
        N.check(self._lib.sc_import_state_device(self._ctx, N._P(particles.data_ptr()), N._P(velocities.data_ptr()),
                                                 None if ids is None else N._P(ids.data_ptr()), n))

    # -- pair lists in torch's memory (sc_pairs_count_device / sc_pairs_fill_device; the rule is tests/pairs_spec.py)
    def pairs_set_batch(self, batch=None) -> None:
        """`batch`, an int64 CUDA tensor of B + 1 ascending offsets (0 .. n), cuts the points of the NEXT `pairs_count`
        into B clouds that see only themselves (sc_pairs_set_batch_device; tests/batch_spec.py is the rule); None clears a
        pending one.  The count consumes it and copies it on the context's stream: it must be ready then."""
        if batch is None:
            N.check(self._lib.sc_pairs_set_batch_device(self._ctx, None, 0))
            return
        entries = _batch_tensor(batch, "batch", self.device)
        N.check(self._lib.sc_pairs_set_batch_device(self._ctx, N._P(batch.data_ptr()), entries - 1))

    def pairs_set_query_batch(self, query_batch=None) -> None:
        """`query_batch`, an int64 CUDA tensor of B + 1 ascending offsets (0 .. q), gives the queries of the NEXT query-form
        reader of a batched grid their clouds (sc_pairs_set_query_batch_device); None clears a pending one.  The reader
        consumes it; its launches read it on the context's stream."""
        if query_batch is not None:
            _batch_tensor(query_batch, "query_batch", self.device)
        N.check(self._lib.sc_pairs_set_query_batch_device(self._ctx, None if query_batch is None else N._P(query_batch.data_ptr())))

    def _query_batch(self, queries, query_batch) -> None:
        if query_batch is None:
            return
        if queries is None:
            raise ValueError("query_batch without queries")
        self.pairs_set_query_batch(query_batch)

    def pairs_count(self, points=None, *, radius: float, offsets, counts, half: bool = False, room: int | None = None,
                    batch=None):
        """Counts the pairs within `radius` among `points`, a float64 (n, 2) CUDA tensor -- or with None among the state's
        particles in particle-index order -- into `offsets`, int64 (R + 1,): the exclusive scan of the row lengths, entries
        0..n.  `counts`, int64 (2,), receives n and E, the number of pairs (E = -1: a coordinate outside the domain
        |c| / radius < 2^31).  `half` keeps j > i only.  `room` defaults to R rows.  `batch`, an int64 CUDA tensor of
        B + 1 ascending offsets from 0 to n, makes the points B clouds that see only themselves (`pairs_set_batch`; needs
        `points`): the readers then read a batched grid -- the clusters, histograms and rays through `pairs_label_batch`,
        `pairs_hist_batch`, `pairs_rays_batch` and `pairs_ray_paths_batch` --, and E = -3 says that
        the offsets are not in order (nothing else is written).  Enqueued on the context's stream, no synchronisation,
        with the stream rules of `export_state`.  Returns `counts`."""
        n = 0 if points is None else _state_tensor(points, "points", "float64", (2,), self.device)
        if batch is not None:
            if points is None:
                raise ValueError("batch needs points: the state is one cloud")
            _batch_tensor(batch, "batch", self.device)
        rows = _state_tensor(offsets, "offsets", "int64", (), self.device) - 1
        _counts_tensor(counts, self.device)
        if rows < 0:
            raise ValueError("offsets must hold at least one entry")
        room = _room(room, rows, "the offsets'")
        radius = float(radius)
        if not (0.0 < radius < float("inf")):
            raise ValueError("radius must be finite and positive")
        self.pairs_set_batch(batch)  # (None: a batch left pending by hand does not reach this count)
        N.check(self._lib.sc_pairs_count_device(self._ctx, *_addresses(offsets, points), n, radius,
                                                N.PAIRS_HALF if half else 0, N._P(offsets.data_ptr()), room,
                                                N._P(counts.data_ptr())))
        return counts

    def pairs_fill(self, partners, d2=None, *, room: int | None = None):
        """Fills `partners`, int64 (K,), and `d2`, float64 (K,) or None, from the last `pairs_count`: row i's partners at
        offsets[i], ascending, and each pair's squared distance.  Entries from `room` (default K) on are left alone: a
        list longer than the room is clipped.  Enqueued on the context's stream, no synchronisation."""
        rows = _state_tensor(partners, "partners", "int64", (), self.device)
        if d2 is not None:
            _state_tensor(d2, "d2", "float64", (), self.device, rows)
        room = _room(room, rows, "the tensors'", "entries")
        N.check(self._lib.sc_pairs_fill_device(self._ctx, N._P(partners.data_ptr()),
                                               None if d2 is None else N._P(d2.data_ptr()), room))
        return partners

    def pairs_label(self, labels, sizes=None, roots=None, *, counts, room: int | None = None,
                    room_clusters: int | None = None):
        """Labels the clusters -- the connected components -- of the graph of the last `pairs_count`, whichever `half` it
        had (sc_pairs_label_device; the rule is tests/cluster_spec.py): `labels`, int64 (R,), receives every point's
        cluster, -1 for a point with a coordinate that is not finite; `sizes` and `roots`, int64 (K,) or None, each
        cluster's member count and smallest member; clusters are numbered 0..C-1 ascending in that member.  `counts`,
        int64 (2,), receives n and C (C = -1: the count found a coordinate outside the domain, nothing else is written).
        `room` defaults to R rows, `room_clusters` to K (0 without `sizes` and `roots`): clusters from it on are not
        written.  Refuses a batched grid: `pairs_label_batch` reads one.  Enqueued on the context's stream, no
        synchronisation.  Returns `counts`."""
        return self._label(labels, sizes, roots, None, counts, room, room_clusters)

    def pairs_label_batch(self, labels, sizes=None, roots=None, *, cluster_ptr, counts, room: int | None = None,
                          room_clusters: int | None = None):
        """`pairs_label` of a batched grid -- the last `pairs_count` had `batch` -- (sc_pairs_label_batch_device; the rule
        is tests/batch_readers_spec.py): a cluster never crosses clouds, labels and roots are global, and `cluster_ptr`,
        int64 (B + 1,), receives the offsets of the clouds into the clusters: cloud b's are
        ``cluster_ptr[b]:cluster_ptr[b + 1]``, always whole.  C = -3 says that the count's offsets were not in order
        (nothing else is written).  `pairs_cluster_sums` reads the label as any other.  Refuses an unbatched grid."""
        _state_tensor(cluster_ptr, "cluster_ptr", "int64", (), self.device)
        return self._label(labels, sizes, roots, cluster_ptr, counts, room, room_clusters)

    def _label(self, labels, sizes, roots, cluster_ptr, counts, room, room_clusters):
        rows = _state_tensor(labels, "labels", "int64", (), self.device)
        clusters = None
        for t, name in ((sizes, "sizes"), (roots, "roots")):
            if t is not None:
                clusters = _state_tensor(t, name, "int64", (), self.device, clusters)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the labels'")
        room_clusters = (clusters or 0) if room_clusters is None else int(room_clusters)
        if room_clusters > (clusters or 0):
            raise ValueError(f"room_clusters {room_clusters} exceeds the tensors' {clusters or 0} entries")
        labels_at, sizes_at, roots_at = _addresses(counts, labels, sizes, roots)
        if cluster_ptr is None:
            N.check(self._lib.sc_pairs_label_device(self._ctx, labels_at, room, sizes_at, roots_at, room_clusters,
                                                    N._P(counts.data_ptr())))
        else:
            N.check(self._lib.sc_pairs_label_batch_device(self._ctx, labels_at, room, sizes_at, roots_at, room_clusters,
                                                          N._P(cluster_ptr.data_ptr()), N._P(counts.data_ptr())))
        return counts

    def pairs_cluster_sums(self, values, sums, mins=None, maxs=None, *, counts, room_clusters: int | None = None):
        """What each cluster of the last `pairs_label` carries (sc_pairs_cluster_sums_device; the rule is
        tests/cluster_sums_spec.py): `sums`, float64 (K, F), receives per cluster the sum of `values[i, :]`, float64 (V, F)
        with F 1 .. 8, over the cluster's members i in ascending order, added pairwise in groups of 64 and groups of groups
        -- the same bits on every call --; `mins` and `maxs`, float64 (K, F) or None, the members' minima and maxima (a NaN
        wins).  A row with label -1 is never read.  `counts`, int64 (2,), receives n and C, or the status in its place:
        -1 when the count found a coordinate outside the domain, -2 when `values` has fewer rows than the count has
        points (then nothing else is written).  `room_clusters` defaults to K: clusters from it on are not written.
        Needs the label of the last `pairs_count`: a count in between is an error.  Enqueued on the context's stream, no
        synchronisation.  Returns `counts`."""
        if getattr(values, "is_cuda", False) and values.dim() == 2 and not 1 <= values.shape[1] <= N.CLUSTER_SUMS_MAX_CHANNELS:
            raise ValueError(f"values must be (points, F) with F 1 .. {N.CLUSTER_SUMS_MAX_CHANNELS}")
        channels = int(values.shape[1]) if getattr(values, "is_cuda", False) and values.dim() == 2 else 1
        held = _state_tensor(values, "values", "float64", (channels,), self.device)
        clusters = _state_tensor(sums, "sums", "float64", (channels,), self.device)
        for t, name in ((mins, "mins"), (maxs, "maxs")):
            if t is not None:
                _state_tensor(t, name, "float64", (channels,), self.device, clusters)
        _counts_tensor(counts, self.device)
        room_clusters = clusters if room_clusters is None else int(room_clusters)
        if room_clusters > clusters:
            raise ValueError(f"room_clusters {room_clusters} exceeds the tensors' {clusters} rows")
        values_at, *tables_at = _addresses(counts, values, sums, mins, maxs)
        N.check(self._lib.sc_pairs_cluster_sums_device(self._ctx, values_at, held, channels, *tables_at, room_clusters,
                                                       N._P(counts.data_ptr())))
        return counts

    def pairs_nearest(self, neighbors, d2=None, partners=None, *, k: int, queries=None, counts, room: int | None = None,
                      query_batch=None):
        """The nearest-k table of the last `pairs_count`, whichever `half` it had (sc_pairs_nearest_device; the rule is
        tests/nearest_spec.py): `neighbors`, int64 (R, k), receives per row the k nearest partners within the count's
        radius, ascending in (d2, j) and padded with -1; `d2`, float64 (R, k) or None, their squared distances, padded
        with +inf; `partners`, int64 (R,) or None, every row's number of partners without the cap.  The rows are the
        count's points, or with `queries`, a float64 (q, 2) CUDA tensor, those points of any kind: a query is not its own
        partner's rival, a point it coincides with is a partner at d2 = 0.  `counts`, int64 (2,), receives the row count
        and the number of rows with more than k partners (-1: a point or a query lies outside the domain, nothing else
        is written; -3: the offsets of a batched call are not in order).  `room` defaults to R rows.  On a batched grid
        `queries` come with `query_batch`, their B + 1 offsets (`pairs_set_query_batch`).  Enqueued on the context's stream,
        no synchronisation.  Returns `counts`."""
        k = int(k)
        if not 1 <= k <= N.NEAREST_MAX_K:
            raise ValueError(f"k must be 1 .. {N.NEAREST_MAX_K}")
        rows = _state_tensor(neighbors, "neighbors", "int64", (k,), self.device)
        if d2 is not None:
            _state_tensor(d2, "d2", "float64", (k,), self.device, rows)
        if partners is not None:
            _state_tensor(partners, "partners", "int64", (), self.device, rows)
        q = _query_rows(queries, self.device)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the table's")
        self._query_batch(queries, query_batch)
        queries_at, *table_at = _addresses(counts, queries, neighbors, d2, partners)
        N.check(self._lib.sc_pairs_nearest_device(self._ctx, queries_at, q, k, *table_at, room, N._P(counts.data_ptr())))
        return counts

    def pairs_sum(self, values=None, sums=None, wsum=None, *, power: int = 3, include_self: bool = True, queries=None,
                  counts, room: int | None = None, values_rows: int | None = None, query_batch=None):
        """The weighted sums over the partners of the last `pairs_count`, whichever `half` it had (sc_pairs_sum_device;
        the rule is tests/field_spec.py): `sums`, float64 (R, C), receives per row the sum of w * values[j, :] over its
        partners j within the count's radius, added in ascending j, and `wsum`, float64 (R,) or None, the sum of the
        weights w = (1 - d2 / radius^2) ** power, `power` 0 .. 3.  `values` is float64 (V, C), row j the values of point j
        of the count, C at most 8; with `values` and `sums` None only `wsum` is written.  The rows are the count's points
        -- `include_self`: point r is a partner of its own row -- or with `queries`, a float64 (q, 2) CUDA tensor, those
        points of any kind.  `counts`, int64 (2,), receives the row count and the status: 0, -1 when a point or a query
        lies outside the domain, -2 when `values` has fewer rows than the count has points (then nothing else is written).
        -3 says that the offsets of a batched call are not in order.  `room` defaults to R rows, `values_rows` to V.  On a
        batched grid `queries` come with `query_batch`, their B + 1 offsets (`pairs_set_query_batch`).  Enqueued on the
        context's stream, no synchronisation.  Returns `counts`."""
        power = int(power)
        if not 0 <= power <= 3:
            raise ValueError("power must be 0 .. 3")
        if (values is None) != (sums is None):
            raise ValueError("values and sums come together")
        if sums is None and wsum is None:
            raise ValueError("neither sums nor wsum to write")
        channels, rows = 0, None
        if values is not None:
            if values.dim() != 2 or not 1 <= values.shape[1] <= N.FIELDS_MAX_CHANNELS:
                raise ValueError(f"values must be (points, C) with C 1 .. {N.FIELDS_MAX_CHANNELS}")
            channels = int(values.shape[1])
            held = _state_tensor(values, "values", "float64", (channels,), self.device)
            values_rows = held if values_rows is None else int(values_rows)
            if not 0 <= values_rows <= held:
                raise ValueError(f"values_rows {values_rows} exceeds the values' {held} rows")
            rows = _state_tensor(sums, "sums", "float64", (channels,), self.device)
        if wsum is not None:
            rows = _state_tensor(wsum, "wsum", "float64", (), self.device, rows)
        q = _query_rows(queries, self.device)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the tensors'")
        self._query_batch(queries, query_batch)
        queries_at, values_at, sums_at, wsum_at = _addresses(counts, queries, values, sums, wsum)
        N.check(self._lib.sc_pairs_sum_device(self._ctx, queries_at, q, values_at, values_rows or 0, channels, power,
                                              N.FIELDS_SELF if include_self else 0, sums_at, wsum_at, room,
                                              N._P(counts.data_ptr())))
        return counts

    def pairs_sum_grad(self, grad, row_a=None, part_b=None, row_s=None, part_s=None, *, power: int = 3, queries=None,
                       counts, room: int | None = None, row_rows: int | None = None, part_rows: int | None = None,
                       query_batch=None):
        """The gradient of the weighted sums with respect to positions, over the partners of the last `pairs_count`
        (sc_pairs_sum_grad_device; the rule is `position_grad` of tests/field_grad_spec.py): `grad`, float64 (R, 2),
        receives per row ``k * sum_j s_rj * t_rj ** (power - 1) * (dx_rj, dy_rj)``, ``k = -2 * power / radius**2``,
        ``s_rj = row_s[r] + part_s[j] + row_a[r] . part_b[j]``, added in ascending j.  `row_a`, float64 (A, C), and
        `row_s`, float64 (A,), belong to the rows; `part_b`, float64 (B, C), and `part_s`, float64 (B,), to the count's
        points; C is at most 8, `row_a` and `part_b` come together, each of the four may be None.  The rows are the count's
        points -- a point is never its own partner here -- or with `queries`, a float64 (q, 2) CUDA tensor, those points.
        `counts`, int64 (2,), receives the row count and the status: 0, -1 when a point or a query lies outside the
        domain, -2 when the row arrays have fewer rows than there are rows or the partner arrays fewer than the count has
        points (then nothing else is written), -3 when the offsets of a batched call are not in order.  `room` defaults
        to R rows, `row_rows` to A, `part_rows` to B.  On a batched grid `queries` come with `query_batch`, their B + 1
        offsets (`pairs_set_query_batch`).  Enqueued on the context's stream, no synchronisation.  Returns `counts`."""
        power = int(power)
        if not 0 <= power <= 3:
            raise ValueError("power must be 0 .. 3")
        if (row_a is None) != (part_b is None):
            raise ValueError("row_a and part_b come together")
        rows = _state_tensor(grad, "grad", "float64", (2,), self.device)
        channels, held_a, held_b = 0, None, None
        if row_a is not None:
            if row_a.dim() != 2 or not 1 <= row_a.shape[1] <= N.FIELDS_MAX_CHANNELS:
                raise ValueError(f"row_a must be (rows, C) with C 1 .. {N.FIELDS_MAX_CHANNELS}")
            channels = int(row_a.shape[1])
            held_a = _state_tensor(row_a, "row_a", "float64", (channels,), self.device)
            held_b = _state_tensor(part_b, "part_b", "float64", (channels,), self.device)
        if row_s is not None:
            held_a = _state_tensor(row_s, "row_s", "float64", (), self.device, held_a)
        if part_s is not None:
            held_b = _state_tensor(part_s, "part_s", "float64", (), self.device, held_b)
        row_rows = (held_a or 0) if row_rows is None else int(row_rows)
        part_rows = (held_b or 0) if part_rows is None else int(part_rows)
        if not 0 <= row_rows <= (held_a or 0):
            raise ValueError(f"row_rows {row_rows} exceeds the row arrays' {held_a or 0} rows")
        if not 0 <= part_rows <= (held_b or 0):
            raise ValueError(f"part_rows {part_rows} exceeds the partner arrays' {held_b or 0} rows")
        q = _query_rows(queries, self.device)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the gradient's")
        self._query_batch(queries, query_batch)
        queries_at, a_at, b_at, row_s_at, part_s_at, grad_at = _addresses(counts, queries, row_a, part_b, row_s, part_s, grad)
        N.check(self._lib.sc_pairs_sum_grad_device(self._ctx, queries_at, q, a_at, row_rows, b_at, part_rows, channels,
                                                   row_s_at, part_s_at, power, grad_at, room, N._P(counts.data_ptr())))
        return counts

    def pairs_hist(self, table=None, total=None, *, edges, queries=None, counts, room: int | None = None):
        """The distance histogram over the partners of the last `pairs_count`, whichever `half` it had
        (sc_pairs_hist_device; the rule is tests/hist_spec.py): `table`, int32 (R, B) or None, receives per row the number
        of partners in each of the B bins, `total`, int64 (B,) or None, their sums over the rows -- in the self form
        ordered pairs, each unordered pair twice.  `edges` is a host sequence of B + 1 distances, B 1 .. 64, ``0 <=
        edges[0] < edges[1] < ...``, squared here in float64 (`_native.hist_squared_edges`); a partner at squared
        distance d2 is in bin b iff ``edges[b]**2 <= d2 < edges[b + 1]**2``, the last bin closed on top, and
        ``edges[-1]`` may be at most the count's radius.  The rows are the count's points -- a point is never its own
        partner -- or with `queries`, a float64 (q, 2) CUDA tensor, those points of any kind.  `counts`, int64 (2,),
        receives the row count and the status: 0, or -1 when a point or a query lies outside the domain (then nothing
        else is written).  `room` defaults to R rows (0 without a table).  Refuses a batched grid: `pairs_hist_batch`
        reads one.  Enqueued on the context's stream, no synchronisation.  Returns `counts`."""
        return self._hist(table, total, False, edges, queries, None, counts, room)

    def pairs_hist_batch(self, table=None, cloud_total=None, *, edges, queries=None, query_batch=None, counts,
                         room: int | None = None):
        """`pairs_hist` of a batched grid -- the last `pairs_count` had `batch` -- (sc_pairs_hist_batch_device; the rule is
        tests/batch_readers_spec.py): a row counts the partners of its own cloud only, `table` is as before and
        `cloud_total`, int64 (B, bins) or None, receives the column sums per cloud.  `queries` come with `query_batch`,
        their B + 1 offsets (`pairs_set_query_batch`).  Status -3 says that offsets were not in order (nothing else is
        written).  Refuses an unbatched grid."""
        return self._hist(table, cloud_total, True, edges, queries, query_batch, counts, room)

    def _hist(self, table, total, batched, edges, queries, query_batch, counts, room):
        e2 = N.hist_squared_edges(edges)
        bins = len(e2) - 1
        if table is None and total is None:
            raise ValueError("neither table nor total to write")
        rows = 0 if table is None else _state_tensor(table, "table", "int32", (bins,), self.device)
        clouds = 0
        if total is not None and batched:
            clouds = _state_tensor(total, "cloud_total", "int64", (bins,), self.device)
        elif total is not None:
            _state_tensor(total, "total", "int64", (), self.device, bins)
        q = _query_rows(queries, self.device)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the table's")
        queries_at, table_at, total_at = _addresses(counts, queries, table, total)
        if batched:
            self._query_batch(queries, query_batch)
            N.check(self._lib.sc_pairs_hist_batch_device(self._ctx, queries_at, q, N.dptr(e2), bins, table_at, total_at, room,
                                                         clouds, N._P(counts.data_ptr())))
        else:
            N.check(self._lib.sc_pairs_hist_device(self._ctx, queries_at, q, N.dptr(e2), bins, table_at, total_at, room,
                                                   N._P(counts.data_ptr())))
        return counts

    def pairs_rays(self, t, hit, *, origins, directions, disc_radius: float, max_t: float, segments=None, counts,
                   room: int | None = None):
        """Ray sensors over the points of the last `pairs_count` and a list of walls (sc_pairs_rays_device; the rule is
        tests/ray_spec.py): `t`, float64 (R,), receives per ray the parameter of the first thing it meets -- in units of
        the direction's length, +inf for nothing, NaN for a dead ray --, `hit`, int64 (R,), what that is: j >= 0 the disc
        of radius `disc_radius` round point j of the count, -2 - s wall s, -1 nothing.  `origins` and `directions` are
        float64 (q, 2) CUDA tensors with the same q; the directions are not normalised.  `disc_radius` may be at most
        half the count's radius, 0 looks at the walls alone; `max_t` is a finite host float >= 0.  `segments` is a host
        array (S, 2, 2), S at most 16, or None.  A wall wins a tie with a disc, the lower index a tie of two of a kind.
        `counts`, int64 (2,), receives the ray count and the status: 0, -1 when a point, an origin or a ray's end point
        ``origin + max_t * direction`` lies outside the domain, -4 when a ray would walk more than 8192 cells (then
        nothing else is written).  `room` defaults to R rows.  Refuses a batched grid: `pairs_rays_batch` reads one.
        Enqueued on the context's stream, no synchronisation.  Returns `counts`."""
        return self._rays("sc_pairs_rays_device", None, t, hit, (), origins, directions, disc_radius, max_t, segments,
                          counts, room)

    def pairs_rays_batch(self, t, hit, *, origins, directions, ray_batch, disc_radius: float, max_t: float, segments=None,
                         counts, room: int | None = None):
        """`pairs_rays` of a batched grid -- the last `pairs_count` had `batch` -- (sc_pairs_rays_batch_device; the rule is
        tests/batch_readers_spec.py): `ray_batch`, int64 (B + 1,), cuts the rays as `batch` cut the points
        (`pairs_set_query_batch`: the rays are queries), rays ``ray_batch[b]:ray_batch[b + 1]`` meet the discs of cloud b
        only, the walls are shared, and `hit` is the global row.  Status -3 says that offsets were not in order (nothing
        else is written).  Refuses an unbatched grid."""
        return self._rays("sc_pairs_rays_batch_device", ray_batch, t, hit, (), origins, directions, disc_radius, max_t,
                          segments, counts, room)

    def _rays(self, fn, ray_batch, t, hit, path, origins, directions, disc_radius, max_t, segments, counts, room):
        # `path`: () for the rays; (points, normals, end, bounces) for the ray paths, a row of L legs per ray then
        disc_radius, max_t, seg = _ray_numbers(disc_radius, max_t, segments)
        legs, bounces = (), ()
        if path:
            *path, bounces = path
            bounces = (int(bounces),)
            if not 0 <= bounces[0] <= N.RAY_MAX_BOUNCES:
                raise ValueError(f"bounces must be 0 .. {N.RAY_MAX_BOUNCES}")
            legs = (bounces[0] + 1,)
        rows = _state_tensor(t, "t", "float64", legs, self.device)
        _state_tensor(hit, "hit", "int64", legs, self.device, rows)
        if path:
            points, normals, end = path
            _state_tensor(points, "points", "float64", legs + (2,), self.device, rows)
            _state_tensor(normals, "normals", "float64", legs + (2,), self.device, rows)
            _state_tensor(end, "end", "int64", (), self.device, rows)
        q = _state_tensor(origins, "origins", "float64", (2,), self.device)
        _state_tensor(directions, "directions", "float64", (2,), self.device, q)
        _counts_tensor(counts, self.device)
        room = _room(room, rows, "the tensors'")
        origins_at, directions_at, *out_at = _addresses(counts, origins, directions, t, hit, *path)
        self._query_batch(origins, ray_batch)
        N.check(getattr(self._lib, fn)(self._ctx, origins_at, directions_at, q, *bounces, disc_radius, max_t,
                                       N.dptr(seg) if len(seg) else None, len(seg), *out_at, room, N._P(counts.data_ptr())))
        return counts

    def pairs_ray_paths(self, t, hit, points, normals, end, *, origins, directions, bounces: int, disc_radius: float,
                        max_t: float, segments=None, counts, room: int | None = None):
        """`pairs_rays` followed through `bounces` specular reflections, 0 .. 15 (sc_pairs_ray_paths_device; the rule is
        tests/ray_path_spec.py): L = bounces + 1 legs per ray.  `t`, float64 (R, L), and `hit`, int64 (R, L), are
        `pairs_rays`' per leg; `points` and `normals`, float64 (R, L, 2), receive the hit point and the surface normal
        there, facing the side the ray came from; `end`, int64 (R,), how the path ended: 0 every leg hit something, 1 a leg
        met nothing within what was left of `max_t` (t = +inf, hit = -1), 2 the ray or its next leg is dead or a normal is
        not finite, -1 and -4 the next leg fails the domain or the cap.  Legs a path never reached are t = NaN, hit = -1,
        NaN points and normals.  A leg >= 1 does not see what the leg before it hit, and a disc its origin lies in or on
        only when it heads inward.  `origins`, `directions`, `disc_radius`, `max_t` and `segments` as in `pairs_rays`.
        `counts`, int64 (2,), receives the ray count and the status of leg 0: 0, -1 or -4 as `pairs_rays` (then nothing
        else is written).  `room` defaults to R rows.  Refuses a batched grid: `pairs_ray_paths_batch` reads one.  Enqueued
        on the context's stream, no synchronisation.  Returns `counts`."""
        return self._rays("sc_pairs_ray_paths_device", None, t, hit, (points, normals, end, bounces), origins, directions,
                          disc_radius, max_t, segments, counts, room)

    def pairs_ray_paths_batch(self, t, hit, points, normals, end, *, origins, directions, ray_batch, bounces: int,
                              disc_radius: float, max_t: float, segments=None, counts, room: int | None = None):
        """`pairs_ray_paths` of a batched grid (sc_pairs_ray_paths_batch_device): `ray_batch` and everything about the
        clouds as in `pairs_rays_batch`; every leg of a path stays in its ray's cloud."""
        return self._rays("sc_pairs_ray_paths_batch_device", ray_batch, t, hit, (points, normals, end, bounces), origins,
                          directions, disc_radius, max_t, segments, counts, room)

    # -- frames
    @staticmethod
    def view(width: int, height: int, particle_radius: float, *, zoom: float = 1.0, center=None,
             segment_width: int = 2) -> N.View:
        """sc_view; `center` defaults to the frame's centre (width/2, height/2), as the reference's viewer has it."""
        cx, cy = (width / 2, height / 2) if center is None else (float(center[0]), float(center[1]))
        return N.View(int(width), int(height), float(zoom), cx, cy, float(particle_radius), int(segment_width), 0)

    def render(self, view: N.View, segments, out=None):
        """The RGB frame (height x width x 3 uint8) of the current device state with these walls (S x 2 x 2).
        out=None: synchronises and returns a NumPy array (sc_render).  `out` a CUDA uint8 tensor of that shape: enqueued
        on the context's stream into it (sc_render_device), no synchronisation; returns `out`."""
        seg = N.f64(segments).reshape(-1, 2, 2)
        shape = (int(view.height), int(view.width), 3)
        if out is None:
            img = np.empty(shape, dtype=np.uint8)
            N.check(self._lib.sc_render(self._ctx, C.byref(view), N.dptr(seg), len(seg), N._P(img.ctypes.data)))
            return img
        if not getattr(out, "is_cuda", False) or tuple(out.shape) != shape or not out.is_contiguous() or \
                str(out.dtype) != "torch.uint8":
            raise ValueError(f"out must be a contiguous CUDA uint8 tensor of shape {shape}")
        N.check(self._lib.sc_render_device(self._ctx, C.byref(view), N.dptr(seg), len(seg), N._P(out.data_ptr())))
        return out

    def _fetch_bytes(self, call, guess: int) -> bytes:
        """Runs call(out, room, n_out) -- an encoder, or a reader of tracked frames -- into a host buffer kept between
        calls, of at least `guess` bytes, and once more into a larger one when the library asks for more than it holds."""
        buf = self._fetch_buf
        if buf is None or len(buf) < guess:
            buf = self._fetch_buf = np.empty(max(int(guess), 1), dtype=np.uint8)
        n = C.c_int64(0)
        rc = call(N._P(buf.ctypes.data), len(buf), C.byref(n))
        if rc == N.ERR_CAPACITY and n.value > len(buf):
            buf = self._fetch_buf = np.empty(n.value, dtype=np.uint8)
            rc = call(N._P(buf.ctypes.data), len(buf), C.byref(n))
        N.check(rc)
        return buf[:n.value].tobytes()

    @staticmethod
    def _frame_guess(width: int, height: int) -> int:
        return 3 * width * height + 4096  # (a frame's raw size: enough for all but noise)

    def encode_jpeg(self, rgb, quality: int = 95) -> bytes:
        """The JPEG file (sc_jpeg_encode_device) of an H x W x 3 uint8 RGB image: a contiguous CUDA tensor, which must
        be ready on the library's stream (torch's current stream is synchronised first), or a NumPy array, which is
        uploaded.  Synchronises.  The bitstream, byte for byte: tests/jpeg_spec.py."""
        import torch
        if isinstance(rgb, np.ndarray):
            rgb = torch.from_numpy(np.ascontiguousarray(rgb)).to(f"cuda:{self.device}")
        if not getattr(rgb, "is_cuda", False) or rgb.dim() != 3 or rgb.shape[2] != 3 or not rgb.is_contiguous() or \
                str(rgb.dtype) != "torch.uint8":
            raise ValueError("rgb must be a contiguous H x W x 3 uint8 CUDA tensor or NumPy array")
        torch.cuda.current_stream(rgb.device).synchronize()  # (the library's stream does not wait for torch's)
        h, w = int(rgb.shape[0]), int(rgb.shape[1])
        ptr = N._P(rgb.data_ptr())
        return self._fetch_bytes(lambda out, cap, n: self._lib.sc_jpeg_encode_device(self._ctx, ptr, w, h, int(quality), out,
                                                                                     cap, n), self._frame_guess(w, h))

    def render_jpeg(self, view: N.View, segments, quality: int = 95) -> bytes:
        """The frame `render` draws, encoded as `encode_jpeg` does, without leaving the GPU before it is compressed
        (sc_render_jpeg).  Synchronises."""
        seg = N.f64(segments).reshape(-1, 2, 2)
        return self._fetch_bytes(lambda out, cap, n: self._lib.sc_render_jpeg(self._ctx, C.byref(view), N.dptr(seg), len(seg),
                                                                              int(quality), out, cap, n),
                                 self._frame_guess(int(view.width), int(view.height)))

    def encode_gif(self, index) -> bytes:
        """The image data of one GIF frame (sc_gif_encode_device; `gif.GifWriter.write` takes it) of an H x W uint8 image
        of palette indices -- entry 0 is black, entry k is (k, k, 255): a contiguous CUDA tensor, which must be ready on
        the library's stream (torch's current stream is synchronised first), or a NumPy array, which is uploaded.
        Synchronises.  The bitstream, byte for byte: tests/gif_spec.py."""
        import torch
        if isinstance(index, np.ndarray):
            index = torch.from_numpy(np.ascontiguousarray(index)).to(f"cuda:{self.device}")
        if not getattr(index, "is_cuda", False) or index.dim() != 2 or not index.is_contiguous() or \
                str(index.dtype) != "torch.uint8":
            raise ValueError("index must be a contiguous H x W uint8 CUDA tensor or NumPy array")
        torch.cuda.current_stream(index.device).synchronize()  # (the library's stream does not wait for torch's)
        h, w = int(index.shape[0]), int(index.shape[1])
        ptr = N._P(index.data_ptr())
        return self._fetch_bytes(lambda out, cap, n: self._lib.sc_gif_encode_device(self._ctx, ptr, w, h, out, cap, n),
                                 self._frame_guess(w, h))

    def render_gif(self, view: N.View, segments) -> bytes:
        """The frame `render` draws as palette indices (background 0, a wall 255, a disc of colour byte c max(c, 1): the
        one loss is that (0, 0, 255) becomes (1, 1, 255); while arrows are set an arrow is 1 and a disc max(c, 2)), encoded as `encode_gif` does without leaving the GPU before it
        is compressed (sc_render_gif).  Synchronises."""
        seg = N.f64(segments).reshape(-1, 2, 2)
        return self._fetch_bytes(lambda out, cap, n: self._lib.sc_render_gif(self._ctx, C.byref(view), N.dptr(seg), len(seg),
                                                                             out, cap, n),
                                 self._frame_guess(int(view.width), int(view.height)))

    def set_hud(self, text: bytes | None, x: int = 6, y: int = 6, scale: int = 1) -> None:
        """From now on every frame of `render`, `render_jpeg` and `render_gif` carries `text` in white over the discs and
        walls: lines split at ``\\n``, the first at pixel (x, y), in the built-in 8 x 16 bitmap font (hud_font.py) with
        every glyph bit `scale` x `scale` pixels; bytes outside ASCII 0x20..0x7E are drawn as ``?``.  None or b"" clears
        it.  Synchronises (sc_set_hud).  The pixel rule, bit for bit: tests/text_spec.py."""
        data = bytes(text) if text else b""
        N.check(self._lib.sc_set_hud(self._ctx, data if data else None, len(data), int(x), int(y), int(scale)))

    def set_arrows(self, mode: int, arrows=None, scale: float = 1.0, every: int = 1) -> None:
        """From now on every frame of `render`, `render_jpeg` and `render_gif` carries debug arrows in green, over the
        discs and walls and under the HUD text (sc_set_arrows).  `mode` N.ARROWS_LIST: `arrows`, K x 2 x 2 of (start, end)
        in world units, at most N.MAX_ARROWS of them.  N.ARROWS_VELOCITY: one arrow per live particle whose id is a
        multiple of `every`, from its position along velocity * `scale`, compressed as playback.py:99 does, all on the
        device.  N.ARROWS_OFF: none.  Synchronises.  The pixel rule, bit for bit: tests/arrow_spec.py."""
        a = None if arrows is None else N.f64(arrows).reshape(-1, 4)
        n = 0 if a is None else len(a)
        ptr = None if n == 0 else C.cast(a.ctypes.data, C.POINTER(N.Arrow))
        N.check(self._lib.sc_set_arrows(self._ctx, int(mode), ptr, n, float(scale), int(every)))

    # -- per-tick inputs
    def set_params(self, *, dt, particle_radius, wall_collision_decay, pressure_amplifier, ignored_pressure,
                   collider_noise_level, viscosity, surface_smoothing, target_pressure, gravity) -> None:
        named = locals()  # (the nine coefficients by name, as _pack_params takes them)
        p = _pack_params(named, np.asarray(gravity, dtype=np.float64).reshape(2))
        N.check(self._lib.sc_set_params(self._ctx, C.byref(p)))

    def set_segments(self, segments, padded, bodies) -> None:
        """segments (S,2,2); padded (2S,2,2); bodies: iterable of (position, center_velocity, omega, n_segments)."""
        seg = N.f64(segments).reshape(-1, 2, 2)
        pad = N.f64(padded).reshape(-1, 2, 2)
        if len(pad) != 2 * len(seg):
            raise ValueError("padded must hold two segments per wall segment")
        arr, n_bodies = _pack_bodies(bodies)
        N.check(self._lib.sc_set_segments(self._ctx, N.dptr(seg), N.dptr(pad), len(seg), arr, n_bodies))

    def set_next_inputs(self, *, gravity, segments, bodies, **coef) -> None:
        """Promise the inputs of the next tick (between step_begin and step_finish); see the header."""
        p = _pack_params(coef, np.asarray(gravity, dtype=np.float64).reshape(2))
        seg = N.f64(segments).reshape(-1, 2, 2)
        arr, n_bodies = _pack_bodies(bodies)
        N.check(self._lib.sc_set_next_inputs(self._ctx, C.byref(p), N.dptr(seg), len(seg), arr, n_bodies))

    def pack_inputs(self, coef, gravity, segments, padded, bodies) -> "PackedInputs":
        """The inputs of one tick as one C struct (sc_tick_inputs): `coef` maps the nine per-tick coefficient
        names to values, `bodies` is an iterable of (position, center_velocity, omega, n_segments)."""
        return PackedInputs(coef, gravity, segments, padded, bodies)

    def tick(self, now: "PackedInputs", nxt: "PackedInputs | None" = None) -> None:
        """One whole tick in one library call (sc_tick); `nxt` promises the next tick's inputs."""
        N.check(self._lib.sc_tick(self._ctx, now.ref, nxt.ref if nxt is not None else None))

    def set_noise_mode(self, mode: int, seed: int = 0) -> None:
        N.check(self._lib.sc_set_noise_mode(self._ctx, int(mode), int(seed) & (2 ** 64 - 1)))

    # -- the tick
    def step_begin(self) -> None:
        N.check(self._lib.sc_step_begin(self._ctx))

    def step_stats(self) -> StepStats:
        s = N.Stats()
        N.check(self._lib.sc_step_stats(self._ctx, C.byref(s)))
        return StepStats(s.particles, s.neighbor_slots, s.max_neighbors, s.wall_particles, s.flags)

    def set_noise_host(self, u01) -> None:
        u = N.f64(u01).reshape(-1, 2)
        N.check(self._lib.sc_set_noise_host(self._ctx, N.dptr(u), len(u)))

    def step_finish(self) -> None:
        N.check(self._lib.sc_step_finish(self._ctx))

    def step(self, n_ticks: int = 1) -> None:
        N.check(self._lib.sc_step(self._ctx, int(n_ticks)))

    def synchronize(self) -> None:
        N.check(self._lib.sc_synchronize(self._ctx))
        self._traj_retired = None  # (nothing is queued any more against the tensors of a recording that was stopped)

    def set_scan_patience(self, polls: int) -> None:
        """How often a workgroup of the bucket scan asks for a predecessor's total before the tick is abandoned
        (sc_set_scan_patience; negative: at once -- the path's test)."""
        N.check(self._lib.sc_set_scan_patience(self._ctx, int(polls)))
        self.scan_patience = int(polls)

    # -- parity taps (between step_begin and step_finish)
    def download_sort(self):
        room = self.capacity
        rows = np.empty(room, dtype=np.int64)
        ids = np.empty(room, dtype=np.int64)
        n = C.c_int64(0)
        N.check(self._lib.sc_download_sort(self._ctx, N.i64ptr(rows), N.i64ptr(ids), room, C.byref(n)))
        return rows[:n.value].copy(), ids[:n.value].copy()

    def download_neighbors(self):
        """-> ids (P,), counts (P,), neighbor ids (P,20), fixed positions (P,2); one row per sorted slot."""
        room = self.capacity
        ids = np.empty(room, dtype=np.int64)
        cnt = np.empty(room, dtype=np.int32)
        nb = np.empty((room, N.MAX_NEIGHBORS), dtype=np.int64)
        fx = np.empty((room, 2))
        n = C.c_int64(0)
        N.check(self._lib.sc_download_neighbors(self._ctx, N.i64ptr(ids), N.i32ptr(cnt), N.i64ptr(nb), N.dptr(fx), room,
                                                C.byref(n)))
        k = n.value
        return ids[:k].copy(), cnt[:k].copy(), nb[:k].copy(), fx[:k].copy()

    def download_normals(self):
        room = self.capacity
        s = np.empty((room, 2))
        n = C.c_int64(0)
        N.check(self._lib.sc_download_normals(self._ctx, N.dptr(s), room, C.byref(n)))
        return s[:n.value].copy()

    def download_pressure(self):
        """-> the finished tick's pressures in id order, one per particle it had -- the rows it left NaN included."""
        room = self.capacity
        pr = np.empty(room)
        n = C.c_int64(0)
        N.check(self._lib.sc_download_pressure(self._ctx, N.dptr(pr), room, C.byref(n)))
        return pr[:n.value].copy()

    # -- multi-GPU slabs (device pointers are plain integers, e.g. torch_tensor.data_ptr())
    def set_slab(self, col_lo: int, col_hi: int, halo: int, has_left: bool, has_right: bool) -> None:
        N.check(self._lib.sc_set_slab(self._ctx, int(col_lo), int(col_hi), int(halo), int(has_left), int(has_right)))

    def set_band_flag(self, on: bool) -> None:
        """Halo overlap with slabs of rows: one launch of the force kernel + a polling kernel on the side stream
        (sc_set_band_flag) instead of two launches."""
        N.check(self._lib.sc_set_band_flag(self._ctx, int(bool(on))))

    def set_slab_axis(self, axis: int) -> None:
        """0: slabs are ranges of columns floor(x / d) (the default); 1: of rows floor(y / d)."""
        N.check(self._lib.sc_set_slab_axis(self._ctx, int(axis)))

    def halo_pack(self, dev_left: int, dev_right: int, capacity_records: int) -> None:
        N.check(self._lib.sc_halo_pack(self._ctx, N._P(dev_left), N._P(dev_right), int(capacity_records)))

    def halo_sizes(self, capacity_records: int) -> tuple[int, int, int, int]:
        """-> records to (send left, receive from the left, send right, receive from the right) in the coming exchange."""
        a, b, c, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        N.check(self._lib.sc_halo_sizes(self._ctx, int(capacity_records), C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def halo_unpack(self, dev_from_left: int | None, left_records: int, dev_from_right: int | None,
                    right_records: int) -> None:
        N.check(self._lib.sc_halo_unpack(self._ctx, N._P(dev_from_left) if dev_from_left else None, int(left_records),
                                         N._P(dev_from_right) if dev_from_right else None, int(right_records)))

    def column_histogram(self, col0: int, n_columns: int) -> np.ndarray:
        hist = np.zeros(int(n_columns), dtype=np.int64)
        N.check(self._lib.sc_column_histogram(self._ctx, int(col0), int(n_columns), N.i64ptr(hist)))
        return hist

    # -- RCCL transport of the halo exchange (optional; see the header)
    @staticmethod
    def comm_available(rccl_path: str | None = None) -> bool:
        """True when librccl can be loaded here (sc_comm_available); never raises."""
        return N.load().sc_comm_available(rccl_path.encode() if rccl_path else None) == 0

    @staticmethod
    def comm_unique_id(rccl_path: str | None = None) -> bytes:
        buf = C.create_string_buffer(128)
        N.check(N.load().sc_comm_unique_id(rccl_path.encode() if rccl_path else None, C.cast(buf, N._P)))
        return buf.raw

    def comm_init(self, unique_id: bytes, rank: int, world: int, rccl_path: str | None = None) -> None:
        if len(unique_id) != 128:
            raise ValueError("an RCCL unique id is 128 bytes")
        buf = C.create_string_buffer(unique_id, 128)
        N.check(self._lib.sc_comm_init(self._ctx, rccl_path.encode() if rccl_path else None, C.cast(buf, N._P),
                                       int(rank), int(world)))

    def comm_destroy(self) -> None:
        N.check(self._lib.sc_comm_destroy(self._ctx))

    def halo_exchange(self, send_left: int | None, recv_left: int | None, left_rank: int, send_right: int | None,
                      recv_right: int | None, right_rank: int, sizes: tuple[int, int, int, int]) -> None:
        """Device pointers as ints; a negative rank = no neighbor on that side; `sizes` as halo_sizes() gives them.
        Enqueued on the context's stream."""
        ptr = lambda a: N._P(a) if a else None  # noqa: E731
        sl, rl, sr, rr = (int(k) for k in sizes)
        N.check(self._lib.sc_halo_exchange(self._ctx, ptr(send_left), sl, ptr(recv_left), rl, int(left_rank),
                                           ptr(send_right), sr, ptr(recv_right), rr, int(right_rank)))

    # -- halo overlap: the exchange on the side stream, next to the interior blocks of the force kernel
    def set_halo_overlap(self, on: bool = True) -> None:
        N.check(self._lib.sc_set_halo_overlap(self._ctx, 1 if on else 0))

    def side_stream(self) -> int:
        s = N._P()
        N.check(self._lib.sc_side_stream(self._ctx, C.byref(s)))
        return int(s.value or 0)

    def halo_overlap_begin(self, peer: "Engine | None" = None) -> None:
        N.check(self._lib.sc_halo_overlap_begin(self._ctx, peer._ctx if peer is not None else None))

    def halo_overlap_end(self) -> None:
        N.check(self._lib.sc_halo_overlap_end(self._ctx))

    def owned_count(self) -> int:
        n = C.c_int64(0)
        N.check(self._lib.sc_owned_count(self._ctx, C.byref(n)))
        return n.value

    # -- the probe: observables of the state, reduced on the device (sc_probe_*; the rule is tests/probe_spec.py)
    PROBE_LAUNCH_THREADS = N.PROBE_BLOCK * N.PROBE_BLOCKS  # threads of the probe's fixed launch: one slot each per turn

    def probe_now(self, bins: int = 0, x0: float = 0.0, x1: float = 1.0):
        """-> (row (16,) float64 in `probe.FIELDS` order, counts (bins,) int32, tops (bins,) float64) of the state as it
        stands (sc_probe_now); synchronises."""
        bins = int(bins)
        row = np.zeros(N.PROBE_FIELDS)
        counts = np.zeros(max(bins, 0), dtype=np.int32)
        tops = np.zeros(max(bins, 0))
        N.check(self._lib.sc_probe_now(self._ctx, bins, float(x0), float(x1), N.dptr(row),
                                       N.i32ptr(counts) if bins > 0 else None, N.dptr(tops) if bins > 0 else None))
        return row, counts, tops

    def probe_enable(self, capacity: int, bins: int = 0, x0: float = 0.0, x1: float = 1.0) -> None:
        """From now on every finished tick appends a row (and a profile of `bins` bins over [x0, x1)) to a log of
        `capacity` rows in device memory, without synchronising (sc_probe_enable)."""
        N.check(self._lib.sc_probe_enable(self._ctx, int(capacity), int(bins), float(x0), float(x1)))
        self._probe_log = (int(capacity), int(bins))

    def probe_disable(self) -> None:
        N.check(self._lib.sc_probe_disable(self._ctx))
        self._probe_log = None

    def probe_read(self, room: int | None = None):
        """-> (rows (T, 16), counts (T, bins), tops (T, bins), dropped): what was logged since the last read, oldest
        first, at most `room` rows (default: the log's capacity), and the ticks that found the log full
        (sc_probe_read); synchronises."""
        capacity, bins = self._probe_log or (0, 0)
        room = capacity if room is None else int(room)
        rows = np.zeros((max(room, 0), N.PROBE_FIELDS))
        counts = np.zeros((max(room, 0), bins), dtype=np.int32)
        tops = np.zeros((max(room, 0), bins))
        n, dropped = C.c_int64(0), C.c_int64(0)
        with_bins = bins > 0 and room > 0
        N.check(self._lib.sc_probe_read(self._ctx, N.dptr(rows) if room > 0 else None,
                                        N.i32ptr(counts) if with_bins else None, N.dptr(tops) if with_bins else None,
                                        room, C.byref(n), C.byref(dropped)))
        k = n.value
        return rows[:k].copy(), counts[:k].copy(), tops[:k].copy(), dropped.value

    # -- tracking: the state as packed frames (sc_track_*; the format is tests/track_spec.py, the host side track.py)
    @staticmethod
    def track_bound(n: int, n_segments: int) -> int:
        """The size in bytes of a frame of `n` particles and `n_segments` walls (sc_track_bound)."""
        b = C.c_int64(0)
        N.check(N.load().sc_track_bound(int(n), int(n_segments), C.byref(b)))
        return b.value

    def track_capture(self) -> bytes:
        """The state as it stands as one packed frame, with the walls of the last set_segments / tick
        (sc_track_capture); synchronises."""
        return self._fetch_bytes(lambda out, room, n: self._lib.sc_track_capture(self._ctx, out, room, n), 1 << 16)

    def track_enable(self, every: int = 1, capacity_bytes: int = 1 << 26) -> None:
        """From now on every tick whose number is a multiple of `every` appends a frame to a log of `capacity_bytes` in
        device memory, without synchronising; a frame that does not fit is dropped whole and counted
        (sc_track_enable)."""
        N.check(self._lib.sc_track_enable(self._ctx, int(every), int(capacity_bytes)))

    def track_disable(self) -> None:
        N.check(self._lib.sc_track_disable(self._ctx))

    def track_read(self):
        """-> (bytes: the frames logged since the last read, oldest first, back to back; how many; dropped frames)
        (sc_track_read); synchronises and rewinds the log."""
        frames, dropped = C.c_int64(0), C.c_int64(0)
        data = self._fetch_bytes(lambda out, room, n: self._lib.sc_track_read(self._ctx, out, room, n, C.byref(frames),
                                                                              C.byref(dropped)), 1 << 16)
        return data, frames.value, dropped.value

    def track_load(self, frame: bytes, plain: bool = False) -> None:
        """The frame becomes the context's state: dequantised positions, zero velocities, its ids, the pressure its
        colour bytes stand for (`plain`: the reference's playback colour for all) (sc_track_load); synchronises."""
        data = np.frombuffer(bytes(frame), dtype=np.uint8)
        N.check(self._lib.sc_track_load(self._ctx, N._P(data.ctypes.data) if len(data) else None, len(data),
                                        1 if plain else 0))

    # -- trajectories: full-precision frames in torch's memory, a row per id (sc_traj_*; the rule is
    # tests/trajectory_spec.py, the owner of the tensors trajectory.py)
    def traj_enable(self, states, pressure, ticks, counts, outside, words, *, id0: int, every: int = 1,
                    reset: bool = True) -> None:
        """From now on every tick whose number is a multiple of `every` writes one frame into the caller's CUDA tensors,
        without synchronising (sc_traj_enable_device): `states` float64 (F, M, 4), `pressure` float64 (F, M) or None,
        `ticks`, `counts`, `outside` int64 (F,) and `words` int64 (4,); row r of a frame is the particle with id
        `id0` + r.  `reset` zeroes the words; without it the recording continues where they stand.  The engine keeps the
        tensors alive until `traj_disable`.  ValueError for tensors that do not fit, before the library is touched."""
        shape = tuple(getattr(states, "shape", ()))
        if len(shape) != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"states must be a contiguous CUDA float64 tensor of shape (F, M, 4), F and M at least 1, on cuda:{self.device}")
        frames, rows = int(shape[0]), int(shape[1])
        _state_tensor(states, "states", "float64", (rows, 4), self.device, frames)
        if pressure is not None:
            _state_tensor(pressure, "pressure", "float64", (rows,), self.device, frames)
        for t, name in ((ticks, "ticks"), (counts, "counts"), (outside, "outside")):
            _state_tensor(t, name, "int64", (), self.device, frames)
        _state_tensor(words, "words", "int64", (), self.device, 4)
        id0, every = int(id0), int(every)
        if id0 < 0 or id0 + rows > 2 ** 31 - 1:
            raise ValueError(f"the window of ids [{id0}, {id0 + rows}) must lie within 0 .. 2^31 - 1")
        if every < 1:
            raise ValueError("every must be at least 1")
        ptr = lambda t: None if t is None else N._P(t.data_ptr())  # noqa: E731
        N.check(self._lib.sc_traj_enable_device(self._ctx, ptr(states), ptr(pressure), ptr(ticks), ptr(counts), ptr(outside),
                                                ptr(words), frames, id0, rows, every, 1 if reset else 0))
        self._traj_log = (states, pressure, ticks, counts, outside, words)

    def traj_capture(self) -> None:
        """One frame of the state as it stands, now, into the log (sc_traj_capture); enqueued only."""
        N.check(self._lib.sc_traj_capture(self._ctx))

    def traj_disable(self) -> None:
        """Stops recording (sc_traj_disable).  Launches may still be queued against the tensors: the engine lets go of
        them at the next `synchronize()`."""
        N.check(self._lib.sc_traj_disable(self._ctx))
        self._traj_retired, self._traj_log = self._traj_log, None

    # -- force monitor
    def enable_force_monitor(self, on: bool = True) -> None:
        N.check(self._lib.sc_enable_force_monitor(self._ctx, 1 if on else 0))
        self.force_monitor_on = bool(on)

    def force_monitor(self):
        """-> (sum of |dv| per phase (6,), particles summed) since the last call; synchronises."""
        sums = np.zeros(6)
        n = C.c_int64(0)
        N.check(self._lib.sc_get_force_monitor(self._ctx, N.dptr(sums), C.byref(n)))
        return sums, n.value

    # -- checkpoint
    def checkpoint_begin(self) -> None:
        N.check(self._lib.sc_checkpoint_begin(self._ctx))

    def checkpoint_finish(self, room: int | None = None):
        """-> dict(particles, velocities, ids, tick, next_id, rng) of the state sc_checkpoint_begin captured."""
        room = self.capacity if room is None else int(room)
        xy, vxy = np.empty((room, 2)), np.empty((room, 2))
        ids = np.empty(room, dtype=np.int64)
        n, tick, nid, pos = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int32(-1)
        key = np.zeros(624, dtype=np.uint32)
        N.check(self._lib.sc_checkpoint_finish(self._ctx, N.dptr(xy), N.dptr(vxy), N.i64ptr(ids), room, C.byref(n),
                                               C.byref(tick), C.byref(nid), key.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               C.byref(pos)))
        k = n.value
        return dict(particles=xy[:k].copy(), velocities=vxy[:k].copy(), ids=ids[:k].copy(), tick=tick.value,
                    next_id=nid.value, rng=(key, pos.value) if pos.value >= 0 else None)

    def restore_counters(self, tick: int, next_id: int) -> None:
        N.check(self._lib.sc_restore_counters(self._ctx, int(tick), int(next_id)))

    # -- NumPy's global MT19937 stream on the device
    def rng_set_state(self, key, pos: int) -> None:
        """Hand the stream of `np.random.get_state()` (624-word key, position) to the device."""
        k = np.ascontiguousarray(key, dtype=np.uint32).reshape(624)
        N.check(self._lib.sc_rng_set_state(self._ctx, k.ctypes.data_as(C.POINTER(C.c_uint32)), int(pos)))

    def rng_get_state(self):
        """-> (key, position) of the device stream; synchronises."""
        k = np.zeros(624, dtype=np.uint32)
        pos = C.c_int32(0)
        N.check(self._lib.sc_rng_get_state(self._ctx, k.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(pos)))
        return k, pos.value

    def emit_particles(self, sources, dt: float, max_particles: int) -> None:
        """particle_source.py:17-24 for `sources` (objects with radius, position, velocity, flow, noise) on the device."""
        arr = (N.Source * max(len(sources), 1))()
        for k, s in enumerate(sources):
            arr[k] = N.Source(float(s.radius), float(s.position[0]), float(s.position[1]), float(s.velocity[0]),
                              float(s.velocity[1]), float(s.noise), int(s.flow))
        N.check(self._lib.sc_emit_particles(self._ctx, arr, len(sources), float(dt), int(max_particles)))

    # -- timing
    def enable_timing(self, on: bool = True) -> None:
        N.check(self._lib.sc_enable_timing(self._ctx, 1 if on else 0))
        self.timing_on = bool(on)

    def reset_timing(self) -> None:
        N.check(self._lib.sc_reset_timing(self._ctx))

    def timing(self) -> dict[str, tuple[float, int]]:
        """-> {kernel name: (total ms, launches)} since reset_timing()."""
        ms = np.zeros(N.NUM_KERNELS)
        cnt = np.zeros(N.NUM_KERNELS, dtype=np.int64)
        N.check(self._lib.sc_get_timing(self._ctx, N.dptr(ms), N.i64ptr(cnt)))
        return {self._lib.sc_kernel_name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(N.NUM_KERNELS)}
