"""The neighbourhood calls of `Crate` -- `pair_tensors`, `cluster_tensors`, `cluster_tensors_batch`, `cluster_sums`,
`cluster_sums_batch`, `cluster_observables`, `neighbor_tensors`, `field_tensors`, `field_function`, `distance_histogram`,
`distance_histogram_batch`, `ray_tensors` and `ray_paths` -- as a mixin `Crate`
inherits (crate.py is the reference's surface, the tick and growth), and the protocol all of them follow,
written once: `_Search`.

Every call counts the pairs on the grid (`Engine.pairs_count`) and then runs one or more readers of that grid
(`pairs_fill`, `pairs_label`, `pairs_cluster_sums`, `pairs_nearest`, `pairs_sum`, `pairs_sum_grad`, `pairs_hist`,
`pairs_rays`, `pairs_ray_paths`, and the `_batch` forms of label, histogram, rays and paths on a batched grid), all on the
library's stream, into tensors of torch's that it allocates at a size known beforehand.  Either
it then synchronises, reads the counts, raises what the status says and cuts the tensors, or it returns the tensors as
they are with `counts` last.  The C side of the same sharing is `reader_begin` / `reader_check`
(csrc/sc_host_state.h).  torch is imported on first use."""
from __future__ import annotations

import numpy as np

from . import _native as N
from .engine import _batch_tensor


def _point_rows(points) -> int:
    """The rows of a caller's (n, 2) tensor of points; what is no such tensor is left to the engine's check (0 rows)."""
    return int(points.shape[0]) if getattr(points, "is_cuda", False) and len(points.shape) == 2 else 0


_BATCH_ORDER = "batch offsets must start at 0, not descend and end at the number of points"

# What a negative status in `counts[1]` says, whichever reader wrote it (PAIRS_*, FIELDS_*, HIST_* and CLUSTER_SUMS_* of
# _native.py number them alike).  The calls that take `queries` say so in their texts.
_STATUS = {
    N.PAIRS_BATCH: "{who}: " + _BATCH_ORDER + "{of_queries}",
    N.PAIRS_DOMAIN: "{who}: a coordinate{of_either} lies outside the domain |c| / radius < 2^31 (radius {radius!r})",
    N.FIELDS_VALUES_SHORT: "{who}: {short}",
    N.PAIRS_RANGE: "{who}: {far}",
}
_QUERY_CALLS = ("neighbor_tensors", "field_tensors", "field_function", "distance_histogram", "ray_tensors", "ray_paths")
_OF_EITHER = dict.fromkeys(("ray_tensors", "ray_paths"), " of a point, an origin or a ray's end point origin + max_t * direction")


def _check_batch(who: str, device: int, points, queries, batch, query_batch, second: str = "query_batch") -> None:
    """The `batch=` / `query_batch=` arguments of a neighbourhood call: ValueError before anything is enqueued.  `second`
    is the name the call gives its second offsets (`ray_batch` for the rays, which are the queries)."""
    if batch is None:
        if query_batch is not None:
            raise ValueError(f"{who}: {second} without batch")
        return
    if points is None:
        raise ValueError(f"{who}: batch needs points, the state is one cloud")
    entries = _batch_tensor(batch, "batch", device)
    if queries is None:
        if query_batch is not None:
            raise ValueError(f"{who}: {second} without queries")
    elif query_batch is None:
        raise ValueError(f"{who}: {'rays' if second == 'ray_batch' else 'queries'} of a batched call need {second}, their clouds")
    else:
        _batch_tensor(query_batch, second, device, entries)


def _field_values(values):
    """-> (`values` of `field_tensors` and `field_function` as the kernels take it, contiguous float64 (n, C), or None;
    whether it came as (n,)).  ValueError for anything else."""
    import torch
    if values is None:
        return None, False
    if not getattr(values, "is_cuda", False) or values.dtype != torch.float64 or values.dim() not in (1, 2):
        raise ValueError("values must be a CUDA float64 tensor of shape (n, C) or (n,)")
    flat = values.dim() == 1
    values = (values.unsqueeze(1) if flat else values).contiguous()
    if values.shape[1] < 1:
        raise ValueError("values must have at least one column")
    return values, flat


class _Search:
    """One count-then-read call of `who`, a method below or `fields.position_grad` (as "field_function").  The caller
    checks its own arguments first -- nothing here is reached, and the engine is not touched, before they have passed --
    then makes one of these, allocates its outputs at `rows` rows on `dev`, calls `count`, runs its readers with
    `counts`, and leaves through `end` (or `read` / `park`, where the way out is its own).

    radius   the crate's diameter unless given
    bound    the rows the count may find: the capacity, or the rows of `points`
    rows     the rows of the readers' tables: those of `queries`, else `bound`
    offsets  int64 (bound + 1,): the count's scan, which only `pair_tensors` returns
    counts   int64 (2,): (n, E) of the count, then (rows, status) of each reader -- with `queries` a second pair, so that
             the count's n, the number of particles, stays readable; both pairs are one allocation and one host copy
    short    the sentence of status -2, the caller's arrays having too few rows
    far      the sentence of status -4, a ray that would walk beyond the cap"""

    def __init__(self, crate, who: str, radius=None, *, points=None, queries=None, batch=None, query_batch=None,
                 sync: bool = True, short: str = "", far: str = "", second: str = "query_batch"):
        import torch
        eng = crate._engine
        self.crate, self.who, self.eng, self.sync, self.short, self.far = crate, who, eng, sync, short, far
        self.points, self.queries, self.batch = points, queries, batch
        self.dev = torch.device("cuda", eng.device)
        self.radius = float(crate.diameter if radius is None else radius)
        _check_batch(who, eng.device, points, queries, batch, query_batch, second)
        self.clouds = 0 if batch is None else int(batch.shape[0]) - 1
        self.bound = eng.capacity if points is None else _point_rows(points)
        self.rows = self.bound if queries is None else _point_rows(queries)

    def count(self, half: bool = True) -> None:
        """Allocates `offsets` and `counts` and enqueues the count.  The synchronising form first waits for torch's stream:
        what the caller asked of torch so far -- contiguous copies, column chunks -- is done, and nothing of torch's
        touches the new tensors (their memory may have been freed with work still queued)."""
        import torch
        self.offsets = torch.empty(self.bound + 1, dtype=torch.int64, device=self.dev)
        self._counts = torch.empty(2 if self.queries is None else 4, dtype=torch.int64, device=self.dev)
        self.counts = self._counts[-2:]
        if self.sync:
            torch.cuda.current_stream(self.dev).synchronize()
        self.eng.pairs_count(self.points, radius=self.radius, offsets=self.offsets, counts=self._counts[:2], half=half,
                             batch=self.batch)

    def read(self):
        """Synchronises and reads the counts -> (n, status) of the last reader (of the count, before any).  ValueError for
        a negative status; the crate learns its particle count when the state was searched."""
        self.eng.synchronize()
        got = self._counts.cpu().tolist()
        n, status = got[-2:]
        if status < 0:
            queries = self.who in _QUERY_CALLS
            raise ValueError(_STATUS.get(status, _STATUS[N.PAIRS_DOMAIN]).format(
                who=self.who, radius=self.radius, short=self.short,
                of_either=_OF_EITHER.get(self.who, " of a point or a query") if queries else "",
                of_queries=f" (of {'rays for ray_batch' if self.who in _OF_EITHER else 'queries for query_batch'})"
                if queries else "", far=self.far))
        if self.points is None:
            self.crate._state_changed(got[0], self.crate._cache)  # (the state is the same: only its count was learned)
        return n, status

    def park(self, *held) -> None:
        """What is still queued and not returned -- `offsets`, the count's `counts`, `held` -- stays alive until the next
        call of the same method: one slot per method, since another method's call says nothing about this one's queue."""
        vars(self.crate).setdefault("_parked", {})[self.who] = (self.offsets, self._counts, *held)

    def end(self, rows=(), items=(), whole=(), held=()):
        """The call's result from its outputs (None: not asked for): `rows` have one row per point or query, `items` one
        per counted item (`counts[1]`: clusters), `whole` are returned as they are.  Not synchronising: parks and
        returns them all, `counts` last.  Synchronising: `read`, and cuts `rows` to n and `items` to the count."""
        rows, items, whole = ([t for t in group if t is not None] for group in (rows, items, whole))
        if not self.sync:
            self.park(*held)
            return (*rows, *items, *whole, self.counts)
        n, total = self.read()
        return (*(t[:n] for t in rows), *(t[:total] for t in items), *whole)


class _Neighbourhood:
    """`Crate`'s neighbourhood calls.  Uses of the crate: `_engine`, `diameter`, `state_tensors`, `segments` and
    `rigid_bodies` (the walls of `ray_tensors`), and `_state_changed`, through which a synchronising search of the state
    brings the particle count up to date."""

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
        sync = max_pairs is None
        if not sync and int(max_pairs) < 0:
            raise ValueError("max_pairs must not be negative")
        call = _Search(self, "pair_tensors", radius, points=points, batch=batch, sync=sync)
        call.count(half)
        n, total = call.read() if sync else (None, int(max_pairs))  # (the one call that synchronises in the middle)
        partners = torch.empty(total, dtype=torch.int64, device=call.dev)
        d2 = torch.empty(total, dtype=torch.float64, device=call.dev) if squared_distances else None
        call.eng.pairs_fill(partners, d2)
        if sync:
            call.eng.synchronize()
            return (call.offsets[:n + 1], partners) + ((d2,) if squared_distances else ())
        return (call.offsets, partners) + ((d2,) if squared_distances else ()) + (call.counts,)

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
        `engine.set_stream`, and everything torch enqueues afterwards sees them.

        The clusters of a minibatch of clouds in one call: `cluster_tensors_batch`."""
        return self._clusters("cluster_tensors", radius, points, None, max_clusters)

    def cluster_tensors_batch(self, radius: float | None = None, *, points, batch, max_clusters: int | None = None):
        """`cluster_tensors` of B disjoint clouds in one call (sc_pairs_label_batch_device): `batch`, an int64 CUDA tensor
        of B + 1 ascending offsets from 0 to n as in `pair_tensors`, cuts `points` into clouds that may overlap in space
        completely, and a cluster never crosses clouds.  ``(labels, sizes, roots, cluster_ptr)``: labels and roots are
        global, and because clusters are numbered by their smallest member, cloud b's clusters are the contiguous range
        ``cluster_ptr[b]:cluster_ptr[b + 1]`` of `sizes` and `roots` -- `cluster_ptr`, int64 (B + 1,), ends at C; a cloud
        without a finite point has none (`sand_crate_amd.pairs.cluster_cloud` gives every cluster's cloud).  The result
        is, bit for bit, `cluster_tensors` cloud by cloud, the labels shifted by the clusters before and the roots by
        ``batch[b]`` (tests/batch_readers_spec.py).  `max_clusters` as in `cluster_tensors`: `counts` stays last and
        `cluster_ptr` is always whole.  Offsets that are not in order raise ValueError at the synchronisation (C = -3
        with `max_clusters`).  (A method of its own and not `batch=` of `cluster_tensors`: the result has one tensor
        more, as `cluster_sums_batch`'s has.)"""
        return self._clusters("cluster_tensors", radius, points, batch, max_clusters, batched=True)

    def _clusters(self, who, radius, points, batch, max_clusters, values=None, extrema=False, batched=False):
        """`cluster_tensors`, `cluster_sums` and their `_batch` forms: count, label and -- with `values` -- reduce."""
        import torch
        sync = max_clusters is None
        if not sync and int(max_clusters) < 0:
            raise ValueError("max_clusters must not be negative")
        if batched and batch is None:
            raise ValueError(f"{who}: batch must be the clouds' offsets")
        short = "" if values is None else f"values has {values.shape[0]} rows, fewer than there are points"
        call = _Search(self, who, radius, points=points, batch=batch, sync=sync, short=short)
        room = call.rows if sync else int(max_clusters)
        labels = torch.empty(call.rows, dtype=torch.int64, device=call.dev)
        sizes = torch.empty(room, dtype=torch.int64, device=call.dev)
        roots = torch.empty(room, dtype=torch.int64, device=call.dev)
        width = 0 if values is None else int(values.shape[1])
        tables = tuple(torch.empty((room, width), dtype=torch.float64, device=call.dev)
                       for _ in range(0 if values is None else 3 if extrema else 1))
        cluster_ptr = None if batch is None else torch.empty(call.clouds + 1, dtype=torch.int64, device=call.dev)
        call.count()  # (one `counts` for all: (n, E) of the count, then (n, C) of the label and of the sums)
        if batch is None:
            call.eng.pairs_label(labels, sizes, roots, counts=call.counts)
        else:
            call.eng.pairs_label_batch(labels, sizes, roots, cluster_ptr=cluster_ptr, counts=call.counts)
        if values is not None:
            call.eng.pairs_cluster_sums(values, *tables, counts=call.counts)
        return call.end(rows=(labels,), items=(sizes, roots, *tables), whole=(cluster_ptr,),
                        held=() if values is None else (values,))

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
        called, as `points` must.

        The sums of a minibatch of clouds in one call: `cluster_sums_batch`."""
        return self._clusters("cluster_sums", radius, points, None, max_clusters, self._cluster_values(values), extrema)

    def cluster_sums_batch(self, values, radius: float | None = None, *, points, batch, extrema: bool = False,
                           max_clusters: int | None = None):
        """`cluster_sums` of B disjoint clouds in one call: the clusters are `cluster_tensors_batch`'s, the rows of `values`
        are global, and the reduction is `cluster_sums`' own, which reads the batched label as any other
        (sc_pairs_label_batch_device, then sc_pairs_cluster_sums_device).
        ``(labels, sizes, roots, sums[, mins, maxs], cluster_ptr)``: `cluster_ptr` comes after the tables and is always
        whole, `counts` stays last with `max_clusters`.  Bit for bit `cluster_sums` cloud by cloud
        (tests/batch_readers_spec.py)."""
        return self._clusters("cluster_sums", radius, points, batch, max_clusters, self._cluster_values(values), extrema,
                              batched=True)

    @staticmethod
    def _cluster_values(values):
        """`values` of `cluster_sums` as the kernel takes it: contiguous float64 (n, F).  ValueError for anything else."""
        import torch
        if not getattr(values, "is_cuda", False) or values.dtype != torch.float64 or values.dim() not in (1, 2):
            raise ValueError("values must be a CUDA float64 tensor of shape (n, F) or (n,)")
        values = (values.unsqueeze(1) if values.dim() == 1 else values).contiguous()
        width = int(values.shape[1])
        if not 1 <= width <= N.CLUSTER_SUMS_MAX_CHANNELS:
            raise ValueError(f"values must have 1 .. {N.CLUSTER_SUMS_MAX_CHANNELS} columns")
        return values

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

    def neighbor_tensors(self, k: int, radius: float | None = None, *, points=None, queries=None,
                         squared_distances: bool = False, partner_counts: bool = False, sync: bool = True,
                         batch=None, query_batch=None):
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

        `batch` makes `points` B disjoint clouds in one call, as in `pair_tensors`; with `queries` comes `query_batch`,
        also B + 1 offsets, from 0 to q: query rows ``query_batch[b]:query_batch[b + 1]`` see only the points of cloud b
        (a cloud may have points and no queries, or queries and no points).  Offsets that are not in order raise
        ValueError at the synchronisation (cut = -3 with `sync=False`)."""
        import torch
        k = int(k)
        if not 1 <= k <= N.NEAREST_MAX_K:
            raise ValueError(f"k must be 1 .. {N.NEAREST_MAX_K}")
        call = _Search(self, "neighbor_tensors", radius, points=points, queries=queries, batch=batch, query_batch=query_batch,
                       sync=sync)
        neighbors = torch.empty((call.rows, k), dtype=torch.int64, device=call.dev)
        d2 = torch.empty((call.rows, k), dtype=torch.float64, device=call.dev) if squared_distances else None
        partners = torch.empty(call.rows, dtype=torch.int64, device=call.dev) if partner_counts else None
        call.count()
        call.eng.pairs_nearest(neighbors, d2, partners, k=k, queries=queries, counts=call.counts, query_batch=query_batch)
        return call.end(rows=(neighbors, d2, partners))

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
        power = int(power)
        if not 0 <= power <= 3:
            raise ValueError("power must be 0 .. 3")
        values, flat = _field_values(values)
        step = N.FIELDS_MAX_CHANNELS
        width = 0 if values is None else int(values.shape[1])
        chunks = [values] if width <= step else [values[:, at:at + step].contiguous() for at in range(0, width, step)]
        short = "" if values is None else f"values has {values.shape[0]} rows, fewer than there are points"
        call = _Search(self, "field_tensors", radius, points=points, queries=queries, batch=batch, query_batch=query_batch,
                       sync=sync, short=short)
        want_wsum = weight_sums or values is None
        wsum = torch.empty(call.rows, dtype=torch.float64, device=call.dev) if want_wsum else None
        parts = [None if v is None else torch.empty((call.rows, v.shape[1]), dtype=torch.float64, device=call.dev)
                 for v in chunks]
        call.count()
        for at, (v, part) in enumerate(zip(chunks, parts)):  # (every launch consumes the query offsets: given each time)
            call.eng.pairs_sum(v, part, wsum if at == 0 else None, power=power, include_self=include_self, queries=queries,
                               counts=call.counts, query_batch=query_batch)
        if sync:  # (before the parts are put together: torch's stream does not wait for the library's)
            n, _ = call.read()
        else:
            call.park(chunks, parts)
        out = ()
        if values is not None:
            sums = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
            out = (sums.view(-1) if flat else sums,)
        if want_wsum:
            out += (wsum,)
        return (*out, call.counts) if not sync else tuple(t[:n] for t in out)

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
        stream, `engine.set_stream`, and everything torch enqueues afterwards sees them.

        The histograms of a minibatch of clouds in one call: `distance_histogram_batch`."""
        return self._histogram(edges, points, queries, None, None, per_row, totals, sync)

    def distance_histogram_batch(self, edges, *, points, batch, queries=None, query_batch=None, per_row: bool = False,
                                 totals: bool = True, sync: bool = True):
        """`distance_histogram` of B disjoint clouds in one call (sc_pairs_hist_batch_device): `batch` cuts `points` and,
        with `queries`, `query_batch` cuts them, as in `neighbor_tensors` -- a row counts the partners of its own cloud
        only.  ``([table, ]total)``: `table` as before, one row per point or query, and `total` int64 (B, bins), row b the
        column sums over the rows of cloud b -- g(r) per frame through `sand_crate_amd.pairs.radial_distribution` with
        the clouds' sizes.  Bit for bit `distance_histogram` cloud by cloud, the tables concatenated and the totals
        stacked (tests/batch_readers_spec.py).  `sync` as in `distance_histogram`; offsets that are not in order raise
        ValueError at the synchronisation (status -3 with `sync=False`).  (A method of its own and not `batch=` of
        `distance_histogram`: `total` has another shape.)"""
        if batch is None:
            raise ValueError("distance_histogram: batch must be the clouds' offsets")
        return self._histogram(edges, points, queries, batch, query_batch, per_row, totals, sync)

    def _histogram(self, edges, points, queries, batch, query_batch, per_row, totals, sync):
        import torch
        if not per_row and not totals:
            raise ValueError("neither per_row nor totals: nothing to return")
        e = np.array(edges, dtype=np.float64)
        bins = len(N.hist_squared_edges(e)) - 1
        if not e[-1] > 0:  # (never: the edges ascend from 0 or more)
            raise ValueError("the last edge must be positive")
        call = _Search(self, "distance_histogram", e[-1], points=points, queries=queries, batch=batch, query_batch=query_batch,
                       sync=sync)
        if call.clouds * bins > N.HIST_BATCH_MAX_CELLS:
            raise ValueError(f"distance_histogram: {call.clouds} clouds x {bins} bins, at most {N.HIST_BATCH_MAX_CELLS} totals")
        table = torch.empty((call.rows, bins), dtype=torch.int32, device=call.dev) if per_row else None
        shape = bins if batch is None else (call.clouds, bins)
        total = torch.empty(shape, dtype=torch.int64, device=call.dev) if totals else None
        call.count()
        if batch is None:
            call.eng.pairs_hist(table, total, edges=e, queries=queries, counts=call.counts)
        else:
            call.eng.pairs_hist_batch(table, total, edges=e, queries=queries, query_batch=query_batch, counts=call.counts)
        return call.end(rows=(table,), whole=(total,), held=() if query_batch is None else (query_batch,))

    def ray_tensors(self, origins, directions, max_t: float, *, disc_radius: float | None = None, walls=True,
                    particles: bool = True, points=None, sync: bool = True, batch=None, ray_batch=None):
        """What a sensor sees along a line: for every ray the first thing it meets among the particles -- discs of radius
        `disc_radius` (default: the crate's particle radius, ``diameter / 2``) -- and the walls, as torch CUDA tensors on
        the crate's device, walked on the GPU through the pair search's grid (sc_pairs_count_device at the radius
        ``2 * disc_radius``, then sc_pairs_rays_device): ``(t, hit)`` -- float64 (R,) and int64 (R,).  `origins` and
        `directions` are float64 (R, 2) CUDA tensors; a direction is not normalised, ``t`` is in units of its length (with
        unit directions, `sand_crate_amd.pairs.ray_fan`, the distance), and only hits with ``0 <= t <= max_t`` count;
        `max_t` is a finite host float.  ``hit[r]`` is j >= 0 for particle j -- the row of `state_tensors()` at the same
        point of the stream, or of `points`, a float64 (n, 2) CUDA tensor that is searched instead of the state --,
        ``-2 - s`` for wall s and -1 for nothing, with ``t = +inf`` (`sand_crate_amd.pairs.hit_particles`, `hit_walls`
        and `ray_points` read the result).  An origin inside or on a disc hits it at t = 0; a wall counts from either
        face, a ray parallel to it misses; of equal t a wall comes before a particle and a lower index before a higher
        one.  A ray with a number that is not finite, or with a zero direction, has t = NaN and hit = -1; a particle
        with a coordinate that is not finite is never hit.  Every operation is rounded on its own and the smallest
        (t, kind, index) is taken: a pure function of the state and the rays, the same on every call
        (tests/ray_spec.py is the rule).

        `walls=True` are the crate's current `segments`, an (S, 2, 2) host array the caller's own (at most 16), `False`
        none; `particles=False` looks at the walls alone (the origins must still lie in the domain).  In an open scene
        keep `max_t` short: a ray may walk at most 8192 cells of one particle diameter before it meets a wall.

        `sync=True` synchronises once at the end and reads 32 bytes; ValueError when a coordinate of a particle, of an
        origin or of an end point ``origin + max_t * direction`` has |c| / (2 disc_radius) >= 2^31, and when a ray would
        walk further than the cap.  `sync=False` synchronises nothing and returns ``(t, hit, counts)``, the int64
        `counts` tensor (rays, status) last: status -1 is the domain error, -4 the cap (nothing else was written).  The
        tensors are written on the library's stream, and the library's stream does not wait for torch's: read them after
        `synchronize()`, and have `origins`, `directions` and `points` ready before the call -- or run the crate on
        torch's stream, `engine.set_stream`, and everything torch enqueues afterwards sees them.

        `batch` and `ray_batch`, both int64 CUDA tensors of B + 1 ascending offsets, come together and make the call B
        scenes at once (sc_pairs_rays_batch_device): `batch` cuts `points` into clouds as in `pair_tensors`, `ray_batch`
        cuts the rays, and rays ``ray_batch[b]:ray_batch[b + 1]`` meet the particles of cloud b only -- a sensor fan per
        recorded frame.  The walls are shared by all clouds, ``hit`` is the global row of `points`, and the result is,
        bit for bit, the per-cloud results concatenated (tests/batch_readers_spec.py).  Offsets that are not in order
        raise ValueError at the synchronisation (status -3 with `sync=False`)."""
        import torch
        rho, max_t, segments, far = self._ray_arguments(origins, directions, max_t, disc_radius, walls)
        call = _Search(self, "ray_tensors", 2 * rho, points=points, queries=origins, batch=batch, query_batch=ray_batch,
                       sync=sync, far=far, second="ray_batch")
        t = torch.empty(call.rows, dtype=torch.float64, device=call.dev)
        hit = torch.empty(call.rows, dtype=torch.int64, device=call.dev)
        call.count()
        common = dict(origins=origins, directions=directions, disc_radius=rho if particles else 0.0, max_t=max_t,
                      segments=segments, counts=call.counts)
        if batch is None:
            call.eng.pairs_rays(t, hit, **common)
        else:
            call.eng.pairs_rays_batch(t, hit, ray_batch=ray_batch, **common)
        return call.end(rows=(t, hit), held=(origins, directions, ray_batch))

    def _ray_arguments(self, origins, directions, max_t, disc_radius, walls):
        """The arguments `ray_tensors` and `ray_paths` share, checked: -> (rho, max_t, segments, the sentence of status
        -4).  ValueError before anything is enqueued."""
        import torch
        rho = float(self.diameter / 2 if disc_radius is None else disc_radius)
        if not 0 < rho < float("inf"):
            raise ValueError("disc_radius must be finite and positive")
        max_t = float(max_t)
        if not 0 <= max_t < float("inf"):
            raise ValueError("max_t must be finite and not negative")
        if walls is True:
            segments = self.segments if self.rigid_bodies else np.zeros((0, 2, 2))
        elif walls is False or walls is None:
            segments = np.zeros((0, 2, 2))
        else:
            segments = np.ascontiguousarray(walls, dtype=np.float64)
        if segments.ndim != 3 or segments.shape[1:] != (2, 2) or len(segments) > N.MAX_SEGMENTS:
            raise ValueError(f"walls must be True, False or an (S, 2, 2) array with S at most {N.MAX_SEGMENTS}")
        for tensor, name in ((origins, "origins"), (directions, "directions")):
            if not getattr(tensor, "is_cuda", False) or tensor.dtype != torch.float64 or tensor.dim() != 2 or \
                    tensor.shape[1] != 2 or not tensor.is_contiguous():
                raise ValueError(f"{name} must be a contiguous CUDA float64 tensor of shape (R, 2)")
        if origins.shape[0] != directions.shape[0]:
            raise ValueError("origins and directions must have the same number of rows")
        far = (f"max_t {max_t!r} lets a ray walk more than the cap of {N.RAY_MAX_STEPS} cells of width {2 * rho!r} before "
               "it meets a wall: shorten max_t, or close the scene with walls")
        return rho, max_t, segments, far

    def ray_paths(self, origins, directions, max_t: float, bounces: int = 1, *, disc_radius: float | None = None, walls=True,
                  particles: bool = True, points=None, sync: bool = True, batch=None, ray_batch=None):
        """Where a signal goes: `ray_tensors` followed through `bounces` specular reflections, 0 .. 15, in one launch
        (sc_pairs_count_device at the radius ``2 * disc_radius``, then sc_pairs_ray_paths_device): the named tuple
        ``RayPaths(t, hit, points, normals, end)`` -- float64 (R, L), int64 (R, L), float64 (R, L, 2), float64 (R, L, 2)
        and int64 (R,), L = bounces + 1 legs per ray.  The arguments are `ray_tensors`'; `max_t` is the budget of the
        whole path, in units of the first direction's length, which a reflection keeps up to rounding.

        Leg 0 is `ray_tensors`' result, bit for bit.  ``points[r, k]`` is where leg k hit, ``origin + t * direction`` of
        that leg, and ``normals[r, k]`` the unit normal of the surface there, facing the side the ray came from: from the
        particle's centre to the point, or the wall's normal.  The next leg starts at that point with the direction
        mirrored about the normal, ``d - 2 (d . n) n``, and with what is left of the budget.  It does not see what the
        leg before it hit, and a disc its origin lies in or on only when it heads inward: the continuation names the thing
        it stands on and needs no epsilon, so the bits depend on none.  A leg 0 that starts inside a disc hits it at
        t = 0; it is reflected when it points inward and kept when it points outward.  ``end[r]`` says how the path ended:
        0 every leg hit something; 1 a leg met nothing within the budget, that leg has t = +inf and hit = -1; 2 the ray is
        dead, as in `ray_tensors`, or a normal is not finite -- a hit from a disc's own centre --, or the next leg would be
        dead; -1 and -4 the next leg would leave the domain or walk past the cap of 8192 cells: for a later leg these end
        that ray only.  Legs a path never reached have t = NaN, hit = -1 and NaN points and normals.  Every operation is
        rounded on its own: a pure function of the state and the rays, the same on every call (tests/ray_path_spec.py is
        the rule; `sand_crate_amd.pairs.path_legs` and `path_arrows` read the result).

        `sync=True` synchronises once at the end and raises `ray_tensors`' ValueErrors for leg 0, the caller's input: a
        coordinate outside the domain, a first leg beyond the cap.  `sync=False` synchronises nothing and returns
        ``(t, hit, points, normals, end, counts)``, the int64 `counts` tensor (rays, status) last, with the stream rules of
        `ray_tensors`.  `batch` and `ray_batch` as in `ray_tensors` (sc_pairs_ray_paths_batch_device): every leg of a
        path stays among the particles of its ray's cloud."""
        import torch
        from .pairs import RayPaths
        bounces = int(bounces)
        if not 0 <= bounces <= N.RAY_MAX_BOUNCES:
            raise ValueError(f"bounces must be 0 .. {N.RAY_MAX_BOUNCES}")
        rho, max_t, segments, far = self._ray_arguments(origins, directions, max_t, disc_radius, walls)
        call = _Search(self, "ray_paths", 2 * rho, points=points, queries=origins, batch=batch, query_batch=ray_batch,
                       sync=sync, far=far, second="ray_batch")
        legs = bounces + 1
        t = torch.empty((call.rows, legs), dtype=torch.float64, device=call.dev)
        hit = torch.empty((call.rows, legs), dtype=torch.int64, device=call.dev)
        at = torch.empty((call.rows, legs, 2), dtype=torch.float64, device=call.dev)
        normals = torch.empty((call.rows, legs, 2), dtype=torch.float64, device=call.dev)
        end = torch.empty(call.rows, dtype=torch.int64, device=call.dev)
        call.count()
        common = dict(origins=origins, directions=directions, bounces=bounces, disc_radius=rho if particles else 0.0,
                      max_t=max_t, segments=segments, counts=call.counts)
        if batch is None:
            call.eng.pairs_ray_paths(t, hit, at, normals, end, **common)
        else:
            call.eng.pairs_ray_paths_batch(t, hit, at, normals, end, ray_batch=ray_batch, **common)
        out = call.end(rows=(t, hit, at, normals, end), held=(origins, directions, ray_batch))
        return RayPaths(*out) if sync else out
