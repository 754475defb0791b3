"""Small torch helpers for the CSR pair lists of `Crate.pair_tensors` (offsets, partners) and for the clusters of
`Crate.cluster_tensors` (labels, sizes), for the nearest-k tables of `Crate.neighbor_tensors` (neighbors), for the
weighted sums of `Crate.field_tensors` (sums, wsum), for the distance histograms of `Crate.distance_histogram`
(edges, total), for the ray sensors of `Crate.ray_tensors` (origins, directions, t, hit) and for the ray paths of
`Crate.ray_paths` (hit, points)."""
from __future__ import annotations

import collections


def batch_ptr(lengths, device=None):
    """The `batch=` offsets of `Crate.pair_tensors`, `neighbor_tensors`, `field_tensors`, `field_function` and the other
    batched neighbourhood calls from the clouds' sizes: int64 (B + 1,), ``ptr[0] = 0`` and ``ptr[b + 1] = ptr[b] + lengths[b]`` -- the `ptr` of a graph
    library's batch.  `lengths` is a sequence or an int64 tensor of B >= 1 sizes, none negative."""
    import torch
    sizes = torch.as_tensor(lengths, dtype=torch.int64).reshape(-1).cpu()
    if sizes.shape[0] < 1 or bool((sizes < 0).any()):
        raise ValueError("lengths must hold at least one size, none negative")
    ptr = torch.zeros(sizes.shape[0] + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(sizes, 0)
    return ptr if device is None else ptr.to(device)


def batch_index(ptr, n=None):
    """The cloud of every row, the `batch` vector of a graph library: int64 (n,), row i lies in cloud b iff
    ``ptr[b] <= i < ptr[b + 1]``.  `n` defaults to ``ptr[-1]`` (which then synchronises to read it)."""
    import torch
    n = int(ptr[-1]) if n is None else int(n)
    clouds = torch.arange(ptr.shape[0] - 1, dtype=torch.int64, device=ptr.device)
    return torch.repeat_interleave(clouds, ptr[1:] - ptr[:-1], output_size=n)


def row_lengths(offsets):
    """The number of partners of every row: int64 (n,)."""
    return offsets[1:] - offsets[:-1]


def edge_index(offsets, partners):
    """The (2, E) int64 edge list (row 0: i, row 1: j) of a CSR pair list, in (i, j) order -- the `edge_index` of a
    graph network.  `partners` may be shorter than offsets[-1] (a clipped list): the edges are then cut to its length."""
    import torch
    n = offsets.shape[0] - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=offsets.device), row_lengths(offsets))
    k = min(int(rows.shape[0]), int(partners.shape[0]))
    return torch.stack([rows[:k], partners[:k]])


def cluster_size_of(labels, sizes):
    """The size of every point's cluster (`Crate.cluster_tensors`): int64 (n,), 0 for a point in no cluster (label -1)."""
    import torch
    if sizes.shape[0] == 0:
        return torch.zeros_like(labels)
    return torch.where(labels >= 0, sizes[labels.clamp(min=0)], torch.zeros_like(labels))


def largest_cluster(sizes):
    """-> (index, size) of the largest cluster, the first of equals; (-1, 0) when there is none."""
    if sizes.shape[0] == 0:
        return -1, 0
    c = int(sizes.argmax())
    return c, int(sizes[c])


# The columns of `Crate.cluster_observables`' table: the probe's observables per cluster, named as `probe.FIELDS` names
# them (a cluster's max_speed2 and max_p are plain maxima over its members: a cluster is never empty).
CLUSTER_FIELDS = ("n", "sum_x", "sum_y", "sum_vx", "sum_vy", "sum_ke", "sum_p", "min_x", "max_x", "min_y", "max_y",
                  "max_speed2", "max_p", "n_pressed")
# ... and the channels they are reduced from (`cluster_channels`), in the order of the table's six sums.
CLUSTER_CHANNELS = ("x", "y", "vx", "vy", "ke", "p", "speed2", "pressed")


def cluster_channels(particles, velocities, pressure):
    """The float64 (n, 8) channel table `Crate.cluster_observables` reduces, from `state_tensors()`: x, y, vx, vy,
    ``0.5 * (vx*vx + vy*vy)``, p, ``vx*vx + vy*vy`` and ``p > 0`` as 0 or 1.  Every torch operation is rounded on its own
    -- two products and a sum, no fused multiply-add --, and the squared speed is evaluated once, so the kinetic energy's
    terms and `max_speed2` are the probe's (tests/probe_spec.py) bit for bit."""
    import torch
    vx, vy = velocities[:, 0], velocities[:, 1]
    speed2 = torch.add(torch.mul(vx, vx), torch.mul(vy, vy))
    return torch.stack([particles[:, 0], particles[:, 1], vx, vy, torch.mul(speed2, 0.5), pressure, speed2,
                        (pressure > 0).to(particles.dtype)], dim=1).contiguous()


def cluster_centers(table):
    """The centre of every cluster of a `Crate.cluster_observables` table: float64 (C, 2), (sum_x / n, sum_y / n)."""
    return table[:, 1:3] / table[:, 0:1]


def cluster_mean_velocities(table):
    """The mean velocity of every cluster of a `Crate.cluster_observables` table: float64 (C, 2)."""
    return table[:, 3:5] / table[:, 0:1]


def neighbor_mask(neighbors):
    """Which places of a nearest-k table (`Crate.neighbor_tensors`) hold a partner: bool (rows, k); the padding is -1."""
    return neighbors >= 0


def neighbor_edge_index(neighbors):
    """The (2, E) int64 edge list (row 0: the table's row, row 1: the partner) of a nearest-k table's valid places, in
    (row, place) order -- nearest first within a row.  With `queries` row 0 numbers the queries, not the points."""
    import torch
    rows, places = torch.nonzero(neighbor_mask(neighbors), as_tuple=True)  # (row-major: rows ascending, then places)
    return torch.stack([rows, neighbors[rows, places]])


def normalized(sums, wsum):
    """The Shepard-normalised field of `Crate.field_tensors(values, weight_sums=True)`: sums / wsum, row by row -- the
    weighted mean of the partners' values --, and 0 where wsum is 0 (a row without partners, or with none inside the
    radius at power >= 1).  `sums` is (rows, C) or (rows,), `wsum` (rows,)."""
    import torch
    w = wsum if sums.dim() == 1 else wsum.unsqueeze(1)
    return torch.where(w == 0, torch.zeros_like(sums), sums / w)


def shell_edges(radius, bins, inner=0.0):
    """B + 1 equal-width edges from `inner` to `radius` as a float64 NumPy array, for `Crate.distance_histogram`:
    ``edges[k] = inner + k * (radius - inner) / bins``, the last exactly `radius`."""
    import numpy as np
    bins = int(bins)
    radius, inner = float(radius), float(inner)
    if bins < 1 or not 0.0 <= inner < radius < float("inf"):
        raise ValueError("bins must be at least 1 and 0 <= inner < radius, both finite")
    edges = inner + np.arange(bins + 1, dtype=np.float64) * ((radius - inner) / bins)
    edges[-1] = radius
    return edges


def radial_distribution(total, edges, n, area):
    """The radial distribution function g(r) of `Crate.distance_histogram`'s totals, one value per bin, as a float64
    torch tensor: ``g[b] = total[b] / (n * (n / area) * pi * (edges[b + 1]**2 - edges[b]**2))`` -- the partners counted
    in the shell over the partners an ideal gas of the same density, n particles on `area`, would have there.  `total`
    counts ORDERED pairs, each unordered pair twice, as the self form of the histogram does: every one of the n
    particles looks around.  Edge effects are not corrected: particles near the boundary of `area` see fewer partners.

    Per cloud: with the (B, bins) `total` of `Crate.distance_histogram_batch`, `n` is the clouds' sizes -- a sequence or
    tensor of B numbers, ``batch[1:] - batch[:-1]`` -- and the result is (B, bins), row b the g(r) of cloud b by the same
    formula (an empty cloud's row is NaN: 0 / 0)."""
    import math

    import torch
    e = torch.as_tensor(edges, dtype=torch.float64, device=total.device)
    if e.dim() != 1 or e.shape[0] != total.shape[-1] + 1:
        raise ValueError("edges must have one entry more than total has bins")
    shell = math.pi * (e[1:] ** 2 - e[:-1] ** 2)
    if total.dim() == 1:
        return total.to(torch.float64) / (float(n) * (float(n) / float(area)) * shell)
    sizes = torch.as_tensor(n, dtype=torch.float64, device=total.device).reshape(-1)
    if total.dim() != 2 or sizes.shape[0] != total.shape[0]:
        raise ValueError("a (B, bins) total needs the B sizes of its clouds")
    return total.to(torch.float64) / ((sizes * (sizes / float(area)))[:, None] * shell[None, :])


def cluster_cloud(cluster_ptr, clusters=None):
    """The cloud of every cluster of `Crate.cluster_tensors_batch` and `cluster_sums_batch`: int64 (C,), cluster c
    lies in cloud b iff ``cluster_ptr[b] <= c < cluster_ptr[b + 1]`` -- `batch_index` over the clusters.  `clusters`
    defaults to ``cluster_ptr[-1]`` (which then synchronises to read it)."""
    return batch_index(cluster_ptr, clusters)


def grid_queries(x0, x1, y0, y1, nx, ny, device=None):
    """The centres of the nx x ny cells of the rectangle [x0, x1] x [y0, y1] as a float64 (nx * ny, 2) tensor of
    queries in row-major order, y the slow axis: query iy * nx + ix is (x0 + (ix + 0.5) (x1 - x0) / nx,
    y0 + (iy + 0.5) (y1 - y0) / ny).  `Crate.field_tensors(v, queries=grid_queries(...))[0].reshape(ny, nx, -1)` is an
    image of the field, row 0 at y0."""
    import torch
    if nx < 0 or ny < 0:
        raise ValueError("nx and ny must not be negative")
    x = x0 + (torch.arange(nx, dtype=torch.float64, device=device) + 0.5) * ((x1 - x0) / nx if nx else 0.0)
    y = y0 + (torch.arange(ny, dtype=torch.float64, device=device) + 0.5) * ((y1 - y0) / ny if ny else 0.0)
    return torch.stack([x.repeat(ny), y.repeat_interleave(nx)], dim=1)


def ray_fan(origin, count, start_angle, stop_angle, device=None):
    """`count` rays from one point for `Crate.ray_tensors`: ``(origins, directions)``, float64 (count, 2) each -- every
    origin is `origin`, direction k is ``(cos a_k, sin a_k)`` with ``a_k = start_angle + k * (stop_angle - start_angle) /
    (count - 1)``, both ends included (one ray looks along `start_angle`), in radians, counter-clockwise from +x.  The
    angles, cosines and sines are NumPy's float64; the directions are unit up to rounding, so t is the distance."""
    import numpy as np
    import torch
    count = int(count)
    if count < 0:
        raise ValueError("count must not be negative")
    start_angle, stop_angle = float(start_angle), float(stop_angle)
    step = (stop_angle - start_angle) / (count - 1) if count > 1 else 0.0
    angles = start_angle + np.arange(count, dtype=np.float64) * step
    directions = torch.from_numpy(np.stack([np.cos(angles), np.sin(angles)], axis=1))
    at = np.array([float(origin[0]), float(origin[1])], dtype=np.float64)
    origins = torch.from_numpy(np.tile(at, (count, 1)))
    return (origins, directions) if device is None else (origins.to(device), directions.to(device))


def ray_points(origins, directions, t):
    """Where the rays of `Crate.ray_tensors` ended: float64 (R, 2), ``origins + t[:, None] * directions`` -- product
    and sum rounded on their own --, NaN in both columns where nothing was hit (t = +inf) and for a dead ray (t = NaN)."""
    import torch
    seen = torch.isfinite(t).unsqueeze(1)
    ends = torch.add(origins, torch.mul(t.unsqueeze(1), directions))
    return torch.where(seen, ends, torch.full_like(ends, float("nan")))


def hit_particles(hit):
    """The particle every ray of `Crate.ray_tensors` hit: int64 (R,), the row of `state_tensors()`, -1 for a wall or nothing."""
    import torch
    return torch.where(hit >= 0, hit, torch.full_like(hit, -1))


def hit_walls(hit):
    """The wall segment every ray of `Crate.ray_tensors` hit: int64 (R,), the row of `segments`, -1 for a particle or nothing."""
    import torch
    return torch.where(hit <= -2, -2 - hit, torch.full_like(hit, -1))


RayPaths = collections.namedtuple("RayPaths", "t hit points normals end")  # what `Crate.ray_paths` returns


def path_legs(hit):
    """How many legs of every path of `Crate.ray_paths` hit something: int64 (R,) from `hit`, int64 (R, L).  The legs
    that hit come first: ``hit[r, :path_legs(hit)[r]]`` are they, and a leg is -1 when it met nothing or was never reached."""
    return (hit != -1).sum(dim=1)


def path_arrows(origins, points, hit):
    """The travelled legs of the paths of `Crate.ray_paths` as the (start, direction) pairs `render(arrows=...)` draws: a
    host float64 array (K, 2, 2), ray by ray and leg by leg.  Leg k of a ray that hit goes from the point of leg k - 1
    -- from the origin for k = 0 -- to ``points[r, k]``, and its direction is the difference of the two; a leg that met
    nothing has no end point and gives no arrow.  Synchronises: it copies the three tensors to the host."""
    import numpy as np
    import torch
    starts = torch.cat([origins.unsqueeze(1), points[:, :-1]], dim=1)
    pairs = torch.stack([starts, points - starts], dim=2)
    return np.ascontiguousarray(pairs[hit != -1].cpu().numpy()).reshape(-1, 2, 2)
