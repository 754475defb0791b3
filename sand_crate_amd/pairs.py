"""Small torch helpers for the CSR pair lists of `Crate.pair_tensors` (offsets, partners) and for the clusters of
`Crate.cluster_tensors` (labels, sizes), and for the nearest-k tables of `Crate.neighbor_tensors` (neighbors)."""
from __future__ import annotations


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


def neighbor_mask(neighbors):
    """Which places of a nearest-k table (`Crate.neighbor_tensors`) hold a partner: bool (rows, k); the padding is -1."""
    return neighbors >= 0


def neighbor_edge_index(neighbors):
    """The (2, E) int64 edge list (row 0: the table's row, row 1: the partner) of a nearest-k table's valid places, in
    (row, place) order -- nearest first within a row.  With `queries` row 0 numbers the queries, not the points."""
    import torch
    rows, places = torch.nonzero(neighbor_mask(neighbors), as_tuple=True)  # (row-major: rows ascending, then places)
    return torch.stack([rows, neighbors[rows, places]])
