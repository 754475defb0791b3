"""Time of the per-cluster sums against the two torch routes over the labels.

    python scripts/cluster_sums_time.py [--reps 30] [--ticks 200] [--big 1048576] [--only states|points]

Two states, the ones scripts/clusters_time.py uses: config/wave_machine.yaml after --ticks ticks (the viewer's size) and
--big synthetic particles (bench.py's world and generator) after three ticks; the values are the eight channels of
`Crate.cluster_observables`.  Then four clouds of --big points through `points=` with eight seeded channels:

  cloud 2 partners   uniform in the unit square at 2 expected partners: many small clusters
  singletons         a lattice with the radius just below its spacing: every point a cluster, one live lane per wave
  giant, raster      the lattice at radius = spacing: one cluster, its members in index order
  giant, shuffled    the same cluster with the indices permuted: the gather of level 0 is scattered

Per input, with sums, minima and maxima of 8 channels:

  cluster_sums     `Crate.cluster_sums(values, extrema=True)`: wall time of the whole call -- count (half), label, reduce,
                   one synchronisation, the 16-byte read
  index_add        `Crate.cluster_tensors()` + ``zeros.index_add_(0, labels, values)``: float atomics, sums only, the bits
                   differ from call to call
  segment_reduce   `Crate.cluster_tensors()` + a stable sort of the labels + a gather + ``torch.segment_reduce`` (sum):
                   deterministic, sums only
  reduce           `Engine.pairs_cluster_sums` after one count and one label, into tensors made once: device time between
                   HIP events on the stream the library runs on, the count's and the label's next to it, and the number of
                   launches of one reduction

The sides alternate inside one loop, the call in question last.  Before anything is timed the device result is compared
with the NumPy rule (tests/cluster_sums_spec.py) over the device's own labels, byte for byte.  One JSON line per case:
median and min over the repetitions, in microseconds.
"""
import argparse
import json

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, viewer_crate

WARMUP = 2                            # rounds before anything is recorded, wall and device alike


def reduce_launches(bound):
    """The launches of one sc_pairs_cluster_sums_device over a host bound of `bound` points: the check, four per pass of
    the sort, the scans of the sizes (2), of the chunks (3) and -- with more than one level -- of the partials and of the
    items of level 1 (3 each), the item list, three more per level from the third on, a reduction per level, the finish."""
    passes = max(1, -(-int(bound).bit_length() // 8))
    levels = 1
    while 64 ** levels < bound:
        levels += 1
    return {"launches": 1 + 4 * passes + 2 + 3 + 1 + (6 if levels > 1 else 0) + 3 * max(0, levels - 2) + levels + 1,
            "sort_passes": passes, "levels": levels}


def rule(labels, values, total):
    """tests/cluster_sums_spec.py over many clusters.  Those of at most 64 members are one group of the tree: the clusters
    of 2^(k-1) < size <= 2^k members are reduced together, padded with +0.0 to 2^k -- k rounds of neighbours -- and the
    rest of the group's padding is one more + 0.0 (every further one changes nothing).  The larger ones go through the
    spec itself.  Minima and maxima do not depend on order: NumPy's reduceat over the members."""
    import cluster_sums_spec as spec
    alive = np.flatnonzero(labels >= 0)
    order = alive[np.argsort(labels[alive], kind="stable")]
    lab = labels[order]
    sizes = np.bincount(lab, minlength=total)
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    rank = np.arange(len(order)) - starts[lab]
    width = values.shape[1]
    rows = values[order]
    sums = np.empty((total, width))
    with np.errstate(all="ignore"):
        mins = np.minimum.reduceat(rows, starts, axis=0) if total else np.empty((0, width))
        maxs = np.maximum.reduceat(rows, starts, axis=0) if total else np.empty((0, width))
        p = 1
        while p <= spec.GROUP:
            which = np.flatnonzero((sizes <= p) & (sizes > p // 2))
            slot = np.full(total, -1, dtype=np.int64)
            slot[which] = np.arange(len(which))
            member = slot[lab] >= 0
            a = np.zeros((len(which), p, width))
            a[slot[lab[member]], rank[member]] = rows[member]
            while a.shape[1] > 1:
                a = a[:, 0::2] + a[:, 1::2]
            sums[which] = a[:, 0] + 0.0 if p < spec.GROUP else a[:, 0]
            p *= 2
    for c in np.flatnonzero(sizes > spec.GROUP):
        sums[c] = spec.cluster_sums(np.zeros(sizes[c], dtype=np.int64), rows[starts[c]:starts[c] + sizes[c]], clusters=1,
                                    extrema=False)[0][0]
    return sums, mins, maxs


def check(name, got, values):
    import cluster_sums_spec as spec
    labels, sizes = got[0].cpu().numpy(), got[1].cpu().numpy()
    if not np.array_equal(np.bincount(labels[labels >= 0], minlength=len(sizes)), sizes):
        raise SystemExit(f"{name}: the sizes differ from the labels")
    want = rule(labels, values.cpu().numpy(), len(sizes))
    for g, w, what in zip(got[3:], want, ("sums", "mins", "maxs")):
        if not spec.same(g.cpu().numpy(), w):
            raise SystemExit(f"{name}: the {what} differ from the rule")


def torch_routes(crate, radius, points, values):
    import torch

    def index_add():
        labels, sizes, _ = crate.cluster_tensors(radius, points=points)
        keep = labels >= 0
        out = torch.zeros((len(sizes), values.shape[1]), dtype=torch.float64, device=values.device)
        out.index_add_(0, labels[keep], values[:len(labels)][keep])
        torch.cuda.synchronize()
        return out

    def segment_reduce():
        labels, sizes, _ = crate.cluster_tensors(radius, points=points)
        order = torch.sort(labels, stable=True).indices
        order = order[int((labels < 0).sum()):]                                     # (dead rows sort first: label -1)
        out = torch.segment_reduce(values[:len(labels)][order], "sum", lengths=sizes, axis=0)
        torch.cuda.synchronize()
        return out

    return index_add, segment_reduce


def reduce_device(eng, points, radius, rows, values, reps):
    """Device time of the count (half), the label and the reduction, by events, into tensors made once."""
    import torch
    dev = torch.device("cuda", eng.device)
    offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    labels, sizes, roots = (torch.empty(rows, dtype=torch.int64, device=dev) for _ in range(3))
    tables = [torch.empty((rows, values.shape[1]), dtype=torch.float64, device=dev) for _ in range(3)]
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True),
        "label": lambda: eng.pairs_label(labels, sizes, roots, counts=counts),
        "reduce": lambda: eng.pairs_cluster_sums(values, *tables, counts=counts)}, reps, WARMUP)
    n, total = (int(v) for v in counts.cpu())
    out = {"n": n, "C": total}
    for name, t in times.items():
        out.update(stats(t, f"{name}_device_"))
    return {**out, **reduce_launches(n)}


def measure(crate, base, radius, points, values, rows, reps):
    import torch
    got = crate.cluster_sums(values, radius, points=points, extrema=True)
    check(base.get("input") or base.get("state"), got, values)
    sizes = got[1]
    base = {**base, "C": len(sizes), "largest": int(sizes.max()) if len(sizes) else 0}
    index_add, segment_reduce = torch_routes(crate, radius, points, values)
    sides = {"index_add": index_add, "segment_reduce": segment_reduce}
    first = {}
    for name in list(sides):
        try:
            first[name] = sides[name]()
        except RuntimeError as err:                                                 # (a torch build without the operator)
            print(json.dumps({**base, "case": name, "unavailable": str(err).splitlines()[0]}), flush=True)
            del sides[name]
    if len(first) == 2:
        base["index_add_equals_segment_reduce"] = bool(torch.equal(*first.values()))
    sides["cluster_sums"] = lambda: crate.cluster_sums(values, radius, points=points, extrema=True)
    times = alternate(sides, reps, WARMUP)
    for name, t in times.items():
        print(json.dumps({**base, "case": name, **stats(t, "wall_")}), flush=True)
    print(json.dumps({**base, "case": "reduce", **reduce_device(crate.engine, points, radius, rows, values, reps)}), flush=True)
    med = {name: median(t) for name, t in times.items()}
    print(json.dumps({**base, "case": "verdict", **{f"cluster_sums_over_{name}": round(med["cluster_sums"] / t, 4)
                                                  for name, t in med.items() if name != "cluster_sums"}}), flush=True)
    torch.cuda.synchronize()


def measure_state(crate, base, reps):
    from sand_crate_amd import pairs
    values = pairs.cluster_channels(*crate.state_tensors())
    measure(crate, base, crate.diameter, None, values, crate.engine.capacity, reps)


def measure_points(crate, big, reps):
    import torch
    import pairs_cases
    side = int(round(np.sqrt(big)))
    spacing = 1.0 / side
    c = np.arange(side, dtype=np.float64) * spacing
    x, y = np.meshgrid(c, c)
    grid = np.stack([x.ravel(), y.ravel()], axis=1)
    cloud, cloud_radius = pairs_cases.cloud(91, big, 2.0)
    shuffled = grid[np.random.RandomState(92).permutation(len(grid))]
    inputs = {"cloud 2 partners": (cloud, cloud_radius), "singletons": (grid, 0.999 * spacing), "giant, raster": (grid, spacing),
              "giant, shuffled": (shuffled, spacing)}
    rs = np.random.RandomState(93)
    for name, (pts, radius) in inputs.items():
        values = torch.from_numpy(rs.standard_normal((len(pts), 8))).cuda()
        t = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        measure(crate, {"input": name, "points": len(pts), "radius": radius}, radius, t, values, len(pts), reps)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--only", choices=["states", "points"], default=None)
    args = ap.parse_args()
    import torch
    torch.cuda.init()

    big_reps = max(5, args.reps // 3)
    if args.only != "points":
        crate = viewer_crate(args.ticks)
        measure_state(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps)
        crate.engine.close()

    if args.only == "points":                                                       # (an empty crate: the points come through `points=`)
        import bench
        import sand_crate_amd as sc
        crate = sc.Crate(bench.world_for(args.big)[0], noise="counter", noise_seed=1, capacity=args.big + 1024)
    else:
        crate = bench_crate(args.big, 3)
        measure_state(crate, {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}, big_reps)
    if args.only != "states":
        measure_points(crate, args.big, big_reps)


if __name__ == "__main__":
    main()
