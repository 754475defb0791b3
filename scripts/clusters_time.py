"""Time of the device cluster labelling against the pair search it rides on and against the floor of the host route.

    python scripts/clusters_time.py [--reps 30] [--ticks 200] [--big 1048576] [--only states|points]

Two states, the ones scripts/pairs_time.py uses: config/wave_machine.yaml after --ticks ticks (the viewer's size) and --big
synthetic particles (bench.py's world and generator) after three ticks.  Radius = the crate's diameter.  Per state:

  cluster_tensors  `Crate.cluster_tensors()`: wall time of the whole call -- five allocations, count (half), label, one
                   synchronisation, the 16-byte read of (n, C)
  pair_tensors     `Crate.pair_tensors(half=True)` on the same state: wall time of the whole call
  download         `Engine.download()`: wall time of the call -- the floor of the host route, before any search
  label            `Engine.pairs_label` after one `Engine.pairs_count`, into tensors made once: device time between HIP
                   events on the stream the library runs on, the count's time next to it, and the number of launches of a
                   label (init, union, the jumps, mark, two of the scan, write, finish)

Then three inputs of --big points through `points=`, labelled the same way (device time of count and of label):

  cloud            uniform in the unit square at 6 expected partners
  lattice          sqrt(big) x sqrt(big) in raster order, radius = spacing: the deepest parent chains the union kernel builds
  lattice, no edges  the same points with the radius just below the spacing: every launch of a label with nothing to unite
                   and nothing to jump -- what the launches cost when the data costs nothing

and the ratio lattice / cloud.  The sides of a comparison alternate inside one loop, in the order download, pair_tensors,
cluster_tensors (the order of scripts/pairs_time.py: the call in question last).  Before anything is timed the device
result is compared with the NumPy rule (tests/cluster_spec.py): `clusters` on the small state, `components` over the
device's own half list on the big state and the cloud, the closed form on the lattices.  One JSON line per case: median
and min over the repetitions, in microseconds.
"""
import argparse
import json

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, viewer_crate, with_wall

WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def label_launches(bound):
    """The launches of one sc_pairs_label_device over a host bound of `bound` points (the point count, or for the state
    the number of slots in use: n, unless particles have left)."""
    jumps = max(1, int(np.ceil(np.log2(max(bound, 2)))))
    return {"launches": 2 + jumps + 1 + 2 + 2, "jump_launches": jumps}


def label_device(eng, points, radius, rows, reps):
    """Device time of the count (half) and of the label, by events, into tensors made once."""
    import torch
    dev = torch.device("cuda", eng.device)
    offsets = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    labels, sizes, roots = (torch.empty(rows, dtype=torch.int64, device=dev) for _ in range(3))
    wall = []
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, half=True),
        "label": with_wall(lambda: eng.pairs_label(labels, sizes, roots, counts=counts), wall)}, reps, WARMUP)
    n, total = (int(v) for v in counts.cpu())
    out = {**stats(times["count"], "count_device_"), **stats(times["label"], "label_device_"),
           **stats(wall[-reps:], "label_enqueue_wall_"), "n": n, "C": total, **label_launches(n)}
    return out, (labels[:n], sizes[:total], roots[:total])


def same(got, want):
    return all(g.cpu().numpy().tobytes() == np.ascontiguousarray(w, dtype=np.int64).tobytes() for g, w in zip(got, want))


def propagated(crate, radius, points, n):
    import cluster_spec
    offsets, partners = crate.pair_tensors(radius, points=points, half=True)
    return cluster_spec.components(n, offsets.cpu().numpy(), partners.cpu().numpy())


def measure_state(crate, base, reps, small):
    import torch
    import cluster_spec
    eng = crate.engine
    got = crate.cluster_tensors()
    n = len(got[0])
    want = (cluster_spec.clusters(crate.state_tensors()[0].cpu().numpy(), crate.diameter) if small
            else propagated(crate, crate.diameter, None, n))
    if not same(got, want):
        raise SystemExit("cluster_tensors differs from the rule")
    base = {**base, "C": len(got[1]), "largest": int(got[1].max()) if len(got[1]) else 0}
    times = alternate({"download": eng.download, "pair_tensors": lambda: crate.pair_tensors(half=True),
                       "cluster_tensors": crate.cluster_tensors}, reps, WARMUP)
    for name, t in times.items():
        print(json.dumps({**base, "case": name, **stats(t, "wall_")}), flush=True)
    dev, _ = label_device(eng, None, crate.diameter, eng.capacity, reps)
    print(json.dumps({**base, "case": "label", **dev}), flush=True)
    med = {name: median(t) for name, t in times.items()}
    print(json.dumps({**base, "case": "verdict", "cluster_tensors_over_pair_tensors": round(med["cluster_tensors"] / med["pair_tensors"], 4),
                      "cluster_tensors_over_download": round(med["cluster_tensors"] / med["download"], 4)}), flush=True)
    torch.cuda.synchronize()


def measure_points(crate, big, reps):
    import torch
    import pairs_cases
    side = int(round(np.sqrt(big)))
    cloud, cloud_radius = pairs_cases.cloud(91, big, 6.0)
    spacing = 1.0 / side
    c = np.arange(side, dtype=np.float64) * spacing
    x, y = np.meshgrid(c, c)
    grid = np.stack([x.ravel(), y.ravel()], axis=1)
    inputs = {"cloud": (cloud, cloud_radius), "lattice": (grid, spacing), "lattice, no edges": (grid, 0.999 * spacing)}
    medians = {}
    for name, (pts, radius) in inputs.items():
        t = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        dev, got = label_device(crate.engine, t, radius, len(pts), reps)
        n = len(pts)
        if name == "cloud":
            ok = same(got, propagated(crate, radius, t, n))
        elif name == "lattice":
            ok = not bool(got[0].any()) and got[1].tolist() == [n] and got[2].tolist() == [0]
        else:
            k = torch.arange(n, device=got[0].device)
            ok = torch.equal(got[0], k) and torch.equal(got[2], k) and bool((got[1] == 1).all())
        if not ok:
            raise SystemExit(f"{name}: the labels differ from the rule")
        medians[name] = dev["label_device_median_us"]
        print(json.dumps({"input": name, "points": n, "radius": radius, "case": "label", **dev}), flush=True)
    print(json.dumps({"case": "verdict", "label_lattice_over_cloud": round(medians["lattice"] / medians["cloud"], 3),
                      "label_no_edges_over_cloud": round(medians["lattice, no edges"] / medians["cloud"], 3)}), flush=True)


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
        measure_state(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps, True)
        crate.engine.close()

    if args.only == "points":                                                       # (an empty crate: the points come through `points=`)
        import bench
        import sand_crate_amd as sc
        crate = sc.Crate(bench.world_for(args.big)[0], noise="counter", noise_seed=1, capacity=args.big + 1024)
    else:
        crate = bench_crate(args.big, 3)
        measure_state(crate, {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}, big_reps, False)
    if args.only != "states":
        measure_points(crate, args.big, big_reps)


if __name__ == "__main__":
    main()
