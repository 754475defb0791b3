"""Time of the device distance histograms against the route there was for the same counts: the CSR pair list, then torch.

    timeout -k 10 900 python scripts/hist_time.py [--reps 30] [--ticks 200] [--big 1048576] [--probes 65536] [--lib PATH]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above: a step that hangs then ends
the run too).  Two states, the ones scripts/fields_time.py uses: config/wave_machine.yaml after --ticks ticks (the
viewer's size) and --big synthetic particles (bench.py's world and generator) after three ticks.  Per state, per radius
-- the crate's diameter and twice the diameter --, per number of bins B -- 16 and 64 equal-width bins from 0 to the radius
(`pairs.shell_edges`) -- and per output -- the totals only, and the table with the totals:

  distance_histogram  `Crate.distance_histogram(edges[, per_row=True])`: wall time of the whole call -- the allocations,
                      count, histogram, ONE synchronisation, the 16-byte read of (rows, status)
  list route          what there was before: `Crate.pair_tensors(radius, squared_distances=True)` and the torch code that
                      turns the list into the counts (`counts_from_list`: bucketize on the squared distances, bincount
                      for the totals; for the table a repeat_interleave and a bincount over rows * B + bin), ending in a
                      synchronisation: wall time, and the pair_tensors part of it
  kernels             `Engine.pairs_count`, `Engine.pairs_hist`, `Engine.pairs_sum` (the weight sums alone, power 3, of
                      the same grid: k_fields_sum's merge with nothing to gather) and `Engine.pairs_fill` (with d2) into
                      tensors made once: device time between HIP events on the stream the library runs on -- the
                      histogram is its memset and two or three launches (the check, the histogram itself, the copy of the
                      totals).  The count is the whole of sc_pairs_count_device: the binning sort, the scans and
                      k_pairs_count's walk
  probes              (big state) `Crate.distance_histogram(edges, queries=, per_row=True)` with --probes random probes
                      inside the state's bounding box: wall time of the call, and the device time of the query-form
                      histogram alone

The sides of a comparison alternate inside one loop, the call in question last.  Before anything is timed the list
route's counts are compared with the kernel's -- integers: they must be equal -- and on the small state the kernel's with
the NumPy rule (tests/hist_spec.py).  `--lib` times another build of the library through the same script.  One JSON line
per case: median and min over the repetitions, microseconds.
"""
import argparse
import json
import time

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, use_library, viewer_crate

WARMUP = 3                            # rounds before anything is recorded, wall and device alike

BINS = (16, 64)


def counts_from_list(offsets, partners, d2, e2, per_row):
    """(table or None, total) of a full CSR pair list with squared distances; e2[0] is 0, so every pair is in a bin."""
    import torch
    bins = e2.shape[0] - 1
    idx = (torch.bucketize(d2, e2, right=True) - 1).clamp_(max=bins - 1)        # (the last bin is closed on top)
    total = torch.bincount(idx, minlength=bins)
    if not per_row:
        return None, total
    n = offsets.shape[0] - 1
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=offsets.device), offsets[1:] - offsets[:-1])
    table = torch.bincount(rows * bins + idx, minlength=n * bins).view(n, bins).to(torch.int32)
    return table, total


def kernels(crate, edges, per_row, reps, total_pairs, queries=None):
    """Device time of count, histogram, weight sums and fill by events, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    radius = float(edges[-1])
    bins = len(edges) - 1
    rows = eng.capacity if queries is None else int(queries.shape[0])
    offsets = torch.empty(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts, other, third = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(3))
    table = torch.empty((rows, bins), dtype=torch.int32, device=dev) if per_row else None
    total = torch.empty(bins, dtype=torch.int64, device=dev)
    wsum = torch.empty(rows, dtype=torch.float64, device=dev)
    partners = torch.empty(total_pairs, dtype=torch.int64, device=dev)
    d2 = torch.empty(total_pairs, dtype=torch.float64, device=dev)
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts),
        "hist": lambda: eng.pairs_hist(table, total, edges=edges, queries=queries, counts=other),
        "wsum": lambda: eng.pairs_sum(None, None, wsum, power=3, queries=queries, counts=third),
        "fill": lambda: eng.pairs_fill(partners, d2)}, reps, WARMUP)
    n_rows, status = (int(v) for v in other.cpu())
    if status != 0:
        raise SystemExit(f"kernels: status {status}")
    return {**stats(times["count"], "count_device_"), **stats(times["hist"], "hist_device_"), **stats(times["wsum"], "wsum_device_"),
            **stats(times["fill"], "fill_device_"), "rows": n_rows, "hist_bytes": 8 * bins + (4 * n_rows * bins if per_row else 0),
            "list_bytes": 16 * total_pairs, "hist_over_count": round(median(times["hist"]) / median(times["count"]), 3),
            "hist_over_wsum": round(median(times["hist"]) / median(times["wsum"]), 3)}


def measure(crate, base, reps, check_rule):
    import torch
    from sand_crate_amd import pairs
    particles, = crate.state_tensors(pressure=False)[:1]
    n = int(particles.shape[0])
    for factor in (1.0, 2.0):
        radius = factor * crate.diameter
        offsets, partners, d2 = crate.pair_tensors(radius, squared_distances=True)
        total_pairs = len(partners)
        for bins in BINS:
            edges = pairs.shell_edges(radius, bins)
            e2 = torch.from_numpy(edges * edges).to(particles.device)
            want = counts_from_list(offsets, partners, d2, e2, True)
            got = crate.distance_histogram(edges, per_row=True)
            if not (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and int(got[1].sum()) == total_pairs):
                raise SystemExit(f"B={bins}: the kernel's counts differ from the list route's")
            if check_rule:
                import hist_spec
                rule = hist_spec.histogram(particles.cpu().numpy(), edges)
                if not (np.array_equal(got[0].cpu().numpy(), rule[0]) and np.array_equal(got[1].cpu().numpy(), rule[1])):
                    raise SystemExit(f"B={bins}: distance_histogram differs from the rule")
            del want, got
            for per_row in (False, True):
                case = {**base, "bins": bins, "radius_in_diameters": factor, "table": per_row, "E": total_pairs,
                        "E_per_n": round(total_pairs / max(n, 1), 3)}
                part = []

                def list_route():
                    t0 = time.perf_counter()
                    o, p, d = crate.pair_tensors(radius, squared_distances=True)
                    part.append(1e6 * (time.perf_counter() - t0))
                    counts_from_list(o, p, d, e2, per_row)
                    torch.cuda.synchronize()

                times = alternate({"list route": list_route,
                                   "distance_histogram": lambda: crate.distance_histogram(edges, per_row=per_row)},
                                  reps, WARMUP)
                print(json.dumps({**case, "case": "list route", **stats(times["list route"], "wall_"),
                                  **stats(part[-reps:], "pair_tensors_part_wall_")}), flush=True)
                print(json.dumps({**case, "case": "distance_histogram", **stats(times["distance_histogram"], "wall_")}), flush=True)
                print(json.dumps({**case, "case": "kernels", **kernels(crate, edges, per_row, reps, total_pairs)}), flush=True)
                med = {name: median(t) for name, t in times.items()}
                print(json.dumps({**case, "case": "verdict", "distance_histogram_over_list_route":
                                  round(med["distance_histogram"] / med["list route"], 4)}), flush=True)
        del offsets, partners, d2
        torch.cuda.empty_cache()


def measure_queries(crate, base, reps, queries):
    import torch
    from sand_crate_amd import pairs
    radius = crate.diameter
    points, = crate.state_tensors(pressure=False)[:1]
    for bins in BINS:
        edges = pairs.shell_edges(radius, bins)
        table, total = crate.distance_histogram(edges, queries=queries, per_row=True)
        # the rule on a sample: brute force over all points, the arithmetic of the kernel
        sample = queries[:64]
        dx, dy = sample[:, None, 0] - points[None, :, 0], sample[:, None, 1] - points[None, :, 1]
        dist = dx * dx + dy * dy
        e2 = torch.from_numpy(edges * edges).to(points.device)
        idx = (torch.bucketize(dist, e2, right=True) - 1).clamp_(max=bins - 1)
        inside = dist <= e2[-1]
        want = torch.stack([((idx == b) & inside).sum(dim=1) for b in range(bins)], dim=1).to(torch.int32)
        if not (torch.equal(table[:64], want) and torch.equal(total, table.sum(0))):
            raise SystemExit("probes: the table differs from the brute force")
        del dx, dy, dist, idx, inside
        times = alternate({"distance_histogram": lambda: crate.distance_histogram(edges, queries=queries, per_row=True)},
                          reps, WARMUP)
        case = {**base, "bins": bins, "radius_in_diameters": 1.0, "table": True, "queries": int(queries.shape[0]),
                "partners": int(total.sum())}
        print(json.dumps({**case, "case": "probes: distance_histogram", **stats(times["distance_histogram"], "wall_")}), flush=True)
        dev = kernels(crate, edges, True, reps, 1, queries)
        dev = {key: v for key, v in dev.items() if not key.startswith("fill") and key != "list_bytes"}
        print(json.dumps({**case, "case": "probes: kernels", **dev}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--probes", type=int, default=65536)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    use_library(args.lib)

    crate = viewer_crate(args.ticks)
    measure(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps, True)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    base = {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}
    big_reps = max(5, args.reps // 3)
    measure(crate, base, big_reps, False)
    points = crate.state_tensors()[0]
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    gen = torch.Generator(device=points.device).manual_seed(11)
    probes = lo + (hi - lo) * torch.rand((args.probes, 2), dtype=torch.float64, device=points.device, generator=gen)
    torch.cuda.synchronize()
    measure_queries(crate, base, big_reps, probes)


if __name__ == "__main__":
    main()
