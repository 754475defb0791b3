"""Time of the device nearest-k tables against the route there was for the same table: the CSR pair list, then torch.

    python scripts/nearest_time.py [--reps 30] [--ticks 200] [--big 1048576] [--probes 65536]

Two states, the ones scripts/pairs_time.py uses: config/wave_machine.yaml after --ticks ticks (the viewer's size) and --big
synthetic particles (bench.py's world and generator) after three ticks.  Per state and per (k, radius) -- k = 16 and k = 64
at radius = the crate's diameter, k = 32 at twice the diameter:

  neighbor_tensors   `Crate.neighbor_tensors(k, radius, squared_distances=True)`: wall time of the whole call -- the
                     allocations, count, table, ONE synchronisation, the 16-byte read of (rows, cut)
  list route         what there was before: `Crate.pair_tensors(radius, squared_distances=True)` and the torch code that
                     turns the list into the table (`table_from_list`: two stable sorts, by d2 and then by row, and a
                     scatter into (n, k)), ending in a synchronisation: wall time, and the pair_tensors part of it
  kernels            `Engine.pairs_count`, `Engine.pairs_nearest` (with d2) and `Engine.pairs_fill` (with d2) of the same grid
                     into tensors made once: device time between HIP events on the stream the library runs on, and the
                     bytes the table and the list take
  probes             (big state) `Crate.neighbor_tensors(16, queries=)` with --probes random probes inside the state's
                     bounding box: wall time of the call, and the device time of the query-form table alone

The sides of a comparison alternate inside one loop, the call in question last.  Before anything is timed the list
route's table is asserted equal to the kernel's, bit for bit, neighbors and d2, and on the small state both are compared
with the NumPy rule (tests/nearest_spec.py).  One JSON line per case: median and min over the repetitions, microseconds.
"""
import argparse
import json
import time

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, use_library, viewer_crate

WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def table_from_list(offsets, partners, d2, k):
    """The (n, k) table of a full CSR pair list with distances: every row sorted by (d2, j) and cut at k."""
    import torch
    n = offsets.shape[0] - 1
    dev = offsets.device
    lengths = offsets[1:] - offsets[:-1]
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), lengths)
    by_d2 = torch.argsort(d2, stable=True)                              # (a row ascends in j: the ties stay in j order)
    order = by_d2[torch.argsort(rows[by_d2], stable=True)]              # ... then by row: (row, d2, j)
    place = torch.arange(rows.shape[0], dtype=torch.int64, device=dev) - offsets[rows]
    keep = place < k
    neighbors = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    distances = torch.full((n, k), float("inf"), dtype=torch.float64, device=dev)
    at = rows[keep] * k + place[keep]
    neighbors.view(-1)[at] = partners[order][keep]
    distances.view(-1)[at] = d2[order][keep]
    return neighbors, distances


def kernels(crate, radius, k, reps, total, queries=None):
    """Device time of count, table and fill by events, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    rows = eng.capacity if queries is None else int(queries.shape[0])
    offsets = torch.empty(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts, other = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2))
    neighbors = torch.empty((rows, k), dtype=torch.int64, device=dev)
    table_d2 = torch.empty((rows, k), dtype=torch.float64, device=dev)
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts),
        "table": lambda: eng.pairs_nearest(neighbors, table_d2, k=k, queries=queries, counts=other),
        "fill": lambda: eng.pairs_fill(partners, d2)}, reps, WARMUP)
    n_rows, cut = (int(v) for v in other.cpu())
    return {**stats(times["count"], "count_device_"), **stats(times["table"], "table_device_"), **stats(times["fill"], "fill_device_"),
            "rows": n_rows, "rows_cut": cut, "table_bytes": 16 * n_rows * k, "list_bytes": 16 * total,
            "table_over_fill": round(median(times["table"]) / median(times["fill"]), 3)}


def measure(crate, base, reps, shapes, check_rule):
    import torch
    for k, factor in shapes:
        radius = factor * crate.diameter
        offsets, partners, d2 = crate.pair_tensors(radius, squared_distances=True)
        n, total = len(offsets) - 1, len(partners)
        want = table_from_list(offsets, partners, d2, k)
        got = crate.neighbor_tensors(k, radius, squared_distances=True, partner_counts=True)
        if not (torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], offsets[1:] - offsets[:-1])):
            raise SystemExit(f"k={k}: the kernel's table differs from the list route's")
        if check_rule:
            import nearest_spec
            rule = nearest_spec.nearest(crate.state_tensors()[0].cpu().numpy(), radius, k)
            if any(g.cpu().numpy().tobytes() != w.tobytes() for g, w in zip(got, rule)):
                raise SystemExit(f"k={k}: neighbor_tensors differs from the rule")
        del want, got
        case = {**base, "k": k, "radius_in_diameters": factor, "E": total, "E_per_n": round(total / max(n, 1), 3)}
        part = []

        def list_route():
            t0 = time.perf_counter()
            o, p, d = crate.pair_tensors(radius, squared_distances=True)
            part.append(1e6 * (time.perf_counter() - t0))
            table_from_list(o, p, d, k)
            torch.cuda.synchronize()

        times = alternate({"list route": list_route,
                           "neighbor_tensors": lambda: crate.neighbor_tensors(k, radius, squared_distances=True)},
                          reps, WARMUP)
        print(json.dumps({**case, "case": "list route", **stats(times["list route"], "wall_"),
                          **stats(part[-reps:], "pair_tensors_part_wall_")}), flush=True)
        print(json.dumps({**case, "case": "neighbor_tensors", **stats(times["neighbor_tensors"], "wall_")}), flush=True)
        print(json.dumps({**case, "case": "kernels", **kernels(crate, radius, k, reps, total)}), flush=True)
        med = {name: median(t) for name, t in times.items()}
        print(json.dumps({**case, "case": "verdict",
                          "neighbor_tensors_over_list_route": round(med["neighbor_tensors"] / med["list route"], 4)}), flush=True)
        del offsets, partners, d2
        torch.cuda.empty_cache()


def measure_probes(crate, base, reps, probes):
    import torch
    k, radius = 16, crate.diameter
    points = crate.state_tensors()[0]
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    gen = torch.Generator(device=points.device).manual_seed(11)
    queries = lo + (hi - lo) * torch.rand((probes, 2), dtype=torch.float64, device=points.device, generator=gen)
    torch.cuda.synchronize()
    # the rule on a sample: the appended-point route over the device's own pair list
    got = crate.neighbor_tensors(k, queries=queries, squared_distances=True, partner_counts=True)
    sample = queries[:64]
    d = ((sample[:, None, :] - points[None, :, :]) ** 2)
    dist = d[..., 0] + d[..., 1]
    if not torch.equal((dist <= radius * radius).sum(dim=1), got[2][:64]):
        raise SystemExit("probes: the partner counts differ from the brute force")
    del d, dist
    times = alternate({"neighbor_tensors": lambda: crate.neighbor_tensors(k, queries=queries, squared_distances=True)},
                      reps, WARMUP)
    case = {**base, "k": k, "radius_in_diameters": 1.0, "probes": probes, "mean_partners": round(float(got[2].double().mean()), 3)}
    print(json.dumps({**case, "case": "probes: neighbor_tensors", **stats(times["neighbor_tensors"], "wall_")}), flush=True)
    dev = kernels(crate, radius, k, reps, 1, queries)
    dev = {key: v for key, v in dev.items() if not key.startswith("fill") and key not in ("list_bytes", "table_over_fill")}
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

    shapes = [(16, 1.0), (64, 1.0), (32, 2.0)]
    crate = viewer_crate(args.ticks)
    measure(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps, shapes, True)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    base = {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}
    big_reps = max(5, args.reps // 3)
    measure(crate, base, big_reps, shapes, False)
    measure_probes(crate, base, big_reps, args.probes)


if __name__ == "__main__":
    main()
