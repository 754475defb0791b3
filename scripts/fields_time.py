"""Time of the device weighted sums against the route there was for the same sums: the CSR pair list, then torch.

    timeout -k 10 600 python scripts/fields_time.py [--reps 30] [--ticks 200] [--big 1048576] [--probes 65536]
                                                    [--raster 512] [--lib PATH]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above: a step that hangs then ends
the run too).  Two states, the ones scripts/nearest_time.py uses: config/wave_machine.yaml after --ticks ticks (the
viewer's size) and --big synthetic particles (bench.py's world and generator) after three ticks.  Per state and per
(channels, radius) -- 2 channels (the velocities) and 8 (random numbers) at radius = the crate's diameter and at twice the
diameter, power 3, include_self:

  field_tensors   `Crate.field_tensors(values, radius, weight_sums=True)`: wall time of the whole call -- the allocations,
                  count, sum, ONE synchronisation, the 16-byte read of (rows, status)
  list route      what there was before: `Crate.pair_tensors(radius, squared_distances=True)` and the torch code that turns
                  the list into the sums (`sums_from_list`: repeat_interleave, the weights, a gather of values[partners], a
                  multiply and two index_add_), ending in a synchronisation: wall time, and the pair_tensors part of it
  kernels         `Engine.pairs_count`, `Engine.pairs_sum` (sums and wsum) and `Engine.pairs_fill` (with d2) of the same grid
                  into tensors made once: device time between HIP events on the stream the library runs on -- the sum is
                  its memset and two launches (the check, the sum itself) --, and the bytes the
                  sums and the list take
  probes, raster  (big state) `Crate.field_tensors(velocities, queries=)` with --probes random probes inside the state's
                  bounding box and with the --raster x --raster `pairs.grid_queries` of that box: wall time of the call,
                  and the device time of the query-form sum alone

The sides of a comparison alternate inside one loop, the call in question last.  Before anything is timed the list
route's sums are compared with the kernel's -- to a relative 1e-9 of the row's sum of magnitudes: index_add_ adds with
floating-point atomics in no fixed order, so the list route has no bits to compare -- and on the small state the kernel's
with the NumPy rule (tests/field_spec.py), bit for bit.  `--lib` times another build of the library (a variant of a
kernel) through the same script.  The synthetic state's particles are numbered in the order of bench.py's uniform random
draws: an index says nothing about the place.  One JSON line per case: median and min over the repetitions, microseconds.
"""
import argparse
import json
import time

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, use_library, viewer_crate

WARMUP = 3                            # rounds before anything is recorded, wall and device alike

POWER = 3


def sums_from_list(offsets, partners, d2, values, radius):
    """(sums, wsum) of a full CSR pair list with distances, power 3 and every point its own partner."""
    import torch
    n = offsets.shape[0] - 1
    dev = offsets.device
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=dev), offsets[1:] - offsets[:-1])
    t = 1.0 - d2 / (radius * radius)
    w = t * t * t
    sums = values[:n].clone()                                           # (the point itself: d2 = 0, w = 1)
    sums.index_add_(0, rows, w.unsqueeze(1) * values[partners])
    wsum = torch.ones(n, dtype=torch.float64, device=dev)
    wsum.index_add_(0, rows, w)
    return sums, wsum


def kernels(crate, radius, values, reps, total, queries=None):
    """Device time of count, sum and fill by events, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    rows = eng.capacity if queries is None else int(queries.shape[0])
    width = int(values.shape[1])
    offsets = torch.empty(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts, other = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2))
    sums = torch.empty((rows, width), dtype=torch.float64, device=dev)
    wsum = torch.empty(rows, dtype=torch.float64, device=dev)
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts),
        "sum": lambda: eng.pairs_sum(values, sums, wsum, power=POWER, queries=queries, counts=other),
        "fill": lambda: eng.pairs_fill(partners, d2)}, reps, WARMUP)
    n_rows, status = (int(v) for v in other.cpu())
    if status != 0:
        raise SystemExit(f"kernels: status {status}")
    return {**stats(times["count"], "count_device_"), **stats(times["sum"], "sum_device_"), **stats(times["fill"], "fill_device_"),
            "rows": n_rows, "sums_bytes": 8 * n_rows * (width + 1), "list_bytes": 16 * total,
            "sum_over_fill": round(median(times["sum"]) / median(times["fill"]), 3)}


def close(got, want, scale):
    """|got - want| <= 1e-9 * scale, row by row (scale: the row's sum of magnitudes, at least 1e-300)."""
    return bool(((got - want).abs() <= 1e-9 * scale.clamp(min=1e-300)).all())


def measure(crate, base, reps, shapes, check_rule):
    import torch
    particles, velocities = crate.state_tensors(pressure=False)
    n = int(particles.shape[0])
    gen = torch.Generator(device=particles.device).manual_seed(13)
    wide = torch.randn((n, 8), dtype=torch.float64, device=particles.device, generator=gen)
    torch.cuda.synchronize()
    for width, factor in shapes:
        values = velocities if width == 2 else wide
        radius = factor * crate.diameter
        offsets, partners, d2 = crate.pair_tensors(radius, squared_distances=True)
        total = len(partners)
        want = sums_from_list(offsets, partners, d2, values, radius)
        got = crate.field_tensors(values, radius, power=POWER, weight_sums=True)
        scale = torch.ones(n, dtype=torch.float64, device=particles.device)
        rows = torch.repeat_interleave(torch.arange(n, device=particles.device), offsets[1:] - offsets[:-1])
        scale.index_add_(0, rows, values[partners].abs().amax(dim=1))
        scale += values.abs().amax(dim=1)
        if not (close(got[0], want[0], scale.unsqueeze(1)) and close(got[1], want[1], got[1])):
            raise SystemExit(f"C={width}: the kernel's sums differ from the list route's")
        if check_rule:
            import field_spec
            rule = field_spec.field(particles.cpu().numpy(), radius, values.cpu().numpy(), POWER, True)
            if any(g.cpu().numpy().tobytes() != w.tobytes() for g, w in zip(got, rule)):
                raise SystemExit(f"C={width}: field_tensors differs from the rule")
        del want, got, rows, scale
        case = {**base, "channels": width, "radius_in_diameters": factor, "E": total, "E_per_n": round(total / max(n, 1), 3)}
        part = []

        def list_route():
            t0 = time.perf_counter()
            o, p, d = crate.pair_tensors(radius, squared_distances=True)
            part.append(1e6 * (time.perf_counter() - t0))
            sums_from_list(o, p, d, values, radius)
            torch.cuda.synchronize()

        times = alternate({"list route": list_route,
                           "field_tensors": lambda: crate.field_tensors(values, radius, power=POWER, weight_sums=True)},
                          reps, WARMUP)
        print(json.dumps({**case, "case": "list route", **stats(times["list route"], "wall_"),
                          **stats(part[-reps:], "pair_tensors_part_wall_")}), flush=True)
        print(json.dumps({**case, "case": "field_tensors", **stats(times["field_tensors"], "wall_")}), flush=True)
        print(json.dumps({**case, "case": "kernels", **kernels(crate, radius, values, reps, total)}), flush=True)
        med = {name: median(t) for name, t in times.items()}
        print(json.dumps({**case, "case": "verdict",
                          "field_tensors_over_list_route": round(med["field_tensors"] / med["list route"], 4)}), flush=True)
        del offsets, partners, d2
        torch.cuda.empty_cache()


def measure_queries(crate, base, reps, name, queries):
    import torch
    radius = crate.diameter
    points, velocities = crate.state_tensors(pressure=False)
    # the rule on a sample: brute force over all points
    got = crate.field_tensors(velocities, queries=queries, power=POWER, weight_sums=True)
    sample = queries[:64]
    d = ((sample[:, None, :] - points[None, :, :]) ** 2)
    dist = d[..., 0] + d[..., 1]
    t = 1.0 - dist / (radius * radius)
    w = torch.where(dist <= radius * radius, t * t * t, torch.zeros_like(t))
    if not (close(got[1][:64], w.sum(dim=1), got[1][:64]) and
            close(got[0][:64], w @ velocities, (w @ velocities.abs()).amax(dim=1, keepdim=True))):
        raise SystemExit(f"{name}: the sums differ from the brute force")
    del d, dist, t, w
    times = alternate({"field_tensors": lambda: crate.field_tensors(velocities, queries=queries, power=POWER,
                                                                    weight_sums=True)}, reps, WARMUP)
    case = {**base, "channels": 2, "radius_in_diameters": 1.0, "queries": int(queries.shape[0]),
            "rows_with_partners": int((got[1] > 0).sum())}
    print(json.dumps({**case, "case": f"{name}: field_tensors", **stats(times["field_tensors"], "wall_")}), flush=True)
    dev = kernels(crate, radius, velocities, reps, 1, queries)
    dev = {key: v for key, v in dev.items() if not key.startswith("fill") and key not in ("list_bytes", "sum_over_fill")}
    print(json.dumps({**case, "case": f"{name}: kernels", **dev}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--probes", type=int, default=65536)
    ap.add_argument("--raster", type=int, default=512)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    use_library(args.lib)
    from sand_crate_amd import pairs

    shapes = [(2, 1.0), (8, 1.0), (2, 2.0), (8, 2.0)]
    crate = viewer_crate(args.ticks)
    measure(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps, shapes, True)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    base = {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}
    big_reps = max(5, args.reps // 3)
    measure(crate, base, big_reps, shapes, False)
    points = crate.state_tensors()[0]
    lo, hi = points.min(dim=0).values, points.max(dim=0).values
    gen = torch.Generator(device=points.device).manual_seed(11)
    probes = lo + (hi - lo) * torch.rand((args.probes, 2), dtype=torch.float64, device=points.device, generator=gen)
    raster = pairs.grid_queries(float(lo[0]), float(hi[0]), float(lo[1]), float(hi[1]), args.raster, args.raster, points.device)
    torch.cuda.synchronize()
    measure_queries(crate, base, big_reps, "probes", probes)
    measure_queries(crate, base, big_reps, "raster", raster)


if __name__ == "__main__":
    main()
