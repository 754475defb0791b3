"""Time of the batched clusters, cluster sums, histograms, rays and ray paths against the loop they replace, and of the
UNBATCHED kernels of the same four readers on one large cloud, where batching must cost nothing.

    timeout -k 10 600 python scripts/batch_readers_time.py [--clouds 64] [--reps 20] [--ticks 200] [--lib PATH]
    timeout -k 10 600 python scripts/batch_readers_time.py --unbatched [--big 1048576] [--reps 15] [--lib PATH]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above).

Without --unbatched, in the manner of scripts/batch_time.py: the frames are recorded from config/wave_machine.yaml, the
state after --ticks ticks and after every tick that follows, --clouds frames of about 1,250 particles that overlap
completely in space, concatenated with `pairs.batch_ptr` of their sizes.  Radius = the crate's diameter.  Per call

  cluster_tensors     `Crate.cluster_tensors_batch(radius)` against the loop of `Crate.cluster_tensors(radius)`
  cluster_sums        `Crate.cluster_sums_batch(values, radius, extrema=True)`, 2 channels, against `cluster_sums`
  distance_histogram  `Crate.distance_histogram_batch(edges, per_row=True)`, 16 bins up to the diameter, against
                      `distance_histogram`
  ray_tensors         `Crate.ray_tensors(..., batch=, ray_batch=)`: a fan of 64 rays per frame from the middle of the box,
                      the crate's walls, against the loop of unbatched calls
  ray_paths           `Crate.ray_paths(..., 3, batch=, ray_batch=)`: the same fans through three bounces

the wall time of the one batched call and of the loop over the frames -- the EXISTING unbatched call with `points=` of one
frame, not the new code --, the two alternating inside one loop after a warm-up; median and min over the repetitions and
the ratio of the medians.  Before anything is timed the batched results are compared with the loop's, concatenated and
shifted as tests/batch_readers_spec.py says: bit for bit.

With --unbatched: --big synthetic particles (bench.py's world and generator) after three ticks, the big state of
scripts/clusters_time.py, hist_time.py and rays_time.py, and the device time between HIP events, into tensors made once,
of `Engine.pairs_label` (k_cluster_union and the launches round it), `Engine.pairs_hist` (16 bins up to the diameter,
table and totals: k_hist), `Engine.pairs_rays` and `Engine.pairs_ray_paths` (3 bounces) for 256 x 256 rays on a lattice
looking along +y (k_rays, k_ray_paths), each after one `Engine.pairs_count`.  `--lib` times another build of the library
through the same script: run the parent commit's build and this one in turn and compare.  One JSON line per case,
microseconds.
"""
import argparse
import json

from timing_support import alternate, bench_crate, bits_equal, device_times, median, record, stats, use_library, viewer_crate

BINS, FAN, BOUNCES = 16, 64, 3
WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def joined(name, parts, ptr):
    """The loop's results as the batched call returns them (tests/batch_readers_spec.py)."""
    import torch
    starts = ptr[:-1].tolist()
    shift = lambda t, by: torch.where(t >= 0, t + by, t)                                         # noqa: E731
    if name in ("cluster_tensors", "cluster_sums"):
        before, labels, cptr = 0, [], [0]
        for part in parts:
            labels.append(shift(part[0], before))
            before += int(part[1].shape[0])
            cptr.append(before)
        roots = torch.cat([part[2] + s for part, s in zip(parts, starts)])
        tables = [torch.cat([part[k] for part in parts]) for k in range(3, len(parts[0]))]
        return (torch.cat(labels), torch.cat([part[1] for part in parts]), roots, *tables,
                torch.tensor(cptr, dtype=torch.int64, device=ptr.device))
    if name == "distance_histogram":
        return torch.cat([part[0] for part in parts]), torch.stack([part[1] for part in parts])
    out = [torch.cat([part[k] for part in parts]) for k in range(len(parts[0]))]
    out[1] = torch.cat([shift(part[1], s) for part, s in zip(parts, starts)])
    return tuple(out)


def batch_mode(args, pairs, torch):
    import numpy as np
    crate = viewer_crate(0)
    frames = record(crate, args.clouds, args.ticks)
    radius = crate.diameter
    walls = crate.segments
    points = torch.cat(frames)
    dev = points.device
    ptr = pairs.batch_ptr([int(f.shape[0]) for f in frames], dev)
    gen = torch.Generator(device=dev).manual_seed(13)
    values = torch.randn((int(points.shape[0]), 2), dtype=torch.float64, device=dev, generator=gen)
    cuts = ptr.tolist()
    frame_values = [values[a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
    edges = pairs.shell_edges(radius, BINS)
    fan = pairs.ray_fan((0.5, 0.5), FAN, 0.0, 2 * np.pi, device=dev)
    origins, directions = (t.repeat(args.clouds, 1).contiguous() for t in fan)
    ray_ptr = pairs.batch_ptr([FAN] * args.clouds, dev)
    ray_kw = dict(walls=walls)
    torch.cuda.synchronize()
    calls = {
        "cluster_tensors": (lambda: crate.cluster_tensors_batch(radius, points=points, batch=ptr),
                            lambda p, v: crate.cluster_tensors(radius, points=p)),
        "cluster_sums": (lambda: crate.cluster_sums_batch(values, radius, extrema=True, points=points, batch=ptr),
                         lambda p, v: crate.cluster_sums(v, radius, extrema=True, points=p)),
        "distance_histogram": (lambda: crate.distance_histogram_batch(edges, per_row=True, points=points, batch=ptr),
                               lambda p, v: crate.distance_histogram(edges, per_row=True, points=p)),
        "ray_tensors": (lambda: crate.ray_tensors(origins, directions, 2.0, points=points, batch=ptr, ray_batch=ray_ptr, **ray_kw),
                        lambda p, v: crate.ray_tensors(*fan, 2.0, points=p, **ray_kw)),
        "ray_paths": (lambda: tuple(crate.ray_paths(origins, directions, 2.0, BOUNCES, points=points, batch=ptr,
                                                    ray_batch=ray_ptr, **ray_kw)),
                      lambda p, v: tuple(crate.ray_paths(*fan, 2.0, BOUNCES, points=p, **ray_kw))),
    }
    base = {"clouds": args.clouds, "points": int(points.shape[0]), "points_per_cloud": round(points.shape[0] / args.clouds, 1),
            "radius_in_diameters": 1.0}
    for name, (batched, single) in calls.items():
        loop = lambda: [single(p, v) for p, v in zip(frames, frame_values)]                  # noqa: E731
        got, want = batched(), joined(name, loop(), ptr)
        if len(got) != len(want) or not all(bits_equal(g, w) for g, w in zip(got, want)):
            raise SystemExit(f"{name}: the batched call differs from the loop")
        times = alternate({"loop": loop, "batched": batched}, args.reps, WARMUP)
        med = {key: median(t) for key, t in times.items()}
        print(json.dumps({**base, "case": name, **stats(times["batched"], "batched_wall_"), **stats(times["loop"], "loop_wall_"),
                          "single_call_wall_us": round(med["loop"] / args.clouds, 2),
                          "batched_over_loop": round(med["batched"] / med["loop"], 4),
                          "batched_over_single": round(med["batched"] * args.clouds / med["loop"], 2)}), flush=True)


def unbatched_mode(args, pairs, torch):
    crate = bench_crate(args.big, 3)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    points = crate.state_tensors(pressure=False)[0].contiguous()
    n = int(points.shape[0])
    radius = crate.diameter
    walls = crate.segments
    side = 256
    k = (torch.arange(side, dtype=torch.float64, device=dev) + 0.5) / side
    origins = torch.stack([k.repeat(side), k.repeat_interleave(side)], dim=1).contiguous()
    down = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev).repeat(side * side, 1).contiguous()
    rays, legs = side * side, BOUNCES + 1
    i64 = lambda *shape: torch.empty(shape, dtype=torch.int64, device=dev)                    # noqa: E731
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)                  # noqa: E731
    offsets, counts, other = i64(n + 1), i64(2), i64(2)
    labels, sizes, roots = i64(n), i64(n), i64(n)
    table, total = torch.empty((n, BINS), dtype=torch.int32, device=dev), i64(BINS)
    t, hit = f64(rays), i64(rays)
    path = (f64(rays, legs), i64(rays, legs), f64(rays, legs, 2), f64(rays, legs, 2), i64(rays))
    edges = pairs.shell_edges(radius, BINS)
    ray_args = dict(origins=origins, directions=down, disc_radius=radius / 2, max_t=2.0, segments=walls, counts=other)
    torch.cuda.synchronize()
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts),
        "label": lambda: eng.pairs_label(labels, sizes, roots, counts=other),
        "hist": lambda: eng.pairs_hist(table, total, edges=edges, counts=other),
        "rays": lambda: eng.pairs_rays(t, hit, **ray_args),
        "ray_paths": lambda: eng.pairs_ray_paths(*path, bounces=BOUNCES, **ray_args)}, args.reps, WARMUP)
    if other.tolist() != [rays, 0]:
        raise SystemExit(f"the last reader reports {other.tolist()}")
    out = {"case": "unbatched kernels", "lib": args.lib or "this build", "points": n, "rays": rays, "bins": BINS,
           "bounces": BOUNCES, "clusters": int(labels.max()) + 1, "pairs_in_bins": int(total.sum()), "hits": int((hit >= 0).sum())}
    for name, series in times.items():
        out.update(stats(series, f"{name}_device_"))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--unbatched", action="store_true", help="time the unbatched kernels on one big cloud instead")
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    lib = use_library(args.lib)
    if lib:
        import ctypes
        from sand_crate_amd import _native
        other = ctypes.CDLL(str(lib))                                              # (an older build lacks the newest calls)
        for name in [name for name in _native.SIGNATURES if not hasattr(other, name)]:
            del _native.SIGNATURES[name]
    from sand_crate_amd import pairs
    if args.reps is None:
        args.reps = 15 if args.unbatched else 20
    (unbatched_mode if args.unbatched else batch_mode)(args, pairs, torch)


if __name__ == "__main__":
    main()
