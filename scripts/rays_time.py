"""Time of the device ray sensors against torch's broadcast route for the same answer.

    timeout -k 10 900 python scripts/rays_time.py [--reps 20] [--ticks 200] [--big 1048576] [--lib PATH]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above).  Three worlds: the state of
config/wave_machine.yaml after --ticks ticks (the viewer's size) with its own walls; --big synthetic particles (bench.py's
world and generator) after three ticks, with the scene's walls -- uniformly dense: a ray meets a disc within a cell or
two --; and every 256th of those particles as `points=`, where a ray walks some seventy cells before it meets one.  The
rays: a fan of 256 from the middle of the box, and -- the big worlds -- 512 x 512 origins on a lattice over the box, all
looking along +y, the way gravity points.  Per world and set of rays:

  ray_tensors   `Crate.ray_tensors(origins, directions, max_t[, points=])`: wall time of the whole call -- the
                allocations, count, rays, ONE synchronisation, the 32-byte read of the counts
  kernels       `Engine.pairs_count` and `Engine.pairs_rays` into tensors made once: device time between HIP events on
                the stream the library runs on.  The count is the whole of sc_pairs_count_device; the rays are a memset,
                the check's two launches and the walk
  torch         the broadcast route: rays x points, the rule's arithmetic in torch operations (each rounded on its own),
                min and argmin over the points, then the walls; in chunks of 256 rays, which is 2.1 GB per temporary over
                1,048,576 points.  Wall time ending in a synchronise.  For 262,144 rays FOUR chunks are timed and the
                figure is that time times 256: it says so ("extrapolated")
  sweep         (big worlds) device time of `Engine.pairs_rays` alone for 256 .. 262,144 rays of the lattice

The sides of a comparison alternate inside one loop.  Before anything is timed the kernel's results are compared with
torch's on the chunks it computes (they must be equal, bit for bit -- reported, not assumed), and on the viewer's state
with the NumPy rule (tests/ray_spec.py).  `--lib` times another build of the library through the same script.  One
JSON line per case: median and min over the repetitions, microseconds.
"""
import argparse
import json

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, use_library, viewer_crate

CHUNK = 256
WARMUP = 2                            # rounds before anything is recorded, wall and device alike


def torch_route(points, walls, origins, directions, rho, max_t):
    """(t, hit) of tests/ray_spec.py in torch, for one chunk of live rays: rays x points, then the walls."""
    import torch
    inf = float("inf")
    ox, oy, dx, dy = origins[:, 0:1], origins[:, 1:2], directions[:, 0:1], directions[:, 1:2]
    fx, fy = ox - points[None, :, 0], oy - points[None, :, 1]
    a = dx * dx + dy * dy
    b = fx * dx + fy * dy
    cc = (fx * fx + fy * fy) - rho * rho
    disc = b * b - a * cc
    t = cc / (torch.sqrt(disc) - b)
    t = torch.where(cc <= 0, torch.zeros_like(t), torch.where((b < 0) & (disc >= 0), t, torch.full_like(t, inf)))
    t = torch.where(t <= max_t, t, torch.full_like(t, inf))
    best, who = t.min(dim=1)
    hit = torch.where(best < inf, who, torch.full_like(who, -1))
    if len(walls):
        w = torch.as_tensor(walls, dtype=torch.float64, device=points.device)
        ax, ay = w[None, :, 0, 0], w[None, :, 0, 1]
        ex, ey = w[None, :, 1, 0] - ax, w[None, :, 1, 1] - ay
        gx, gy = ax - ox, ay - oy
        den = dx * ey - dy * ex
        tw = (gx * ey - gy * ex) / den
        uw = (gx * dy - gy * dx) / den
        ok = (den != 0) & (tw >= 0) & (tw <= max_t) & (uw >= 0) & (uw <= 1)
        tw = torch.where(ok, tw + 0.0, torch.full_like(tw, inf))
        wall_t, wall_s = tw.min(dim=1)
        wins = wall_t <= best                                                       # (a wall wins a tie)
        wins &= wall_t < inf
        best = torch.where(wins, wall_t, best)
        hit = torch.where(wins, -2 - wall_s, hit)
    return best, hit


def kernels(crate, points, origins, directions, rho, max_t, walls, reps):
    """Device time of the count and of the rays by events, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    bound = eng.capacity if points is None else int(points.shape[0])
    rays = int(origins.shape[0])
    offsets = torch.empty(bound + 1, dtype=torch.int64, device=dev)
    counts, out = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    t, hit = torch.empty(rays, dtype=torch.float64, device=dev), torch.empty(rays, dtype=torch.int64, device=dev)
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=2 * rho, offsets=offsets, counts=counts),
        "rays": lambda: eng.pairs_rays(t, hit, origins=origins, directions=directions, disc_radius=rho, max_t=max_t, segments=walls,
                                       counts=out)}, reps, WARMUP)
    if int(out[1]) != 0:
        raise SystemExit(f"kernels: status {int(out[1])}")
    return {**stats(times["count"], "count_device_"), **stats(times["rays"], "rays_device_"),
            "rays_over_count": round(median(times["rays"]) / median(times["count"]), 3)}


def measure(crate, base, points, origins, directions, max_t, walls, reps, check_rule=False):
    import torch
    rho = crate.diameter / 2
    rays = int(origins.shape[0])
    case = {**base, "rays": rays, "points": crate.particle_count if points is None else int(points.shape[0])}
    t, hit = crate.ray_tensors(origins, directions, max_t, walls=walls, points=points)
    cloud = crate.state_tensors(pressure=False)[0] if points is None else points
    if check_rule:
        import ray_spec
        want = ray_spec.rays(cloud.cpu().numpy(), walls, origins.cpu().numpy(), directions.cpu().numpy(), rho, max_t)
        if not (np.array_equal(t.cpu().numpy(), want[0]) and np.array_equal(hit.cpu().numpy(), want[1])):
            raise SystemExit(f"{case}: ray_tensors differs from the rule")
    chunks = min(4, (rays + CHUNK - 1) // CHUNK)
    equal = True
    for k in range(chunks):
        rows = slice(k * CHUNK, (k + 1) * CHUNK)
        got = torch_route(cloud, walls, origins[rows], directions[rows], rho, max_t)
        equal &= bool(torch.equal(got[1], hit[rows])) and bool(torch.equal(got[0], t[rows]))
    del got

    def by_torch():
        for k in range(chunks):
            rows = slice(k * CHUNK, (k + 1) * CHUNK)
            torch_route(cloud, walls, origins[rows], directions[rows], rho, max_t)
        torch.cuda.synchronize()

    times = alternate({"torch": by_torch,
                       "ray_tensors": lambda: crate.ray_tensors(origins, directions, max_t, walls=walls, points=points)},
                      reps, WARMUP)
    scale = ((rays + CHUNK - 1) // CHUNK) / chunks
    print(json.dumps({**case, "case": "torch broadcast", "chunks_timed": chunks, "extrapolated": scale != 1.0,
                      "equal_to_the_kernel": equal, **stats([v * scale for v in times["torch"]], "wall_")}), flush=True)
    med = {name: median(series) for name, series in times.items()}
    print(json.dumps({**case, "case": "ray_tensors", **stats(times["ray_tensors"], "wall_"),
                      "ray_tensors_over_torch": round(med["ray_tensors"] / (med["torch"] * scale), 5)}), flush=True)
    print(json.dumps({**case, "case": "kernels", "hits_on_particles": int((hit >= 0).sum()), "hits_on_walls": int((hit <= -2).sum()),
                      "mean_t_in_cells": round(float(t[torch.isfinite(t)].mean()) / crate.diameter, 2),
                      **kernels(crate, points, origins, directions, rho, max_t, walls, reps)}), flush=True)


def sweep(crate, base, points, origins, directions, max_t, walls, reps):
    rho = crate.diameter / 2
    for rays in (256, 1024, 4096, 16384, 65536, 262144):
        step = max(1, int(origins.shape[0]) // rays)
        o, d = origins[::step][:rays].contiguous(), directions[::step][:rays].contiguous()
        got = kernels(crate, points, o, d, rho, max_t, walls, reps)
        print(json.dumps({**base, "case": "sweep", "rays": int(o.shape[0]),
                          **{k: v for k, v in got.items() if not k.startswith("count")}}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    use_library(args.lib)
    from sand_crate_amd import pairs

    crate = viewer_crate(args.ticks)
    dev = torch.device("cuda", crate.engine.device)
    fan = pairs.ray_fan((0.5, 0.5), 256, 0.0, 2 * np.pi, device=dev)
    torch.cuda.synchronize()
    measure(crate, {"state": "wave_machine", "ticks": args.ticks}, None, *fan, 2.0, crate.segments, args.reps, check_rule=True)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    walls = crate.segments
    side = 512
    k = (torch.arange(side, dtype=torch.float64, device=dev) + 0.5) / side
    lattice = torch.stack([k.repeat(side), k.repeat_interleave(side)], dim=1).contiguous()
    down = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev).repeat(side * side, 1).contiguous()
    sparse = crate.state_tensors(pressure=False)[0][::256].contiguous()
    torch.cuda.synchronize()
    big_reps = max(5, args.reps // 2)
    for name, points in (("synthetic", None), ("synthetic, every 256th", sparse)):
        base = {"state": name, "ticks": 3}
        measure(crate, base, points, *fan, 2.0, walls, big_reps)
        measure(crate, base, points, lattice, down, 2.0, walls, big_reps)
        sweep(crate, base, points, lattice, down, 2.0, walls, big_reps)


if __name__ == "__main__":
    main()
