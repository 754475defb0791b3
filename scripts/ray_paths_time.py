"""Time of the device ray paths against the ray sensors and against the route there was: one `ray_tensors` per leg.

    timeout -k 10 900 python scripts/ray_paths_time.py [--reps 10] [--ticks 200] [--big 1048576] [--lib PATH] [--rays-only]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above).  The worlds and the rays
are scripts/rays_time.py's: the state of config/wave_machine.yaml after --ticks ticks (the viewer's size) with a fan of
256 rays; --big synthetic particles after three ticks and every 256th of them as `points=`, each with the fan and with
512 x 512 rays on a lattice, looking along +y.  max_t is 2 per leg: `ray_paths` gets 2 (bounces + 1) for the path.

  bounces 0     `Crate.ray_paths(bounces=0)` against `Crate.ray_tensors` on the same rays: wall time of the whole call,
                and device time between HIP events of `Engine.pairs_ray_paths` against `Engine.pairs_rays` alone, into
                tensors made once -- what a leg's hit point, normal and end cost
  bounces 1 3 7 `Crate.ray_paths` against the loop: `ray_tensors` once per leg and, in between, torch's gather of the
                centres, the normal, the reflection and an origin nudged off the surface by EPSILON along the normal.
                The loop's results are NOT the same bits -- they depend on the epsilon, its budget is per leg, and a ray
                that leaves a disc it started in hits it again --: it is timed as the floor of what a caller could do
                without the kernel, and it pays one count per leg
  --rays-only   device time of `Engine.pairs_rays` alone on the synthetic world, fan and lattice: with --lib, another
                build of the library through the same script -- the ray sensors' kernel before and after the paths

The sides of a comparison alternate inside one loop, after 2 warm-up rounds.  One JSON line per case: median, min and
max over the repetitions, microseconds."""
import argparse
import json
from functools import partial

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, use_library, viewer_crate
import timing_support

EPSILON = 1e-9                        # of a particle diameter: the loop's nudge off the surface it has just hit
WARMUP = 2                            # rounds before anything is recorded, wall and device alike
stats = partial(timing_support.stats, maximum=True)                                  # (this script reports the max as well)


def kernels(crate, points, origins, directions, max_t, walls, bounces, reps, paths=True):
    """Device time of `pairs_rays` and `pairs_ray_paths` after one count, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    rho = crate.diameter / 2
    bound = eng.capacity if points is None else int(points.shape[0])
    rays, legs = int(origins.shape[0]), bounces + 1
    offsets = torch.empty(bound + 1, dtype=torch.int64, device=dev)
    counts, out = torch.empty(2, dtype=torch.int64, device=dev), torch.empty(2, dtype=torch.int64, device=dev)
    t, hit = torch.empty(rays, dtype=torch.float64, device=dev), torch.empty(rays, dtype=torch.int64, device=dev)
    eng.pairs_count(points, radius=2 * rho, offsets=offsets, counts=counts)
    kw = dict(origins=origins, directions=directions, disc_radius=rho, segments=walls, counts=out)
    calls = {"rays": lambda: eng.pairs_rays(t, hit, max_t=max_t, **kw)}
    if paths:
        held = (torch.empty((rays, legs), dtype=torch.float64, device=dev), torch.empty((rays, legs), dtype=torch.int64, device=dev),
                torch.empty((rays, legs, 2), dtype=torch.float64, device=dev), torch.empty((rays, legs, 2), dtype=torch.float64, device=dev),
                torch.empty(rays, dtype=torch.int64, device=dev))
        calls["paths"] = lambda: eng.pairs_ray_paths(*held, bounces=bounces, max_t=max_t * legs, **kw)
    times = device_times(eng, calls, reps, WARMUP)
    if int(out[1]) != 0:
        raise SystemExit(f"kernels: status {int(out[1])}")
    return times


def loop_route(crate, cloud, points, origins, directions, max_t, walls, bounces):
    """One `ray_tensors` per leg; between them the hit point, the normal and the reflection in torch, and the nudge."""
    import torch
    w = torch.as_tensor(walls, dtype=torch.float64, device=origins.device).reshape(-1, 2, 2)
    e = w[:, 1] - w[:, 0]
    wall_n = torch.stack([e[:, 1], -e[:, 0]], dim=1) / torch.linalg.norm(e, dim=1, keepdim=True)
    o, d = origins, directions
    eps = EPSILON * crate.diameter
    for leg in range(bounces + 1):
        t, hit = crate.ray_tensors(o, d, max_t, walls=walls, points=points)
        if leg == bounces:
            break
        at = o + t.unsqueeze(1) * d
        n = torch.where((hit >= 0).unsqueeze(1), at - cloud[hit.clamp(min=0)], wall_n[(-2 - hit).clamp(min=0)])
        n = n / torch.linalg.norm(n, dim=1, keepdim=True)
        n = torch.where(((d * n).sum(dim=1) > 0).unsqueeze(1) & (hit <= -2).unsqueeze(1), -n, n)
        dn = (d * n).sum(dim=1, keepdim=True)
        d = torch.where(dn < 0, d - 2 * dn * n, d).contiguous()
        o = (at + eps * n).contiguous()                                             # (a ray that met nothing is dead from here on)
    return t, hit


def measure(crate, base, points, origins, directions, max_t, walls, reps):
    import torch
    rays = int(origins.shape[0])
    case = {**base, "rays": rays, "points": crate.particle_count if points is None else int(points.shape[0])}
    cloud = crate.state_tensors(pressure=False)[0] if points is None else points
    # bounces = 0 against ray_tensors: the same t and hit, then the two calls and the two kernels in turn
    t, hit = crate.ray_tensors(origins, directions, max_t, walls=walls, points=points)
    flat = crate.ray_paths(origins, directions, max_t, 0, walls=walls, points=points)
    if not (torch.equal(flat.hit[:, 0], hit) and torch.equal(flat.t[:, 0], t)):
        raise SystemExit(f"{case}: ray_paths(bounces=0) differs from ray_tensors")
    wall = alternate({"ray_tensors": lambda: crate.ray_tensors(origins, directions, max_t, walls=walls, points=points),
                      "ray_paths": lambda: crate.ray_paths(origins, directions, max_t, 0, walls=walls, points=points)},
                     reps, WARMUP)
    dev = kernels(crate, points, origins, directions, max_t, walls, 0, reps)
    print(json.dumps({**case, "case": "bounces 0", **stats(wall["ray_tensors"], "ray_tensors_wall_"), **stats(wall["ray_paths"], "ray_paths_wall_"),
                      **stats(dev["rays"], "rays_device_"), **stats(dev["paths"], "paths_device_"),
                      "paths_over_rays_wall": round(median(wall["ray_paths"]) / median(wall["ray_tensors"]), 3),
                      "paths_over_rays_device": round(median(dev["paths"]) / median(dev["rays"]), 3)}), flush=True)
    for bounces in (1, 3, 7):
        got = crate.ray_paths(origins, directions, max_t * (bounces + 1), bounces, walls=walls, points=points)
        wall = alternate({"loop": lambda: loop_route(crate, cloud, points, origins, directions, max_t, walls, bounces),
                          "ray_paths": lambda: crate.ray_paths(origins, directions, max_t * (bounces + 1), bounces, walls=walls,
                                                               points=points)}, reps, WARMUP)
        dev = kernels(crate, points, origins, directions, max_t, walls, bounces, reps)
        print(json.dumps({**case, "case": f"bounces {bounces}", "legs_that_hit": int((got.hit != -1).sum()),
                          "ends": {str(k): int((got.end == k).sum()) for k in (0, 1, 2, -1, -4)},
                          **stats(wall["loop"], "loop_wall_"), **stats(wall["ray_paths"], "ray_paths_wall_"),
                          **stats(dev["paths"], "paths_device_"),
                          "paths_over_loop_wall": round(median(wall["ray_paths"]) / median(wall["loop"]), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time (with --rays-only)")
    ap.add_argument("--rays-only", action="store_true", help="only Engine.pairs_rays on the synthetic world")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    if use_library(args.lib) and args.rays_only:                                    # (a build from before the paths has no such export)
        from sand_crate_amd import _native
        _native.SIGNATURES.pop("sc_pairs_ray_paths_device", None)
    from sand_crate_amd import pairs

    dev = torch.device("cuda", 0)
    fan = pairs.ray_fan((0.5, 0.5), 256, 0.0, 2 * np.pi, device=dev)
    if not args.rays_only:
        crate = viewer_crate(args.ticks)
        torch.cuda.synchronize()
        measure(crate, {"state": "wave_machine", "ticks": args.ticks}, None, *fan, 2.0, crate.segments, args.reps)
        crate.engine.close()

    crate = bench_crate(args.big, 3)
    walls = crate.segments
    side = 512
    k = (torch.arange(side, dtype=torch.float64, device=dev) + 0.5) / side
    lattice = torch.stack([k.repeat(side), k.repeat_interleave(side)], dim=1).contiguous()
    down = torch.tensor([0.0, 1.0], dtype=torch.float64, device=dev).repeat(side * side, 1).contiguous()
    sparse = crate.state_tensors(pressure=False)[0][::256].contiguous()
    torch.cuda.synchronize()
    if args.rays_only:
        for name, (o, d) in (("fan", fan), ("lattice", (lattice, down))):
            for points, world in ((None, "synthetic"), (sparse, "synthetic, every 256th")):
                times = kernels(crate, points, o, d, 2.0, walls, 0, args.reps, paths=False)
                print(json.dumps({"case": "pairs_rays alone", "lib": args.lib or "this build", "state": world, "set": name,
                                  "rays": int(o.shape[0]), **stats(times["rays"], "rays_device_")}), flush=True)
        return
    for name, points in (("synthetic", None), ("synthetic, every 256th", sparse)):
        base = {"state": name, "ticks": 3}
        measure(crate, base, points, *fan, 2.0, walls, args.reps)
        measure(crate, base, points, lattice, down, 2.0, walls, args.reps)


if __name__ == "__main__":
    main()
