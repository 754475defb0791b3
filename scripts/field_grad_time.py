"""Time of forward + backward of `Crate.field_function` against the route there was for a gradient of the same sums: the CSR
pair list, then torch under autograd.

    timeout -k 10 900 python scripts/field_grad_time.py [--reps 20] [--ticks 200] [--big 1048576] [--probes 65536]
                                                        [--raster 512]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above: a step that hangs then ends
the run too).  Two states, the ones scripts/fields_time.py uses: config/wave_machine.yaml after --ticks ticks (the
viewer's size) and --big synthetic particles (bench.py's world and generator) after three ticks.  The positions are taken
once with `state_tensors()` and given to both routes as `points=`.  Per state and per (channels, radius) -- 2 channels (the
velocities) and 8 (random numbers) at radius = the crate's diameter and at twice the diameter, power 3, include_self, both
outputs used (upstream G and gw are random numbers) -- and per set of gradients, "values" and "values+points":

  field_function  `Crate.field_function(values, radius, points=, weight_sums=True)` and `torch.autograd.grad` of both
                  outputs: wall time of forward + backward, ending in a synchronisation
  list route      `Crate.pair_tensors(radius, points=, squared_distances=True)`, then torch float64 under autograd:
                  repeat_interleave, the weights, a gather of values[partners], a multiply and two index_add, and
                  `torch.autograd.grad` of the same outputs, ending in a synchronisation.  For "values" the weights come
                  from the list's d2; for "values+points" d2 is recomputed in torch from points[rows] - points[partners],
                  or nothing would reach the points
  kernels         `Engine.pairs_count`, `Engine.pairs_sum` (sums and wsum), `Engine.pairs_sum_grad` (as many channels as
                  the sum has, both scalars, the self form) and `Engine.pairs_fill` (with d2) of the same grid into
                  tensors made once: device time between HIP events on the stream the library runs on; each of the two
                  in the middle is a memset and two launches (the check and the kernel itself)
  probes, raster  (big state) `Crate.field_function(velocities, points=, queries=, weight_sums=True)` with --probes random
                  probes inside the state's bounding box and with the --raster x --raster `pairs.grid_queries` of that
                  box, gradients with respect to the values and the queries: wall time of forward + backward next to the
                  forward alone, and the device time of the query-form gradient kernel next to the query-form sum.  The
                  pair list has no query form: there is no list route to compare with

The sides of a comparison alternate inside one loop, the call in question last.  Before anything is timed the two routes'
gradients are compared -- to 1e-9 of the largest magnitude: index_add adds with floating-point atomics in no fixed order,
so the list route has no bits to compare -- and on the small state `field_function`'s with the NumPy rule
(tests/field_grad_spec.py), bit for bit.  One JSON line per case: median and min over the repetitions, microseconds.
"""
import argparse
import json
import time

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, use_library, viewer_crate

WARMUP = 2                            # rounds before anything is recorded, wall and device alike

POWER = 3


def field_route(crate, values, points, radius, G, gw, with_points, queries=None):
    """forward + backward through field_function -> the gradients, synchronised."""
    import torch
    v = values.detach().requires_grad_()
    p = points.detach().requires_grad_() if with_points and queries is None else points
    q = None if queries is None else queries.detach().requires_grad_()
    out = crate.field_function(v, radius, power=POWER, points=p, queries=q, weight_sums=True)
    wanted = [v] + ([p] if with_points and queries is None else []) + ([q] if q is not None else [])
    grads = torch.autograd.grad(list(out), wanted, [G, gw])
    torch.cuda.synchronize()
    return grads


def list_route(crate, values, points, radius, G, gw, with_points, part=None):
    """forward + backward through the pair list and torch's autograd -> the gradients, synchronised."""
    import torch
    t0 = time.perf_counter()
    offsets, partners, d2 = crate.pair_tensors(radius, points=points, squared_distances=True)
    if part is not None:
        part.append(1e6 * (time.perf_counter() - t0))
    n = offsets.shape[0] - 1
    v = values.detach().requires_grad_()
    rows = torch.repeat_interleave(torch.arange(n, dtype=torch.int64, device=offsets.device), offsets[1:] - offsets[:-1])
    wanted = [v]
    if with_points:
        p = points.detach().requires_grad_()
        wanted.append(p)
        diff = p[rows] - p[partners]
        d2 = (diff * diff).sum(dim=1)
    t = 1.0 - d2 / (radius * radius)
    w = t * t * t
    sums = v.index_add(0, rows, w.unsqueeze(1) * v[partners])            # (from v: the point itself, d2 = 0, w = 1)
    wsum = torch.ones(n, dtype=torch.float64, device=offsets.device).index_add(0, rows, w)
    outputs = [(o, g) for o, g in ((sums, G), (wsum, gw)) if o.requires_grad]   # (for "values" wsum is a constant)
    grads = torch.autograd.grad([o for o, _ in outputs], wanted, [g for _, g in outputs])
    torch.cuda.synchronize()
    return grads


def kernels(crate, points, radius, values, G, gw, reps, total, queries=None):
    """Device time of count, sum, gradient and fill by events, into tensors made once."""
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = int(points.shape[0])
    rows = n if queries is None else int(queries.shape[0])
    width = int(values.shape[1])
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    counts, other, third = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(3))
    sums = torch.empty((rows, width), dtype=torch.float64, device=dev)
    wsum = torch.empty(rows, dtype=torch.float64, device=dev)
    grad = torch.empty((rows, 2), dtype=torch.float64, device=dev)
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    spans = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts),
        "sum": lambda: eng.pairs_sum(values, sums, wsum, power=POWER, queries=queries, counts=other),
        "grad": lambda: eng.pairs_sum_grad(grad, G, values, gw, gw if queries is None else None, power=POWER, queries=queries,
                                           counts=third),
        "fill": lambda: eng.pairs_fill(partners, d2)}, reps, WARMUP)
    for name, c in (("sum", other), ("grad", third)):
        if int(c[1]) != 0:
            raise SystemExit(f"kernels: {name} status {int(c[1])}")
    return {**stats(spans["count"], "count_device_"), **stats(spans["sum"], "sum_device_"), **stats(spans["grad"], "grad_device_"),
            **stats(spans["fill"], "fill_device_"), "rows": int(third[0]), "grad_bytes": 16 * rows, "list_bytes": 16 * total,
            "grad_over_sum": round(median(spans["grad"]) / median(spans["sum"]), 3),
            "grad_over_fill": round(median(spans["grad"]) / median(spans["fill"]), 3)}


def agree(got, want, what):
    for g, w in zip(got, want):
        if not bool(((g - w).abs().max() <= 1e-9 * w.abs().max().clamp(min=1e-300)) if g.numel() else True):
            raise SystemExit(f"{what}: the two routes' gradients differ")


def measure(crate, base, reps, shapes, check_rule):
    import torch
    particles, velocities = crate.state_tensors(pressure=False)
    n = int(particles.shape[0])
    dev = particles.device
    gen = torch.Generator(device=dev).manual_seed(13)
    wide = torch.randn((n, 8), dtype=torch.float64, device=dev, generator=gen)
    upstream = torch.randn((n, 9), dtype=torch.float64, device=dev, generator=gen)
    torch.cuda.synchronize()
    for width, factor in shapes:
        values = velocities if width == 2 else wide
        G, gw = upstream[:, :width].contiguous(), upstream[:, 8].contiguous()
        radius = factor * crate.diameter
        total = len(crate.pair_tensors(radius, points=particles)[1])
        case = {**base, "channels": width, "radius_in_diameters": factor, "E": total, "E_per_n": round(total / max(n, 1), 3)}
        for with_points in (False, True):
            wrt = "values+points" if with_points else "values"
            got = field_route(crate, values, particles, radius, G, gw, with_points)
            agree(got, list_route(crate, values, particles, radius, G, gw, with_points), f"C={width} {wrt}")
            if check_rule:
                import field_grad_spec as GS
                P, V, Gn, gwn = (t.cpu().numpy() for t in (particles, values, G, gw))
                rule = [GS.values_grad(P, radius, Gn, POWER, True)] + ([GS.self_points_grad(P, radius, V, POWER, Gn, gwn)] if with_points else [])
                if any(g.cpu().numpy().tobytes() != w.tobytes() for g, w in zip(got, rule)):
                    raise SystemExit(f"C={width} {wrt}: field_function differs from the rule")
            del got
            part = []
            times = alternate({"list route": lambda: list_route(crate, values, particles, radius, G, gw, with_points, part),
                               "field_function": lambda: field_route(crate, values, particles, radius, G, gw, with_points)},
                              reps, WARMUP)
            print(json.dumps({**case, "wrt": wrt, "case": "list route", **stats(times["list route"], "wall_"),
                              **stats(part[-reps:], "pair_tensors_part_wall_")}), flush=True)
            print(json.dumps({**case, "wrt": wrt, "case": "field_function", **stats(times["field_function"], "wall_")}), flush=True)
            med = {name: median(t) for name, t in times.items()}
            print(json.dumps({**case, "wrt": wrt, "case": "verdict",
                              "field_function_over_list_route": round(med["field_function"] / med["list route"], 4)}), flush=True)
            torch.cuda.empty_cache()
        print(json.dumps({**case, "case": "kernels", **kernels(crate, particles, radius, values, G, gw, reps, total)}), flush=True)
        torch.cuda.empty_cache()


def measure_queries(crate, base, reps, name, queries):
    import torch
    radius = crate.diameter
    points, velocities = crate.state_tensors(pressure=False)
    q = int(queries.shape[0])
    gen = torch.Generator(device=points.device).manual_seed(17)
    upstream = torch.randn((q, 3), dtype=torch.float64, device=points.device, generator=gen)
    G, gw = upstream[:, :2].contiguous(), upstream[:, 2].contiguous()
    torch.cuda.synchronize()
    # the gradient with respect to the queries against torch's autograd of the brute force, on a sample
    got = field_route(crate, velocities, points, radius, G, gw, False, queries)
    sample = queries[:64].detach().requires_grad_()
    diff = sample[:, None, :] - points[None, :, :]
    dist = (diff * diff).sum(dim=2)
    t = 1.0 - dist / (radius * radius)
    w = torch.where(dist.detach() <= radius * radius, t * t * t, torch.zeros_like(t))
    want, = torch.autograd.grad([w @ velocities, w.sum(dim=1)], [sample], [G[:64], gw[:64]])
    agree([got[1][:64]], [want], name)
    del diff, dist, t, w, want, got
    times = alternate({"field_tensors": lambda: (crate.field_tensors(velocities, radius, power=POWER, points=points, queries=queries,
                                                                     weight_sums=True), torch.cuda.synchronize()),
                       "field_function": lambda: field_route(crate, velocities, points, radius, G, gw, False, queries)},
                      reps, WARMUP)
    case = {**base, "channels": 2, "radius_in_diameters": 1.0, "queries": q, "wrt": "values+queries"}
    print(json.dumps({**case, "case": f"{name}: forward alone (field_tensors)", **stats(times["field_tensors"], "wall_")}), flush=True)
    print(json.dumps({**case, "case": f"{name}: field_function", **stats(times["field_function"], "wall_")}), flush=True)
    dev = kernels(crate, points, radius, velocities, G, gw, reps, 1, queries)
    dev = {key: v for key, v in dev.items() if not key.startswith("fill") and key not in ("list_bytes", "grad_over_fill")}
    print(json.dumps({**case, "case": f"{name}: kernels", **dev}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=20)
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
    big_reps = max(5, args.reps // 4)
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
