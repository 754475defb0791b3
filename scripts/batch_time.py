"""Time of the batched neighbourhood calls against the loop they replace: B frames of the viewer's size in ONE call with
`batch=`, against a Python loop of B single calls on the same build.

    timeout -k 10 600 python scripts/batch_time.py [--clouds 64] [--reps 20] [--ticks 200] [--lib PATH]

One process, every step in turn, the first failure ends it (run it under `timeout`, as above).  The frames are recorded
from config/wave_machine.yaml: the state after --ticks ticks and after every tick that follows, --clouds frames of about
1,248 particles that overlap completely in space, concatenated into one (n, 2) tensor with `pairs.batch_ptr` of their
sizes.  Radius = the crate's diameter.  Per function

  pair_tensors      `Crate.pair_tensors(radius, squared_distances=True)`
  neighbor_tensors  `Crate.neighbor_tensors(16, radius, squared_distances=True)`
  field_tensors     `Crate.field_tensors(values, radius, weight_sums=True)`, 2 channels
  field_function    forward and backward of `Crate.field_function(values, radius, weight_sums=True)` with gradients for
                    the values and the points, 2 channels

the wall time of the one batched call and of the loop over the frames (each a call with `points=` of one frame), the two
alternating inside one loop after a warm-up; median and min over the repetitions, and the ratio of the medians.  Before
anything is timed the batched results are compared with the loop's, concatenated and with the partners shifted: bit for
bit.  `kernels` gives the device time of the batched call's parts between HIP events -- the count, and the fill, the
table and the sum that read its grid -- and of one frame's, to say where a batched call's time goes.  One JSON line per
case, microseconds.
"""
import argparse
import json

from timing_support import alternate, bits_equal, device_times, median, record, stats, use_library, viewer_crate

K = 16
WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def functions(crate, radius):
    """name -> (batched(points, values, ptr), single(points, values)), each returning the tensors to compare."""
    import torch

    def grads(points, values, **kw):
        v, p = values.detach().requires_grad_(), points.detach().requires_grad_()
        sums, wsum = crate.field_function(v, radius, weight_sums=True, points=p, **kw)
        (sums.sum() + wsum.sum()).backward()
        torch.cuda.synchronize()
        return sums.detach(), wsum.detach(), v.grad, p.grad

    return {
        "pair_tensors": lambda points, values, **kw: crate.pair_tensors(radius, squared_distances=True, points=points, **kw),
        "neighbor_tensors": lambda points, values, **kw: crate.neighbor_tensors(K, radius, squared_distances=True,
                                                                                points=points, **kw),
        "field_tensors": lambda points, values, **kw: crate.field_tensors(values, radius, weight_sums=True, points=points, **kw),
        "field_function": grads,
    }


def joined(name, parts, ptr):
    """The loop's results as the batched call returns them: concatenated, partners shifted, offsets continued."""
    import torch
    starts = ptr[:-1].tolist()
    if name == "pair_tensors":
        offsets, at = [torch.zeros(1, dtype=torch.int64, device=ptr.device)], 0
        for o, _, _ in parts:
            offsets.append(o[1:] + at)
            at += int(o[-1])
        return (torch.cat(offsets), torch.cat([p + s for (_, p, _), s in zip(parts, starts)]), torch.cat([d for _, _, d in parts]))
    if name == "neighbor_tensors":
        return (torch.cat([torch.where(nb >= 0, nb + s, nb) for (nb, _), s in zip(parts, starts)]), torch.cat([d for _, d in parts]))
    return tuple(torch.cat([part[k] for part in parts]) for k in range(len(parts[0])))


def kernels(crate, radius, points, values, ptr, reps):
    """Device time of the count and of the three readers by events, into tensors made once; `ptr` None: unbatched."""
    import torch
    eng = crate.engine
    dev = points.device
    n = int(points.shape[0])
    offsets = torch.empty(n + 1, dtype=torch.int64, device=dev)
    counts, other = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2))
    eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, batch=ptr)
    eng.synchronize()
    total = int(counts[1])
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    table = torch.empty((n, K), dtype=torch.int64, device=dev)
    table_d2 = torch.empty((n, K), dtype=torch.float64, device=dev)
    sums = torch.empty((n, int(values.shape[1])), dtype=torch.float64, device=dev)
    wsum = torch.empty(n, dtype=torch.float64, device=dev)
    times = device_times(eng, {
        "count": lambda: eng.pairs_count(points, radius=radius, offsets=offsets, counts=counts, batch=ptr),
        "fill": lambda: eng.pairs_fill(partners, d2),
        "table": lambda: eng.pairs_nearest(table, table_d2, k=K, counts=other),
        "sum": lambda: eng.pairs_sum(values, sums, wsum, counts=other)}, reps, WARMUP)
    out = {"points": n, "pairs": total}
    for name, series in times.items():
        out.update(stats(series, f"{name}_device_"))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--clouds", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--lib", default=None, help="another build of libsandcrate_hip.so to time")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    use_library(args.lib)
    from sand_crate_amd import pairs

    crate = viewer_crate(0)
    frames = record(crate, args.clouds, args.ticks)
    radius = crate.diameter
    points = torch.cat(frames)
    ptr = pairs.batch_ptr([int(f.shape[0]) for f in frames], points.device)
    gen = torch.Generator(device=points.device).manual_seed(13)
    values = torch.randn((int(points.shape[0]), 2), dtype=torch.float64, device=points.device, generator=gen)
    cuts = ptr.tolist()
    frame_values = [values[a:b].contiguous() for a, b in zip(cuts[:-1], cuts[1:])]
    torch.cuda.synchronize()
    base = {"clouds": args.clouds, "points": int(points.shape[0]), "points_per_cloud": round(points.shape[0] / args.clouds, 1),
            "radius_in_diameters": 1.0}
    for name, fn in functions(crate, radius).items():
        batched = lambda: fn(points, values, batch=ptr)                                      # noqa: E731
        loop = lambda: [fn(p, v) for p, v in zip(frames, frame_values)]                      # noqa: E731
        got, want = batched(), joined(name, loop(), ptr)
        if len(got) != len(want) or not all(bits_equal(g, w) for g, w in zip(got, want)):
            raise SystemExit(f"{name}: the batched call differs from the loop")
        times = alternate({"loop": loop, "batched": batched}, args.reps, WARMUP)
        med = {key: median(t) for key, t in times.items()}
        print(json.dumps({**base, "case": name, **stats(times["batched"], "batched_wall_"), **stats(times["loop"], "loop_wall_"),
                          "single_call_wall_us": round(med["loop"] / args.clouds, 2),
                          "batched_over_loop": round(med["batched"] / med["loop"], 4),
                          "batched_over_single": round(med["batched"] * args.clouds / med["loop"], 2)}), flush=True)
    print(json.dumps({**base, "case": "kernels, batched", **kernels(crate, radius, points, values, ptr, args.reps)}), flush=True)
    print(json.dumps({**base, "case": "kernels, one frame",
                      **kernels(crate, radius, frames[0], frame_values[0], None, args.reps)}), flush=True)


if __name__ == "__main__":
    main()
