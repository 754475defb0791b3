"""Time of the device pair search against the only route there was: the state over PCIe, then a host search.

    python scripts/pairs_time.py [--reps 30] [--ticks 200] [--big 1048576]

Two states, the ones scripts/state_time.py uses: config/wave_machine.yaml after --ticks ticks (the viewer's size) and --big
synthetic particles (bench.py's world and generator) after three ticks.  Radius = the crate's diameter.  Per state:

  download         `Engine.download()`: wall time of the call (it synchronises) -- the floor of the host route, before any
                   search has started
  state_tensors    `Crate.state_tensors(ids=True)`: wall time of the call
  pair_tensors     `Crate.pair_tensors(squared_distances=True)`: wall time of the whole call -- count, one synchronisation,
                   the 16-byte read of (n, E), two allocations of E entries, fill, synchronisation
  pair kernels     `Engine.pairs_count` and `Engine.pairs_fill` into tensors made once: device time between HIP events on
                   the stream the library runs on, and the bytes the kernels write to the caller's tensors (8 (n + 1) of
                   offsets, 16 E of partners and distances) over that time as a fraction of an 8 TB/s roofline
  host search      (viewer's size only) NumPy brute force in row blocks (tests/pairs_spec.py) over the downloaded
                   state, for scale

The sides of a comparison alternate inside one loop.  Before anything is timed the device list is compared with the NumPy
rule on the small state, and `half` with the full list on the big one.  One JSON line per case: median and min over the
repetitions, in microseconds.
"""
import argparse
import json
import time

import numpy as np

from timing_support import alternate, bench_crate, device_times, median, stats, viewer_crate, wall_us

ROOFLINE_BYTES_PER_S = 8e12
WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def pair_kernels(crate, reps, total):
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    offsets = torch.empty(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    radius = crate.diameter
    began, wall = [], []                  # the enqueue of both calls: from before the count to after the fill

    def count():
        began.append(time.perf_counter())
        eng.pairs_count(None, radius=radius, offsets=offsets, counts=counts)

    def fill():
        eng.pairs_fill(partners, d2)
        wall.append(1e6 * (time.perf_counter() - began[-1]))

    times = device_times(eng, {"count": count, "fill": fill}, reps, WARMUP)
    n = int(counts[0])
    written = 8 * (n + 1) + 16 * total
    both = median([x + y for x, y in zip(times["count"], times["fill"])])
    return {**stats(times["count"], "count_device_"), **stats(times["fill"], "fill_device_"),
            **stats(wall[-reps:], "enqueue_wall_"), "bytes_written": written,
            "roofline_fraction": round(written / (both * 1e-6) / ROOFLINE_BYTES_PER_S, 4)}


def measure(crate, base, reps, check_rule):
    import torch
    eng = crate.engine
    offsets, partners, d2 = crate.pair_tensors(squared_distances=True)
    n, total = len(offsets) - 1, len(partners)
    if check_rule:
        import pairs_spec
        want = pairs_spec.pairs(crate.state_tensors()[0].cpu().numpy(), crate.diameter)
        for g, w in zip((offsets, partners, d2), want):
            if g.cpu().numpy().tobytes() != w.tobytes():
                raise SystemExit("pair_tensors differs from the rule")
    else:
        half = crate.pair_tensors(half=True)
        if 2 * len(half[1]) != total or not bool((d2 <= crate.diameter * crate.diameter).all()):
            raise SystemExit("the half list is not half the list")
    base = {**base, "E": total, "E_per_n": round(total / max(n, 1), 3)}
    times = alternate({"download": eng.download, "state_tensors": lambda: crate.state_tensors(ids=True),
                       "pair_tensors": lambda: crate.pair_tensors(squared_distances=True)}, reps, WARMUP)
    for name, t in times.items():
        print(json.dumps({**base, "case": name, **stats(t, "wall_")}), flush=True)
    print(json.dumps({**base, "case": "pair kernels", **pair_kernels(crate, reps, total)}), flush=True)
    if check_rule:
        import pairs_spec
        p = eng.download()[0]
        t = [wall_us(lambda: pairs_spec.pairs(p, crate.diameter)) for _ in range(5)]
        print(json.dumps({**base, "case": "host search (NumPy brute force, after the download)", **stats(t, "wall_")}), flush=True)
    med = {name: median(t) for name, t in times.items()}
    print(json.dumps({**base, "case": "verdict", "pair_tensors_over_download": round(med["pair_tensors"] / med["download"], 4),
                      "pair_tensors_is_faster_than_download": bool(med["pair_tensors"] < med["download"])}), flush=True)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    args = ap.parse_args()
    import torch
    torch.cuda.init()

    crate = viewer_crate(args.ticks)
    measure(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps, True)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    measure(crate, {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}, max(5, args.reps // 3), False)


if __name__ == "__main__":
    main()
