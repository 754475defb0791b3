"""GPU time the probe's log (sc_probe_enable) adds to a tick, measured with HIP events.

    python scripts/probe_time.py [--ticks 100] [--blocks 5] [--rounds 3]

Scenes: bench.py's M2 inputs (1,048,576 particles in the wave_machine world, `Crate.run` blocks of --ticks ticks) and, for
the viewer's end, config/wave_machine.yaml after 215 ticks of its source (about 3,000 particles), continued with
noise="counter" and no active source through `physics_tick()` loops of 4 x --ticks ticks.  The library runs on torch's
current stream so that the events bracket exactly a block's launches.  Per scene: --blocks blocks with the log off, on
without bins and on with 1,024 bins, in --rounds alternating rounds after a warm-up block each; the log is read (and so
cleared) between blocks, outside the events.  Prints one JSON line per round and setting -- median and min microseconds
per tick over its blocks -- then the medians over all rounds, what each setting adds per tick, the spread of the log-off
rounds' medians, and the time of a device-to-device copy of 40 bytes per particle (x, y, vx, vy, P once: the traffic the
probe cannot avoid), with the ratio of the two."""
import argparse
import json
from functools import partial

import timing_support
from timing_support import ROOT, bench_crate, viewer_crate

SETTINGS = {"off": None, "on, no bins": 0, "on, 1024 bins": 1024}
stats = partial(timing_support.stats, digits=3)                                      # (per tick: three digits)


def block_times(crate, advance, ticks, blocks, bins):
    """Device microseconds per tick of `blocks` blocks of `ticks` ticks (`advance(ticks)` runs one), after a warm-up block."""
    import torch
    stream = torch.cuda.current_stream()
    if bins is not None:
        crate.observe(capacity=ticks, bins=bins)
    times = []
    for k in range(blocks + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        advance(ticks)
        b.record(stream)
        b.synchronize()
        if bins is not None:
            got = crate.observations()
            assert len(got["tick"]) == ticks and got["dropped"] == 0
        if k > 0:
            times.append(1000.0 * a.elapsed_time(b) / ticks)
    if bins is not None:
        crate.observe(False)
        crate.observations()
    return times


def copy_time(n, reps=50):
    import torch
    src = torch.rand(5 * n, dtype=torch.float64, device="cuda")
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream()
    for _ in range(5):
        dst.copy_(src)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        dst.copy_(src)
        b.record(stream)
        b.synchronize()
        times.append(1000.0 * a.elapsed_time(b))
    return stats(times)


def report(head, crate, advance, ticks, blocks, rounds):
    import torch
    crate.engine.set_stream(torch.cuda.current_stream().cuda_stream)
    has_probe = hasattr(crate, "observe")
    settings = SETTINGS if has_probe else {"off": None}
    print(json.dumps({**head, "particles": crate.particle_count, "ticks_per_block": ticks, "probe_available": has_probe}), flush=True)
    got = {name: [] for name in settings}
    medians = {name: [] for name in settings}
    for rnd in range(rounds):
        for name, bins in settings.items():
            times = block_times(crate, advance, ticks, blocks, bins)
            got[name] += times
            medians[name].append(stats(times)["median_us"])
            print(json.dumps({**head, "log": name, "round": rnd, "clock": "device, per tick", **stats(times)}), flush=True)
    off = stats(got["off"])["median_us"]
    print(json.dumps({**head, "log": "off", "all_rounds": True, **stats(got["off"]),
                      "spread_of_round_medians_us": round(max(medians["off"]) - min(medians["off"]), 3)}), flush=True)
    n = crate.particle_count
    copy = copy_time(max(n, 1))
    print(json.dumps({**head, "copy_of_40_bytes_per_particle": True, "bytes": 40 * n, **copy}), flush=True)
    for name in list(settings)[1:]:
        on = stats(got[name])["median_us"]
        print(json.dumps({**head, "log": name, "all_rounds": True, **stats(got[name]), "added_us_per_tick": round(on - off, 3),
                          "added_over_copy": round((on - off) / copy["median_us"], 2)}), flush=True)
    crate.engine.use_own_stream()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import sand_crate_amd as sc

    crate = bench_crate(1048576, 20)
    report({"scene": "M2"}, crate, crate.run, args.ticks, args.blocks, args.rounds)
    del crate

    seed = viewer_crate(215)
    wc = sc.load_config(ROOT / "config" / "wave_machine.yaml").world_config
    wc.particle_sources = []
    crate = sc.Crate(wc, noise="counter", noise_seed=1)
    crate.rigid_bodies = seed.rigid_bodies
    crate.particles = seed.particles
    crate.particle_velocities = seed.particle_velocities
    del seed

    def advance(ticks):
        for _ in range(ticks):
            crate.physics_tick()

    report({"scene": "wave_machine"}, crate, advance, 4 * args.ticks, args.blocks, args.rounds)


if __name__ == "__main__":
    main()
