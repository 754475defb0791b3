"""GPU time of one rendered frame (sc_render_device: clear + splat + resolve), measured with HIP events.

    python scripts/render_time.py [--reps 50]

Scenes: bench.py's M2 inputs (1,048,576 particles in the wave_machine world) after 5 ticks at 1000 x 1000 and
4096 x 4096, and config/wave_machine.yaml after 200 ticks of its source at 1000 x 1000 (discs of radius 5).  The
library runs on torch's current stream so that the events bracket exactly the render's launches.  Prints one JSON line
per case: median and min over the repetitions, in microseconds.
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def time_render(crate, width, height, reps):
    import torch
    stream = torch.cuda.current_stream()
    crate.engine.set_stream(stream.cuda_stream)
    out = torch.empty((height, width, 3), dtype=torch.uint8, device="cuda")
    for _ in range(3):  # first-use costs: buffer growth, code object load
        crate.render(width, height, out=out)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        crate.render(width, height, out=out)
        b.record(stream)
        b.synchronize()
        times.append(1000.0 * a.elapsed_time(b))
    crate.engine.use_own_stream()
    times.sort()
    return {"median_us": round(times[len(times) // 2], 2), "min_us": round(times[0], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    import bench
    import sand_crate_amd as sc

    n = 1048576
    wc, _ = bench.world_for(n)
    crate = sc.Crate(wc, noise="counter", noise_seed=1, capacity=n + 1024)
    crate.particles, crate.particle_velocities = bench.synthetic_state(n)
    crate.run(5)
    crate.synchronize()
    for side in (1000, 4096):
        radius = int(side * crate.particle_radius)
        print(json.dumps({"scene": "M2", "particles": crate.particle_count, "frame": f"{side}x{side}", "disc_radius": radius,
                          "splat": "wave per disc" if radius > 4 else "thread per particle",
                          **time_render(crate, side, side, args.reps)}), flush=True)
    del crate

    crate = sc.Crate(sc.load_config(ROOT / "config" / "wave_machine.yaml").world_config)
    for _ in range(200):
        crate.physics_tick()
    crate.synchronize()
    print(json.dumps({"scene": "wave_machine", "particles": crate.particle_count, "frame": "1000x1000", "disc_radius": 5,
                      "splat": "wave per disc", **time_render(crate, 1000, 1000, args.reps)}), flush=True)


if __name__ == "__main__":
    main()
