"""GPU time of one rendered frame (sc_render_device: clear + splat + resolve), measured with HIP events.

    python scripts/render_time.py [--reps 50] [--hud | --arrows]

Scenes: bench.py's M2 inputs (1,048,576 particles in the wave_machine world) after 5 ticks at 1000 x 1000 and
4096 x 4096, and config/wave_machine.yaml after 200 ticks of its source at 1000 x 1000 (discs of radius 5).  The
library runs on torch's current stream so that the events bracket exactly the render's launches.  Prints one JSON line
per case: median and min over the repetitions, in microseconds.

--hud measures the HUD overlay (sc_set_hud) instead: config/wave_machine.yaml after 200 ticks with `show_forces()` on, at
1000 x 1000; `render` (device time, HIP events), `render_jpeg` and `render_gif` (host wall time: both synchronise), each
without and with `hud=True`, in two alternating rounds, and the time `hud=True` adds (the difference of the medians of
all rounds).  Beside it the host alternative: download the frame, PIL.ImageDraw.text, upload it again (skipped without
PIL).  The rows without a HUD use nothing this option's commit added, so the same script times an older library.

--arrows measures the debug arrows (sc_set_arrows) instead: the M2 inputs after 5 ticks at 1000 x 1000, `render` (device
time, HIP events) without arrows, with a list of 2,048 seeded arrows, and with velocity arrows for every 64th particle,
in three alternating rounds; then the medians over all rounds, what each kind of arrows adds, and the spread of the
arrow-free rounds' medians.  The rows without arrows use nothing this option's commit added, so the same script times an
older library.
"""
import argparse
import json

from timing_support import ROOT, alternate, bench_crate, device_times, stats, viewer_crate

WARMUP = 3                            # rounds before anything is recorded: first-use costs, buffer growth, code object load


def render_times(crate, width, height, reps, **kw):
    """Device time of `reps` renders (with these keywords of `Crate.render`), HIP events around each."""
    import torch
    out = torch.empty((height, width, 3), dtype=torch.uint8, device="cuda")
    return device_times(crate.engine, {"render": lambda: crate.render(width, height, out=out, **kw)}, reps, WARMUP)["render"]


def time_render(crate, width, height, reps):
    return stats(render_times(crate, width, height, reps))


def wall_times(call, reps):
    """Host wall time of a call that ends in a device synchronise."""
    return alternate({"call": call}, reps, WARMUP)["call"]


def hud_report(reps):
    import numpy as np
    import sand_crate_amd as sc
    side = 1000
    crate = sc.Crate(sc.load_config(ROOT / "config" / "wave_machine.yaml").world_config)
    crate.show_forces()
    for _ in range(200):
        crate.physics_tick()
    crate.synchronize()
    has_hud = hasattr(crate.engine, "set_hud")
    text = crate.debug_prints
    lines = text.split("\n")
    head = {"scene": "wave_machine", "ticks": 200, "particles": crate.particle_count, "frame": f"{side}x{side}"}
    print(json.dumps({**head, "hud_bytes": len(text), "hud_lines": len(lines), "hud_longest_line": max(map(len, lines)),
                      "hud_available": has_hud}), flush=True)
    cases = {
        "render": ("device", lambda **kw: render_times(crate, side, side, reps, **kw)),
        "render_jpeg": ("wall", lambda **kw: wall_times(lambda: crate.render_jpeg(side, side, **kw), reps)),
        "render_gif": ("wall", lambda **kw: wall_times(lambda: crate.render_gif(side, side, **kw), reps)),
    }
    for name, (clock, measure) in cases.items():
        got = {False: [], True: []}
        for rnd in range(2):
            for hud in ((False, True) if has_hud else (False,)):
                times = measure(**({"hud": True} if hud else {}))
                got[hud] += times
                print(json.dumps({**head, "case": name, "hud": hud, "round": rnd, "clock": clock, **stats(times)}), flush=True)
        if has_hud:
            off, on = stats(got[False])["median_us"], stats(got[True])["median_us"]
            print(json.dumps({**head, "case": name, "hud_added_us": round(on - off, 2), "off_median_us": off,
                              "on_median_us": on}), flush=True)
    try:
        from PIL import Image, ImageDraw
    except ImportError:
        print(json.dumps({**head, "case": "host HUD (download + PIL text + upload)", "skipped": "PIL is not installed"}))
        return
    import torch

    def host_hud():
        frame = crate.render(side, side)
        image = Image.fromarray(frame, "RGB")
        ImageDraw.Draw(image).multiline_text((6, 6), text, fill=(255, 255, 255))
        dev = torch.from_numpy(np.array(image)).cuda()
        torch.cuda.synchronize()
        return dev

    plain = stats(wall_times(lambda: crate.render(side, side), reps))
    whole = stats(wall_times(host_hud, reps))
    print(json.dumps({**head, "case": "host HUD (download + PIL text + upload)", "clock": "wall", **whole,
                      "render_to_host_median_us": plain["median_us"],
                      "added_over_device_frame_us": round(whole["median_us"] - stats(render_times(crate, side, side, reps))["median_us"], 2)}),
          flush=True)


def arrows_report(reps, rounds=3):
    import numpy as np
    side = 1000
    crate = bench_crate(1048576, 5)
    has_arrows = hasattr(crate.engine, "set_arrows")
    rs = np.random.RandomState(2048)
    pairs = np.stack([rs.rand(2048, 2), (rs.rand(2048, 2) - 0.5) * 0.1], axis=1)  # (start, direction): 10 to 40 pixels
    head = {"scene": "M2", "ticks": 5, "particles": crate.particle_count, "frame": f"{side}x{side}"}
    print(json.dumps({**head, "arrows_available": has_arrows}), flush=True)
    kinds = {"none": {}}
    if has_arrows:
        kinds["list of 2048"] = {"arrows": pairs}
        kinds["velocity, every 64th"] = {"arrows": "velocity", "arrow_every": 64}
    got = {kind: [] for kind in kinds}
    medians = {kind: [] for kind in kinds}
    for rnd in range(rounds):
        for kind, kw in kinds.items():
            times = render_times(crate, side, side, reps, **kw)
            got[kind] += times
            medians[kind].append(stats(times)["median_us"])
            print(json.dumps({**head, "arrows": kind, "round": rnd, "clock": "device", **stats(times)}), flush=True)
    off = stats(got["none"])["median_us"]
    print(json.dumps({**head, "arrows": "none", "all_rounds": True, **stats(got["none"]),
                      "spread_of_round_medians_us": round(max(medians["none"]) - min(medians["none"]), 2)}), flush=True)
    for kind in list(kinds)[1:]:
        on = stats(got[kind])["median_us"]
        print(json.dumps({**head, "arrows": kind, "all_rounds": True, **stats(got[kind]),
                          "added_us": round(on - off, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--hud", action="store_true", help="measure the HUD overlay instead (see above)")
    ap.add_argument("--arrows", action="store_true", help="measure the debug arrows instead (see above)")
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    if args.hud:
        hud_report(args.reps)
        return
    if args.arrows:
        arrows_report(args.reps)
        return

    crate = bench_crate(1048576, 5)
    for side in (1000, 4096):
        radius = int(side * crate.particle_radius)
        print(json.dumps({"scene": "M2", "particles": crate.particle_count, "frame": f"{side}x{side}", "disc_radius": radius,
                          "splat": "wave per disc" if radius > 4 else "thread per particle",
                          **time_render(crate, side, side, args.reps)}), flush=True)
    del crate

    crate = viewer_crate(200)
    print(json.dumps({"scene": "wave_machine", "particles": crate.particle_count, "frame": "1000x1000", "disc_radius": 5,
                      "splat": "wave per disc", **time_render(crate, 1000, 1000, args.reps)}), flush=True)


if __name__ == "__main__":
    main()
