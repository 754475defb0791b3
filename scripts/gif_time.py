"""Time of one GIF frame on the GPU (sc_render_gif) against the host path it replaces, and against sc_render_jpeg.

    python scripts/gif_time.py [--reps 50] [--ticks 200]

The scene is config/wave_machine.yaml after --ticks ticks, the frame 1000 x 1000.  Per frame:

  render_gif     `Crate.render_gif`: device time between two HIP events on the library's stream -- the call synchronises
                 (it reads the length before it copies the bytes), so the span covers the kernels, the two copies to the
                 host and the host's share in between -- and the wall time of the call
  render_jpeg    the same two figures for `Crate.render_jpeg` at quality 95
  host GIF       the wall time of what `main --frames` does per frame without --gif: `Crate.render` with its download,
                 and the frame's share of PIL's `save(..., save_all=True, duration=10, loop=0)`, timed over a file of
                 the frames of --host-frames consecutive ticks (PIL quantises each frame to an adaptive palette on one
                 core, and stores the frames after the first as the rectangle that changed)

`rocprofv3 --kernel-trace --stats -- python scripts/gif_time.py` gives the kernels alone.  One JSON line per case: median
and min over the repetitions, in microseconds, and the size of a frame.
"""
import argparse
import io
import json
import time

from timing_support import device_times, median, stats, viewer_crate, with_wall


def time_gpu(crate, fn, reps):
    data, wall = None, []

    def call():
        nonlocal data
        data = fn()

    # 3 rounds of warm-up for the first-use costs: workspace growth, code object load
    device = device_times(crate.engine, {"call": with_wall(call, wall)}, reps, 3)["call"]
    return {**stats(device, "device_"), **stats(wall[-reps:], "wall_"), "bytes": len(data)}


def time_host_gif(crate, side, frames, reps):
    from PIL import Image
    render, save = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        crate.render(side, side)
        render.append(1e6 * (time.perf_counter() - t0))
    imgs = []
    for _ in range(frames):
        crate.physics_tick()
        imgs.append(crate.render(side, side))
    for _ in range(max(3, reps // 10)):
        t0 = time.perf_counter()
        images = [Image.fromarray(img, "RGB") for img in imgs]
        buf = io.BytesIO()
        images[0].save(buf, format="GIF", append_images=images[1:], save_all=True, duration=10, loop=0)
        save.append(1e6 * (time.perf_counter() - t0) / frames)
    median_render = median(render)
    both = [median_render + s for s in save]
    return {**stats(both, "wall_"), **stats(render, "render_wall_"), **stats(save, "pil_save_wall_"),
            "bytes": buf.tell() // frames}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--host-frames", type=int, default=4)
    args = ap.parse_args()
    import torch
    torch.cuda.init()

    side = 1000
    crate = viewer_crate(args.ticks)
    base = {"scene": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count, "frame": f"{side}x{side}"}
    print(json.dumps({**base, "case": "render_gif", **time_gpu(crate, lambda: crate.render_gif(side, side), args.reps)}),
          flush=True)
    print(json.dumps({**base, "case": "render_jpeg",
                      **time_gpu(crate, lambda: crate.render_jpeg(side, side, quality=95), args.reps)}), flush=True)
    print(json.dumps({**base, "case": "render_gif", **time_gpu(crate, lambda: crate.render_gif(side, side), args.reps)}),
          flush=True)  # (again, after the other: the spread between two runs of the same thing)
    try:
        host = time_host_gif(crate, side, args.host_frames, args.reps)
    except ImportError:
        print(json.dumps({**base, "case": "host GIF (render + download + PIL save)", "skipped": "PIL is not installed"}))
        return
    print(json.dumps({**base, "case": "host GIF (render + download + PIL save)", **host}), flush=True)


if __name__ == "__main__":
    main()
