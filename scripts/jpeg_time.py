"""Time of one JPEG frame on the GPU (sc_jpeg_encode_device, sc_render_jpeg) against PIL on the host.

    python scripts/jpeg_time.py [--reps 50]

Cases: encoding alone of a rendered frame at 1000 x 1000 and 4096 x 4096 (bench.py's M2 scene, 1,048,576 particles after
5 ticks), render + encode of the same scene at both sizes, and render + encode of config/wave_machine.yaml after 200
ticks at 1000 x 1000.  The library runs on torch's current stream, and two HIP events bracket each call: the call
synchronises (it reads the file's length before copying the bytes), so the span covers the kernels, the two copies
to the host and the host's share in between.  `rocprofv3 --kernel-trace --stats -- python scripts/jpeg_time.py` gives the
kernels alone.  PIL's time is the host's for the same frame (quality 95, 4:4:4).  One JSON line per case: median and
min over the repetitions, in microseconds, and the file's size.
"""
import argparse
import io
import json
import time

from timing_support import bench_crate, device_times, stats, viewer_crate


def time_gpu(crate, fn, reps):
    data = None

    def call():
        nonlocal data
        data = fn()

    # 3 rounds of warm-up for the first-use costs: workspace growth, code object load
    times = device_times(crate.engine, {"call": call}, reps, 3)
    return {**stats(times["call"]), "bytes": len(data)}


def time_pil(img, reps):
    from PIL import Image
    times = []
    for _ in range(max(3, reps // 5)):
        t0 = time.perf_counter()
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=95, subsampling=0)
        times.append(1e6 * (time.perf_counter() - t0))
    return {**stats(times), "bytes": buf.tell()}


def cases(crate, name, sides, reps, encode_alone):
    import torch
    for side in sides:
        base = {"scene": name, "particles": crate.particle_count, "frame": f"{side}x{side}"}
        if encode_alone:
            frame = torch.empty((side, side, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            crate.render(side, side, out=frame)
            crate.synchronize()
            print(json.dumps({**base, "case": "encode", **time_gpu(crate, lambda: crate.engine.encode_jpeg(frame, 95),
                                                                   reps)}), flush=True)
        print(json.dumps({**base, "case": "render+encode",
                          **time_gpu(crate, lambda: crate.render_jpeg(side, side, quality=95), reps)}), flush=True)
        try:
            host = time_pil(crate.render(side, side), reps)
        except ImportError:
            continue
        print(json.dumps({**base, "case": "PIL encode (host)", **host}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()
    import torch
    torch.cuda.init()

    crate = bench_crate(1048576, 5)
    cases(crate, "M2", (1000, 4096), args.reps, True)
    del crate

    crate = viewer_crate(200)
    cases(crate, "wave_machine", (1000,), args.reps, False)


if __name__ == "__main__":
    main()
