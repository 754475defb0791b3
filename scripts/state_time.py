"""Time of the state exchange with torch on the device against the host path it stands next to.

    python scripts/state_time.py [--reps 30] [--ticks 200] [--big 1048576]

Two states: config/wave_machine.yaml after --ticks ticks (the viewer's size, about 3,000 particles) and --big synthetic
particles (bench.py's world and generator) after three ticks, so that the storage is cell-sorted.  Per state:

  download         `Engine.download()`: wall time of the call (it synchronises): five arrays over PCIe, a host sort by id,
                   a host loop that interleaves
  state_tensors    `Crate.state_tensors(ids=True)`: wall time of the call (it synchronises and reads the 8-byte count)
  export kernels   `Engine.export_state` into tensors made once: device time between two HIP events on the stream the
                   library runs on -- the sort's passes and the gather, nothing else -- and the wall time of the enqueue
  upload           `Engine.upload(p, v)` + `synchronize()`: wall time, NumPy arrays through the staging copy
  load_tensors     `Crate.load_state_tensors(p, v)` + `synchronize()`: wall time, CUDA tensors
  upload_ids / load_tensors_ids   the same two with ids (`upload_with_ids`; the device form synchronises once for them)

The two sides of a comparison alternate inside one loop.  Before anything is timed the exported tensors are compared
with the download, byte for byte.  One JSON line per case: median and min over the repetitions, in microseconds.
"""
import argparse
import json

import numpy as np

from timing_support import alternate, bench_crate, device_times, stats, viewer_crate, with_wall

WARMUP = 3                            # rounds before anything is recorded, wall and device alike


def check_equal(crate):
    got = crate.state_tensors(ids=True)
    want = crate.engine.download()
    for g, w in zip(got, want):
        if g.cpu().numpy().tobytes() != np.ascontiguousarray(w).tobytes():
            raise SystemExit("state_tensors differs from download")


def export_kernels(crate, reps):
    import torch
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    room = eng.capacity
    p, v = (torch.empty((room, 2), dtype=torch.float64, device=dev) for _ in range(2))
    pr = torch.empty(room, dtype=torch.float64, device=dev)
    ids = torch.empty(room, dtype=torch.int64, device=dev)
    count = torch.empty(1, dtype=torch.int64, device=dev)
    wall = []
    export = with_wall(lambda: eng.export_state(p, v, pr, ids, count=count), wall)
    device = device_times(eng, {"export": export}, reps, WARMUP)["export"]
    return {**stats(device, "device_"), **stats(wall[-reps:], "enqueue_wall_")}


def measure(crate, base, reps):
    import torch
    check_equal(crate)
    eng = crate.engine
    times = alternate({"download": eng.download, "state_tensors": lambda: crate.state_tensors(ids=True)}, reps, WARMUP)
    for name, t in times.items():
        print(json.dumps({**base, "case": name, **stats(t, "wall_")}), flush=True)
    print(json.dumps({**base, "case": "export kernels", **export_kernels(crate, reps)}), flush=True)

    p, v, _, ids = eng.download()
    tp, tv, ti = (torch.from_numpy(a).to(f"cuda:{eng.device}") for a in (p, v, ids))
    torch.cuda.synchronize()

    def synced(fn):
        def run():
            fn()
            eng.synchronize()
        return run

    times = alternate({"upload": synced(lambda: eng.upload(p, v)),
                       "load_tensors": synced(lambda: crate.load_state_tensors(tp, tv)),
                       "upload_ids": synced(lambda: eng.upload_with_ids(p, v, ids)),
                       "load_tensors_ids": synced(lambda: crate.load_state_tensors(tp, tv, ti))}, reps, WARMUP)
    for name, t in times.items():
        print(json.dumps({**base, "case": name, **stats(t, "wall_")}), flush=True)
    check_equal(crate)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    args = ap.parse_args()
    import torch
    torch.cuda.init()

    crate = viewer_crate(args.ticks)
    measure(crate, {"state": "wave_machine", "ticks": args.ticks, "particles": crate.particle_count}, args.reps)
    crate.engine.close()

    crate = bench_crate(args.big, 3)
    measure(crate, {"state": "synthetic", "ticks": 3, "particles": crate.particle_count}, max(5, args.reps // 3))


if __name__ == "__main__":
    main()
