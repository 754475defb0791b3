"""Cost of recording trajectories on the device (`Crate.record_trajectory`) against the route there was before it.

    python scripts/trajectory_time.py [--reps 30] [--ticks 200] [--big 1048576] [--run-ticks 100]
    rocprofv3 --kernel-trace --stats -- python scripts/trajectory_time.py --frames-only 200 --state synthetic
                                                                      (the three kernels alone, one state per run)

Two states: config/wave_machine.yaml after --ticks ticks (the viewer's size) and --big synthetic particles (bench.py's
world and generator) after three ticks, so that the storage is cell-sorted.  Per state:

  frame: recorded      `Trajectory.capture()`: the three launches of one frame (reserve, clear, scatter) into a log that is
                       restarted before it fills -- device time between two events on the stream the library runs on, and
                       the wall time of the enqueue
  frame: export+copy   the route without the recorder: `Engine.export_state(ids)` (the radix sort by id and the gather)
                       into tensors made once, then torch's `fill_` of an (M, 4) frame with NaN and `index_copy_` of the
                       n exported rows into it at their ids -- the same events, the same stream.  (`index_copy_` takes
                       the n rows of the host's last count; a caller without one pays a synchronisation on top.)
  tick: ...            ticks per second over --run-ticks ticks ending in a synchronisation, recording off and on
                       (every=1), alternating in one loop.  The big state through `Crate.run` -- without a recording each
                       tick is fused with its successor's wall pass, a recorded tick is not -- and through `physics_tick`,
                       which never fuses: the difference between the two "off" lines is the look-ahead, the difference
                       between `physics_tick` off and on is the three kernels.  wave_machine has active sources: only
                       `physics_tick`.

The sides of a comparison alternate inside one loop.  Before anything is timed a recorded frame is compared with the
export scattered by torch, byte for byte.  One JSON line per case: median, min and max over the repetitions."""
import argparse
import json
import time
from functools import partial

import timing_support
from timing_support import bench_crate, viewer_crate

stats = partial(timing_support.stats, maximum=True, unit="")                         # (the unit is in the prefix: us, ticks per s)


class Frames:
    """The two routes to one (M, 4) frame, on torch's current stream."""

    def __init__(self, crate, rows):
        import torch
        self.torch, self.crate, self.eng, self.rows = torch, crate, crate.engine, rows
        self.dev = torch.device("cuda", self.eng.device)
        self.stream = torch.cuda.current_stream(self.dev)
        room = self.eng.capacity
        self.p, self.v = (torch.empty((room, 2), dtype=torch.float64, device=self.dev) for _ in range(2))
        self.ids = torch.empty(room, dtype=torch.int64, device=self.dev)
        self.count = torch.empty(1, dtype=torch.int64, device=self.dev)
        ids = self.eng.download()[3]
        self.n = len(ids)
        self.rows = rows = max(rows, int(ids.max()) + 1 if self.n else 0)  # (every id has a row: index_copy_ stays in bounds)
        self.frame = torch.empty((rows, 4), dtype=torch.float64, device=self.dev)
        self.eng.set_stream(self.stream.cuda_stream)
        self.rec = crate.record_trajectory(8, ids=(0, rows), initial=False)
        self.taken = 0

    def recorded(self):
        if self.taken == self.rec.frames:
            self.rec.restart()
            self.taken = 0
        self.rec.capture()
        self.taken += 1

    def export_copy(self):
        self.eng.export_state(self.p, self.v, None, self.ids, count=self.count)
        self.frame.fill_(float("nan"))
        self.frame[:, 0:2].index_copy_(0, self.ids[:self.n], self.p[:self.n])
        self.frame[:, 2:4].index_copy_(0, self.ids[:self.n], self.v[:self.n])

    def check(self):
        self.rec.restart()
        self.taken = 0
        self.recorded()
        self.export_copy()
        got = self.rec.read()["states"][0]
        self.torch.cuda.synchronize(self.dev)
        if got.cpu().numpy().tobytes() != self.frame.cpu().numpy().tobytes():
            raise SystemExit("the recorded frame differs from the export scattered by torch")

    def time(self, reps):
        torch = self.torch
        cases = {"recorded": self.recorded, "export+copy": self.export_copy}
        out = {name: ([], []) for name in cases}
        for rep in range(reps + 3):
            for name, fn in cases.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(self.stream)
                t0 = time.perf_counter()
                fn()
                wall = 1e6 * (time.perf_counter() - t0)
                b.record(self.stream)
                b.synchronize()
                if rep >= 3:
                    out[name][0].append(1000.0 * a.elapsed_time(b))
                    out[name][1].append(wall)
        return {name: {**stats(d, "device_us_"), **stats(w, "enqueue_wall_us_")} for name, (d, w) in out.items()}

    def close(self):
        self.crate.stop_trajectory()
        self.eng.use_own_stream()


def ticks_per_s(crate, advance, ticks, reps, rows):
    """-> {"off": [...], "on": [...]} ticks per second, the two alternating."""
    out = {"off": [], "on": []}
    for rep in range(reps + 1):
        for mode in ("off", "on"):
            if mode == "on":
                crate.record_trajectory(ticks + 1, ids=(0, rows), initial=False)
            crate.synchronize()
            t0 = time.perf_counter()
            advance(ticks)
            crate.synchronize()
            dt = time.perf_counter() - t0
            if mode == "on":
                crate.stop_trajectory()
            if rep:
                out[mode].append(ticks / dt)
    return out


def by_tick(crate):
    def advance(k):
        for _ in range(k):
            crate.physics_tick()
    return advance


def measure(crate, base, reps, run_ticks, rows, can_run):
    frames = Frames(crate, rows)
    frames.check()
    for name, row in frames.time(reps).items():
        print(json.dumps({**base, "case": f"frame: {name}", "rows": rows, **row}), flush=True)
    frames.close()
    paths = {"physics_tick": by_tick(crate)}
    if can_run:
        paths["run"] = crate.run
    for path, advance in paths.items():
        for mode, rates in ticks_per_s(crate, advance, run_ticks, max(3, reps // 6), rows).items():
            print(json.dumps({**base, "case": f"tick: {path}, recording {mode}", "ticks": run_ticks,
                              **stats(rates, "ticks_per_s_", 1)}), flush=True)


def frames_only(n_frames, ticks, big, which):
    """For the profiler: `n_frames` recorded frames of each state and nothing else that is timed."""
    for _, crate, rows in states(ticks, big, which):
        rec = crate.record_trajectory(8, ids=(0, rows), initial=False)
        for k in range(n_frames):
            if k % 8 == 0:
                rec.restart()
            rec.capture()
        crate.close()


def states(ticks, big, which="both"):
    """-> (name, crate, rows of the default window) per state."""
    if which in ("both", "wave_machine"):
        crate = viewer_crate(ticks)
        yield "wave_machine", crate, int(crate.world_config.coefficients["max_particles"])
    if which == "wave_machine":
        return
    crate = bench_crate(big, 3)
    yield "synthetic", crate, big


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--big", type=int, default=1048576)
    ap.add_argument("--run-ticks", type=int, default=100)
    ap.add_argument("--frames-only", type=int, default=0, metavar="N")
    ap.add_argument("--state", default="both", choices=["both", "wave_machine", "synthetic"])
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    if args.frames_only:
        frames_only(args.frames_only, args.ticks, args.big, args.state)
        return
    for name, crate, rows in states(args.ticks, args.big, args.state):
        small = name == "wave_machine"   # (ten times the ticks at the viewer's size: a window of some tenths of a second)
        base = {"state": name, "particles": crate.particle_count}
        measure(crate, base, args.reps, args.run_ticks * (10 if small else 1), rows, can_run=not small)
        crate.close()


if __name__ == "__main__":
    main()
