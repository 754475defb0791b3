"""What the timing scripts share: how this project measures, written once.  A new `scripts/<name>_time.py` starts from
here (`from timing_support import ...`: a script's own directory is on `sys.path`) and keeps what is its own -- its
cases, its keys, its checks against the rule, its warm-up count, which it passes in.

    stats, median            median (element len // 2 of the sorted list) and min of a series, as the keys of a JSON line
    wall_us, alternate       host wall time; the sides of a comparison alternate inside one loop, after unrecorded warm-up
    device_times, with_wall  device time of library calls between HIP events, on the stream the library runs on; the
                             wall time of a call's enqueue inside that loop
    use_library              time another build of libsandcrate_hip.so (`--lib PATH`, or $SAND_CRATE_LIB) through the
                             same script: the tree's own library is never overwritten
    viewer_crate, bench_crate  the two states every script times on
    bits_equal, record       of the batch scripts: tensors equal bit for bit; the frames of consecutive ticks

Importing this puts the repository's root (the package, bench.py) and tests/ (the `*_spec.py` rules) on `sys.path`.
torch and the package are imported inside the functions: `--help` needs neither, and a script calls `torch.cuda.init()`
before anything here loads the library (torch's HIP runtime must come up first in a process that uses both)."""
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LIB_ENV = "SAND_CRATE_LIB"


def median(times):
    return sorted(times)[len(times) // 2]


def stats(times, prefix="", digits=2, maximum=False, unit="_us"):
    """-> {"<prefix>median<unit>", "<prefix>min<unit>"[, "<prefix>max<unit>"]}, rounded to `digits`."""
    times = sorted(times)
    out = {f"{prefix}median{unit}": round(times[len(times) // 2], digits), f"{prefix}min{unit}": round(times[0], digits)}
    if maximum:
        out[f"{prefix}max{unit}"] = round(times[-1], digits)
    return out


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return 1e6 * (time.perf_counter() - t0)


def with_wall(fn, into):
    """-> `fn` as a call that appends its own wall time, microseconds, to `into`: the enqueue inside `device_times`
    (the warm-up rounds are appended too: take `into[-reps:]`)."""
    def run():
        into.append(wall_us(fn))
    return run


def alternate(cases, reps, warmup):
    """{name: fn} -> {name: [wall us]}: every repetition runs each case once, in turn, after `warmup` rounds that are
    not recorded."""
    for _ in range(warmup):
        for fn in cases.values():
            fn()
    out = {name: [] for name in cases}
    for _ in range(reps):
        for name, fn in cases.items():
            out[name].append(wall_us(fn))
    return out


def device_times(eng, calls, reps, warmup):
    """{name: call} -> {name: [device us]}: every repetition records an event before each call and one after the last,
    after `warmup` rounds without events.  The engine runs on torch's current stream for the loop, so that the events
    bracket exactly the calls' launches, and on its own stream again afterwards."""
    import torch
    dev = torch.device("cuda", eng.device)
    stream = torch.cuda.current_stream(dev)
    eng.set_stream(stream.cuda_stream)
    names = list(calls)
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize(dev)
    out = {name: [] for name in names}
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(names) + 1)]
        for mark, name in zip(ev, names):
            mark.record(stream)
            calls[name]()
        ev[-1].record(stream)
        ev[-1].synchronize()
        for k, name in enumerate(names):
            out[name].append(1000.0 * ev[k].elapsed_time(ev[k + 1]))
    eng.use_own_stream()
    return out


def use_library(path=None):
    """Points the package at another build of libsandcrate_hip.so: `path`, else $SAND_CRATE_LIB, else nothing changes.
    -> the resolved path, or None.  Call it before the first crate is made: once the package has loaded a library it
    keeps that handle, so this raises instead of timing the wrong build."""
    path = path or os.environ.get(LIB_ENV)
    if not path:
        return None
    from sand_crate_amd import _native
    if _native._lib is not None:
        raise RuntimeError(f"use_library({str(path)!r}): the package has already loaded {_native.LIB_PATH}")
    _native.LIB_PATH = Path(path).resolve()
    return _native.LIB_PATH


def viewer_crate(ticks):
    """The viewer's state: config/wave_machine.yaml, default noise, after `ticks` calls of `physics_tick()`."""
    import sand_crate_amd as sc
    crate = sc.Crate(sc.load_config(ROOT / "config" / "wave_machine.yaml").world_config)
    for _ in range(ticks):
        crate.physics_tick()
    crate.synchronize()
    return crate


def bench_crate(n, ticks):
    """The benchmark's state: bench.py's world and generator at `n` particles, counter noise, after `run(ticks)`."""
    import bench
    import sand_crate_amd as sc
    wc, _ = bench.world_for(n)
    crate = sc.Crate(wc, noise="counter", noise_seed=1, capacity=n + 1024)
    crate.particles, crate.particle_velocities = bench.synthetic_state(n)
    crate.run(ticks)
    crate.synchronize()
    return crate


def bits_equal(a, b):
    import torch
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float64:
        a, b = a.contiguous().view(torch.int64), b.contiguous().view(torch.int64)
    return torch.equal(a, b)


def record(crate, clouds, ticks):
    """-> the frames, float64 (n_b, 2) CUDA tensors: the state after `ticks` ticks and after each of the next ones."""
    for _ in range(ticks):
        crate.physics_tick()
    frames = []
    for _ in range(clouds):
        frames.append(crate.state_tensors(pressure=False)[0].clone())
        crate.physics_tick()
    crate.synchronize()
    return frames
