"""Wall time per tick of the contract workload in its pile-up regime (ticks 400-499 of a 500-tick run, no events) and
the kernels' HIP-event times over ticks 500-549.   python scripts/pile_time.py [tag] [particles]"""
import sys, time
from timing_support import bench_crate, use_library
use_library()  # $SAND_CRATE_LIB: a variant build (scripts/run_variants.sh), else the package's own library
tag = sys.argv[1] if len(sys.argv) > 1 else ""
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1048576
s = bench_crate(n, 400)
t0 = time.perf_counter(); s.run(100); s.synchronize(); wall = (time.perf_counter() - t0) / 100
e = s.engine
e.reset_timing(); e.enable_timing(True); s.run(50); s.synchronize(); e.enable_timing(False)
tm = {k: round(1000 * ms / 50, 1) for k, (ms, c) in e.timing().items() if c}
print(f"{tag:40s} ticks 400-499: {1e6 * wall:7.1f} us/tick   kernels per tick (ticks 500-549, events): {tm}", flush=True)
