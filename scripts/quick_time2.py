"""Wall time per tick only (no kernel events): python scripts/quick_time2.py <tag> [particles] [ticks]"""
import sys, time
import numpy as np
from timing_support import bench_crate, use_library
use_library()  # $SAND_CRATE_LIB: a variant build (scripts/run_variants.sh), else the package's own library
tag = sys.argv[1] if len(sys.argv) > 1 else ""
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1048576
k = int(sys.argv[3]) if len(sys.argv) > 3 else 20
res = []
for rep in range(5):
    s = bench_crate(n, 5)
    t0 = time.perf_counter(); s.run(k); s.synchronize(); res.append((time.perf_counter() - t0) / k)
    state = s.engine.download()
print(f"{tag:30s} tick {1e6 * np.median(res):7.1f} us (min {1e6 * min(res):.1f} max {1e6 * max(res):.1f})  checksum {float(state[0].sum()):.12f} {float(state[1].sum()):.12f}", flush=True)
