import sys, time
from timing_support import bench_crate, use_library
use_library()  # $SAND_CRATE_LIB: a variant build (scripts/run_variants.sh), else the package's own library
tag = sys.argv[1] if len(sys.argv) > 1 else ""
n = int(sys.argv[2]) if len(sys.argv) > 2 else 262144
s = bench_crate(n, 5)
t0 = time.perf_counter(); s.run(60); s.synchronize(); el = (time.perf_counter() - t0) / 60
s = bench_crate(n, 5); e = s.engine; e.reset_timing(); e.enable_timing(True); s.run(60); s.synchronize(); e.enable_timing(False)
tm = {k: round(1000*ms/c, 1) for k, (ms, c) in e.timing().items() if c}
print(f"{tag:60s} tick {el*1e6:7.1f} us  A {tm.get('neighbors_density')}  B {tm.get('force_integrate')}  AB {tm.get('neighbors_density_force')}  sort {tm.get('wall_bin')}+{tm.get('cell_scan')}+{tm.get('scatter')}+{tm.get('reorder')}", flush=True)
