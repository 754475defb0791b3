"""Pass A split into its two halves at full size: the search alone (ENUM launch) and the pair math alone (DENS launch
reading the lists back), via the host-noise path of the C ABI with a zero noise block."""
import sys
import numpy as np
from timing_support import bench_crate, use_library
use_library()  # $SAND_CRATE_LIB: a variant build (scripts/run_variants.sh), else the package's own library
import bench, sand_crate_amd as sc
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
c = bench_crate(n, 10)
p, v, _, _ = c.engine.download()
h = sc.Crate(bench.world_for(n)[0], noise="host-sync", capacity=n + 1024)
e = h.engine
acc = {}
for rep in range(6):
    e.upload(p, v)
    for b in h.rigid_bodies: b.apply_velocity(h.dt)
    h._send_tick_inputs()
    e.synchronize(); e.reset_timing(); e.enable_timing(True)
    e.step_begin()
    st = e.step_stats()
    e.set_noise_host(np.full((st.neighbor_slots, 2), 0.5))
    e.step_finish(); e.synchronize(); e.enable_timing(False)
    for k, (ms, cnt) in e.timing().items():
        if cnt and rep: acc.setdefault(k, []).append(1000 * ms / cnt)
print({k: round(float(np.median(x)), 1) for k, x in acc.items()}, "mean C", st.neighbor_slots / st.particles)
