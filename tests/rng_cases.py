"""The emission cases the device stream is pinned against (tests/test_gpu_rng_stream.py), and NumPy's emission rule.

`generate_particles` (particle_source.py:17-24) is the spec: binomial(flow, dt), then rand(count, 2) for the position
jitter, then rand(count, 2) for the velocity noise, source after source, each seeing the room the previous ones left.
NumPy's legacy binomial takes sequential inversion while flow * dt <= 30 and BTPE beyond; which branch a case takes is
computed here, not assumed.  tests/test_rng_cases_cpu.py proves that the BTPE cases below, at these seeds and CALLS
calls each, reach every branch of BTPE -- shrinking the sweep fails that test."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

CALLS = 300  # emit calls (binomial draws) per case

# (flow, dt): inversion up to flow * dt = 30 -- 14999 x 0.002 just under it, 15000 x 0.002 exactly on it --, BTPE
# beyond, from just past the switch to n p q = 9900
SWEEP = (
    (1, 0.002), (7000, 0.002), (2000, 0.5), (14999, 0.002), (15000, 0.002),
    (15001, 0.002), (20000, 0.002), (22500, 0.002), (100000, 0.002), (1000, 0.5), (10 ** 6, 0.01),
)


def seed_of(flow: int, dt: float) -> int:
    return 1000 + SWEEP.index((flow, dt))


def takes_btpe(flow: int, dt: float) -> bool:
    """NumPy's legacy `binomial` for p <= 0.5: inversion while p * n <= 30.0, BTPE beyond (the same float product)."""
    return flow * dt > 30.0


def source(flow, *, radius=0.05, position=(0.5, 0.5), velocity=(0.0, 0.0), noise=0.05):
    return SimpleNamespace(radius=radius, position=list(position), velocity=list(velocity), flow=flow, noise=noise)


def mixed_sources(n: int) -> list:
    """`n` sources mixing inversion and BTPE flows (at dt = 0.002), with different radius, position, noise and
    velocity."""
    flows = (7000, 20000, 100, 22500, 15000, 100000, 1, 14999, 30000)
    return [source(flows[k % len(flows)], radius=0.01 + 0.013 * k, position=(0.1 + 0.04 * k, 0.9 - 0.03 * k),
                   velocity=(3.0 - 0.5 * k, 0.25 * k - 1.0), noise=0.002 + 0.011 * k) for k in range(n)]


def numpy_emit(rs: np.random.RandomState, sources, dt: float, stored: int, max_particles: int):
    """One call of the device's emission with NumPy's generator `rs`: -> [(binomial, positions, velocities) per
    source], where positions and velocities are None when the source emitted nothing.  A source whose room is 0 or
    less draws its binomial and no `rand`."""
    out = []
    for s in sources:
        x = int(rs.binomial(s.flow, dt))
        count = min(x, max_particles - stored)
        if count <= 0:
            out.append((x, None, None))
            continue
        jitter = rs.rand(count, 2)
        positions = (jitter - 0.5) * s.radius + np.array(s.position)
        velocities = np.ones_like(positions) * np.array(s.velocity)[None]
        velocities += (rs.rand(count, 2) - 0.5) * s.noise
        out.append((x, positions, velocities))
        stored += count
    return out
