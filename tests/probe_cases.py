"""Small worlds for the probe (tests/probe_spec.py), as data: positions, velocities and the profile's bins.  Each names the
place where the device's reduction can go wrong.  `cases(block, threads)` takes the two sizes of the probe's launch -- the
threads of a workgroup and of the whole launch -- from the caller, who reads them from the product."""
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np


@dataclass
class Case:
    xy: np.ndarray
    vxy: np.ndarray
    bins: int = 0
    x_range: tuple = (0.0, 1.0)
    tick: bool = False          # measured after one tick of the spread-out wave_machine world (pressures), not as uploaded
    claims: dict = field(default_factory=dict)  # what the CPU test checks of the case itself


def cloud(seed, n, lo=0.02, hi=0.98, speed=0.1):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 2) * (hi - lo) + lo, (rs.rand(n, 2) - 0.5) * speed


def fma(a, b, c):
    """a * b + c rounded once (exact rational arithmetic, then the one rounding of float())."""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def contraction_sensitive(vxy):
    """Which rows' vx * vx + vy * vy changes when a compiler contracts it into a fused multiply-add, either way round."""
    out = np.zeros(len(vxy), dtype=bool)
    for k, (vx, vy) in enumerate(np.asarray(vxy, dtype=np.float64)):
        plain = vx * vx + vy * vy
        out[k] = fma(vx, vx, vy * vy) != plain or fma(vy, vy, vx * vx) != plain
    return out


def contraction_batch():
    """A seeded batch of velocities; about a third of its rows are contraction-sensitive."""
    return (np.random.RandomState(2024).rand(600, 2) - 0.5) * 3.0


def edge_positions(bins, x0, x1):
    """x exactly on x0, on every interior edge x0 + k w, on x1 (outside), one ulp below x1, below x0 and far outside;
    with the bin each falls into by the spec's arithmetic done by hand here (-1: none)."""
    w = (np.float64(x1) - np.float64(x0)) / np.float64(bins)
    xs = [np.float64(x0)] + [np.float64(x0) + k * w for k in range(1, bins)]
    want = [int(np.floor((x - np.float64(x0)) / w)) for x in xs]
    xs += [np.float64(x1), np.nextafter(np.float64(x1), -np.inf), np.nextafter(np.float64(x0), -np.inf),
           np.float64(x0) - 0.01, np.float64(x1) + 4.0, np.float64(-3.0), np.float64(7.5)]
    want += [-1, bins - 1, -1, -1, -1, -1, -1]
    return np.array(xs), np.array(want)


def cases(block: int, threads: int) -> dict:
    out = {}
    out["empty"] = Case(np.zeros((0, 2)), np.zeros((0, 2)), bins=8)
    out["one"] = Case(np.array([[0.3, 0.7]]), np.array([[0.25, -1.5]]), bins=8)
    for n in (63, 64, 65):                                   # one wave and its edges
        out[f"n{n}"] = Case(*cloud(n, n), bins=5)
    for n in (block - 1, block, block + 1):                  # a workgroup and its edges
        out[f"block{n - block:+d}"] = Case(*cloud(n, n), bins=16)
    out["second_turn"] = Case(*cloud(5, threads + 1), bins=64)  # the strided loop's second turn, for one thread

    # every particle in one bin (LDS contention); two share the smallest y, a third is one ulp smaller
    xy, vxy = cloud(11, 3000)
    xy[:, 0] = 0.375 + xy[:, 0] * 0.12                       # bin 3 of 8
    xy[:, 1] = 0.2 + 0.7 * xy[:, 1]
    xy[100, 1] = xy[2100, 1] = 0.1
    xy[1500, 1] = np.nextafter(0.1, -np.inf)
    out["one_bin"] = Case(xy, vxy, bins=8, claims=dict(bin=3, top=float(np.nextafter(0.1, -np.inf))))

    for name, bins, rng in (("edges", 8, (0.0, 1.0)), ("edges_sub_range", 7, (0.25, 0.75))):
        xs, want = edge_positions(bins, *rng)
        ys = np.linspace(0.1, 0.9, len(xs))
        out[name] = Case(np.stack([xs, ys], axis=1), np.zeros((len(xs), 2)), bins=bins, x_range=rng, claims=dict(bins=want))

    out["bins_1"] = Case(*cloud(21, 700, -0.2, 1.2), bins=1)
    out["bins_1024"] = Case(*cloud(22, 3000, -0.1, 1.1), bins=1024)
    out["sub_range"] = Case(*cloud(23, 2000), bins=37, x_range=(0.25, 0.75))
    out["no_bins"] = Case(*cloud(24, 1500), bins=0)

    xy, vxy = cloud(31, 300)
    xy[17, 0] = np.inf                                       # not a particle: skipped everywhere
    out["inf_x"] = Case(xy, vxy, bins=8)
    xy, vxy = cloud(32, 300)
    vxy[40, 0] = np.nan                                      # a particle: counted, binned, and its NaN propagates
    out["nan_velocity"] = Case(xy, vxy, bins=8)

    batch = contraction_batch()
    picked = batch[contraction_sensitive(batch)]             # the maximum is then one of them, whichever it is
    xy, _ = cloud(41, len(picked))
    out["contraction"] = Case(xy, picked, bins=0)

    xy, vxy = cloud(77, 400)                                 # the 400 particles of test_gpu_arrows.py's world, after a tick
    out["after_tick"] = Case(xy, vxy, bins=32, tick=True)
    return out
