"""The probe's rule in plain NumPy (sc_probe_now / sc_probe_read, `Crate.measure` / `Crate.observations`): what the
device reduces a state to.  Nothing here imports the product; tests/test_gpu_probe.py holds the GPU to it.

`row(xy, vxy, pressure, tick)` is sixteen float64 values over the particles `sc_download_state` returns.  Particles whose
x is not finite are skipped by the rule of the library's owned count, |x| < 1e300 (a NaN fails it too):

     0 tick         ticks finished by the context when the state was measured
     1 n            live particles
     2..5           sum_x, sum_y, sum_vx, sum_vy: plain sums
     6 sum_ke       sum of 0.5 * (vx * vx + vy * vy)
     7 sum_p        sum of the pressures (zeros where the download gives zeros, e.g. right after an upload)
     8..11          min_x, max_x, min_y, max_y; +inf / -inf for an empty crate
    12 max_speed2   max of vx * vx + vy * vy over the set and 0
    13 max_p        max pressure over the set and 0
    14 n_pressed    particles with pressure > 0
    15 n_binned     particles that fell into a bin of the profile (0 without bins)

`profile(xy, n_bins, x0, x1)` is (count int32[n_bins], top float64[n_bins]): the bin width is w = (x1 - x0) / n_bins, taken
once in float64; a particle's bin is k = floor((x - x0) / w), the same operations in the same order, and it takes part when
0 <= k < n_bins; top[k] is the smallest y in bin k -- gravity points to +y, so that is the free surface -- and +inf for an
empty bin.

A particle with a NaN velocity (or pressure, or y) at a finite x counts, and its NaN propagates as NumPy's sum, min and
max propagate it: into the sums, minima and maxima its NaN takes part in.  A NaN y takes no part in `top`.

Exactness.  Counts, minima and maxima do not depend on the order of the particles.  max_speed2 is exact because the
device evaluates vx * vx + vy * vy as two products and a sum, each rounded (no fused multiply-add), which also makes the
terms of sum_ke NumPy's bit for bit.  So every field and both profile arrays are compared for equality -- except the six
sums, whose value depends on the order of summation.  For those:

    any order of summing n float64 terms lies within gamma_n * sum|term| of the exact sum, gamma_n ~ n * 2^-53;
    two such sums, the device's and NumPy's, therefore differ by at most twice that;
    a further factor 2 covers the second-order part of gamma_n (n u / (1 - n u) against n u).

    tolerance = 4 * n * 2^-53 * fsum(|term|)

There is no other tolerance."""
import math

import numpy as np

FIELDS = ("tick", "n", "sum_x", "sum_y", "sum_vx", "sum_vy", "sum_ke", "sum_p", "min_x", "max_x", "min_y", "max_y",
          "max_speed2", "max_p", "n_pressed", "n_binned")
SUMS = ("sum_x", "sum_y", "sum_vx", "sum_vy", "sum_ke", "sum_p")
MAX_BINS = 1024


def _arrays(xy, vxy, pressure):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    vxy = np.asarray(vxy, dtype=np.float64).reshape(-1, 2)
    pressure = np.zeros(len(xy)) if pressure is None else np.asarray(pressure, dtype=np.float64).reshape(-1)
    assert len(xy) == len(vxy) == len(pressure)
    with np.errstate(invalid="ignore"):
        live = np.abs(xy[:, 0]) < 1e300
    return xy[live], vxy[live], pressure[live]


def bins_of(x, n_bins, x0, x1):
    """The bin of every x, -1 where it takes part in none."""
    x = np.asarray(x, dtype=np.float64)
    if n_bins <= 0:
        return np.full(len(x), -1, dtype=np.int64)
    w = (np.float64(x1) - np.float64(x0)) / np.float64(n_bins)
    with np.errstate(all="ignore"):
        k = np.floor((x - np.float64(x0)) / w)
        inside = (k >= 0) & (k < n_bins)
    return np.where(inside, k, -1).astype(np.int64)


def profile(xy, n_bins, x0, x1):
    xy, _, _ = _arrays(xy, np.zeros_like(np.asarray(xy, dtype=np.float64).reshape(-1, 2)), None)
    count = np.zeros(n_bins, dtype=np.int32)
    top = np.full(n_bins, np.inf)
    k = bins_of(xy[:, 0], n_bins, x0, x1)
    inside = k >= 0
    np.add.at(count, k[inside], 1)
    with_y = inside & ~np.isnan(xy[:, 1])
    np.minimum.at(top, k[with_y], xy[with_y, 1])
    return count, top


def terms(xy, vxy, pressure):
    """The terms of the six sums, by name."""
    xy, vxy, p = _arrays(xy, vxy, pressure)
    with np.errstate(all="ignore"):
        speed2 = vxy[:, 0] * vxy[:, 0] + vxy[:, 1] * vxy[:, 1]
        return {"sum_x": xy[:, 0], "sum_y": xy[:, 1], "sum_vx": vxy[:, 0], "sum_vy": vxy[:, 1], "sum_ke": 0.5 * speed2,
                "sum_p": p}


def tolerances(xy, vxy, pressure):
    """4 n 2^-53 fsum(|term|) for each of the six sums (see the module's docstring)."""
    out = {}
    for name, t in terms(xy, vxy, pressure).items():
        out[name] = 4.0 * len(t) * 2.0 ** -53 * math.fsum(np.abs(t).tolist()) if len(t) else 0.0
    return out


def row(xy, vxy, pressure, tick, n_bins=0, x0=0.0, x1=1.0):
    xy, vxy, p = _arrays(xy, vxy, pressure)
    t = terms(xy, vxy, p)
    out = np.zeros(len(FIELDS))
    with np.errstate(all="ignore"):
        out[0] = tick
        out[1] = len(xy)
        for k, name in enumerate(SUMS):
            out[2 + k] = np.sum(t[name])
        out[8] = np.min(xy[:, 0], initial=np.inf)
        out[9] = np.max(xy[:, 0], initial=-np.inf)
        out[10] = np.min(xy[:, 1], initial=np.inf)
        out[11] = np.max(xy[:, 1], initial=-np.inf)
        out[12] = np.max(vxy[:, 0] * vxy[:, 0] + vxy[:, 1] * vxy[:, 1], initial=0.0)
        out[13] = np.max(p, initial=0.0)
        out[14] = np.count_nonzero(p > 0)
        out[15] = np.count_nonzero(bins_of(xy[:, 0], n_bins, x0, x1) >= 0)
    return out


def as_dict(r):
    return {name: float(r[k]) for k, name in enumerate(FIELDS)}


def compare_row(got, xy, vxy, pressure, tick, n_bins=0, x0=0.0, x1=1.0, want=None):
    """Raises unless `got` (16 values, FIELDS' order) is the row of this state: the sums within their tolerance, every
    other field equal (a NaN equal to a NaN)."""
    got = np.asarray(got, dtype=np.float64).reshape(len(FIELDS))
    want = row(xy, vxy, pressure, tick, n_bins, x0, x1) if want is None else np.asarray(want, dtype=np.float64)
    tol = tolerances(xy, vxy, pressure)
    for k, name in enumerate(FIELDS):
        g, w = float(got[k]), float(want[k])
        if name in SUMS:
            if math.isnan(w) or math.isinf(w):
                ok = (math.isnan(g) and math.isnan(w)) or g == w
            else:
                ok = abs(g - w) <= tol[name]
            assert ok, f"{name}: {g!r} against {w!r}, off by {abs(g - w)!r}, tolerance {tol[name]!r}"
        else:
            assert g == w or (math.isnan(g) and math.isnan(w)), f"{name}: {g!r} against {w!r}"
