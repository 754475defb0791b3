"""The inputs of the tracker's tests (test_track_cpu.py, test_gpu_track.py): coordinates and pressures at the edges of
the packed frame's rules (track_spec.py), the particle counts that reach every plane padding, and the worlds whose
states are captured.  NumPy only."""
import numpy as np

import track_spec as S

# every plane padding (n mod 8), odd u16 tails, the last partial dword, wave (64) and workgroup (256 threads of four
# particles: 1024) of the pack kernel
COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
SEGMENT_COUNTS = (0, 1, 16)
HALF_STEP_KS = 400  # how many codes get their half-step neighbourhood tested


def neighbours(v, k=2):
    """v with its k neighbouring doubles on each side."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def half_step_coordinates() -> np.ndarray:
    """lo + (k + 0.5) * step and its two neighbouring doubles on each side, for HALF_STEP_KS codes k spread over the range
    (both ends and a dense run at the start among them): where rounding the product and the sum separately, fusing them,
    rounding half to even or truncating give different codes."""
    ks = np.unique(np.concatenate([np.arange(0, 64), np.linspace(0, S.CODES - 1, HALF_STEP_KS - 128).astype(np.int64),
                                   np.arange(S.CODES - 64, S.CODES)]))
    return neighbours(S.LO + (ks.astype(np.float64) + 0.5) * S.STEP)


def coordinates() -> np.ndarray:
    lo, hi = S.LO, S.LO + S.SPAN
    edges = [lo, hi, np.nextafter(lo, -np.inf), np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(hi, np.inf),
             lo - S.STEP, lo + S.STEP, hi - S.STEP, hi + S.STEP, 0.0, -0.0, 1.0, 1e300, -1e300, np.nan, np.inf, -np.inf]
    return np.concatenate([np.array(edges, dtype=np.float64), half_step_coordinates()])


def finite_coordinates() -> np.ndarray:
    c = coordinates()
    return c[np.isfinite(c)]


def pressures() -> np.ndarray:
    """k / 255 with both neighbouring doubles for every byte k, negative values, values above 1, NaN and the infinities."""
    k = np.arange(256, dtype=np.float64) / 255.0
    extra = [-1.0, -1e-300, -0.5 / 255.0, -1.0 / 255.0, -254.5 / 255.0, -1e300, 1.0 + 1e-9, 1.5, 256.0 / 255.0, 2.0, 1e300,
             0.5 / 255.0, 254.5 / 255.0, 0.999 / 255.0, np.nan, np.inf, -np.inf]
    return np.concatenate([neighbours(k, 1), np.array(extra, dtype=np.float64)])


def cloud(seed: int, n: int, lo=0.05, hi=0.95, speed=0.1):
    rs = np.random.RandomState(seed)
    return rs.rand(n, 2) * (hi - lo) + lo, (rs.rand(n, 2) - 0.5) * speed


def sparse_ids(seed: int, n: int) -> np.ndarray:
    """n distinct ids, in no order, most above 65,536 and up to 10^6 (that one included when n > 0)."""
    rs = np.random.RandomState(seed)
    ids = rs.choice(np.arange(60_000, 1_000_000), size=n, replace=False).astype(np.int64)
    if n:
        ids[rs.randint(n)] = 1_000_000
    return ids


def walls(n_segments: int) -> np.ndarray:
    """n_segments walls (S x 2 x 2) with coordinates no 16-bit grid holds: they must come back as float64."""
    rs = np.random.RandomState(100 + n_segments)
    return rs.rand(n_segments, 2, 2) * 1.5 - 0.25 + np.pi * 1e-9


def box_bodies():
    """Walls all round the unit square: nothing leaves, nothing is removed."""
    return [{"fixed": {"name": "edge", "segments": [[[0.0, 0.0], [0.0, 1.0]], [[0.0, 0.0], [1.0, 0.0]],
                                                     [[1.0, 0.0], [1.0, 1.0]], [[0.0, 1.0], [1.0, 1.0]]]}}]


def wall_bodies(n_segments: int):
    """One fixed body of n_segments short walls outside the unit square (they touch no particle)."""
    if n_segments == 0:
        return []
    seg = walls(n_segments) * 0.01 - 0.2
    return [{"fixed": {"name": "far", "segments": seg.tolist()}}]
