"""ctypes binding of include/sandcrate_hip.h.

There is no CPU path: if libsandcrate_hip.so is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "libsandcrate_hip.so"

MAX_NEIGHBORS = 20
MAX_SEGMENTS = 16
MAX_BODIES = 8
NUM_KERNELS = 12
NOISE_NONE, NOISE_HOST, NOISE_COUNTER = 0, 1, 2
ARROWS_OFF, ARROWS_LIST, ARROWS_VELOCITY = 0, 1, 2
MAX_ARROWS = 1 << 20
PROBE_FIELDS = 16
PROBE_MAX_BINS = 1024
PROBE_MAX_ROWS = 1 << 20
PROBE_BLOCK, PROBE_BLOCKS = 1024, 256  # the probe's fixed launch (csrc/sc_probe.h: kProbeBlock, kProbeBlocks)
# the device export's launches (csrc/sc_radix.h, sc_kernels.h, sc_state.h): keys per workgroup of a sorting pass
# (kRadixTile), counts per workgroup of the scan between its two kernels (kScanPerBlock), rows per workgroup of the gather
# (kBlock)
STATE_TILE, STATE_SCAN_BLOCK, STATE_GATHER_BLOCK = 256, 2048, 256
# the pair search's launches and table (csrc/sc_pairs.h, sc_radix.h, sc_kernels.h): rows per workgroup of its row kernels
# (kBlock), keys per workgroup of a pass of the binning sort (kRadixTile, the same sort), entries per workgroup of the scans
# (kScanPerBlock); the hashed table has the smallest power of two of buckets that is at least PAIRS_LOAD per point and
# PAIRS_MIN_BUCKETS, a cell (cx, cy) -- floor(x / h), floor(y / h) as 32-bit words, h = radius * PAIRS_CELL_FACTOR -- lies in
# bucket `pairs_bucket(cx, cy, buckets)`; in the batched form (sc_pairs_set_batch_device) the cloud is a third factor of the
# hash, `pairs_bucket(cx, cy, buckets, cloud)`, and PAIRS_BATCH is the status of offsets that are not in order
PAIRS_BLOCK, PAIRS_SORT_TILE, PAIRS_SCAN_BLOCK = 256, 256, 2048
PAIRS_LOAD, PAIRS_MIN_BUCKETS = 2, 256
PAIRS_HASH_X, PAIRS_HASH_Y, PAIRS_HASH_MIX = 0x9E3779B1, 0x85EBCA77, 0x2C1B3C6D
PAIRS_HASH_CLOUD = 0xC2B2AE3D
PAIRS_DOMAIN, PAIRS_BATCH = -1, -3
PAIRS_CELL_FACTOR = 1.0 + 2.0 ** -20
PAIRS_HALF = 1
# the nearest-k table (csrc/sc_nearest.h): the largest k (SC_NEAREST_MAX_K), the rows per workgroup of its kernel
# (kNearestBlock: one wave, whatever k -- `nearest_width(k)`), and the places per row its LDS holds: the smallest of
# NEAREST_SLOTS that is at least k (`nearest_slots(k)`), each a kernel of its own
NEAREST_MAX_K = 64
NEAREST_BLOCK = 64
NEAREST_SLOTS = (16, 32, 64)
# the weighted sums (csrc/sc_fields.h): the most channels of one call (SC_FIELDS_MAX_CHANNELS), the channels its four
# kernels are made for -- a call runs the smallest that holds its own, `fields_kernel_channels(c)` --, the flag that makes
# a point its own partner (SC_FIELDS_SELF), the rows per workgroup (kBlock) and the status values of counts[1]
FIELDS_MAX_CHANNELS = 8
FIELDS_KERNEL_CHANNELS = (1, 2, 4, 8)
FIELDS_SELF = 1
FIELDS_BLOCK = 256
FIELDS_OK, FIELDS_DOMAIN, FIELDS_VALUES_SHORT = 0, -1, -2
# the per-cluster sums (csrc/sc_cluster_sums.h): the most channels of one call (SC_CLUSTER_SUMS_MAX_CHANNELS), the members
# one work item of a level reduces (kCsumGroup: a wave) and the status values of counts[1]
CLUSTER_SUMS_MAX_CHANNELS = 8
CLUSTER_SUMS_GROUP = 64
CLUSTER_SUMS_DOMAIN, CLUSTER_SUMS_VALUES_SHORT = -1, -2
# the distance histograms (csrc/sc_hist.h): the most bins of one call (SC_HIST_MAX_BINS), the rows per workgroup of its
# kernel (kHistBlock: one wave), the bins its search is made for -- the smallest of HIST_SLOTS that is at least the call's,
# `hist_slots(bins)`, each a kernel of its own -- and the status values of counts[1]
HIST_MAX_BINS = 64
HIST_BLOCK = 64
HIST_SLOTS = (16, 32, 64)
HIST_OK, HIST_DOMAIN = 0, -1
HIST_BATCH_MAX_CELLS = 1 << 24  # clouds x bins of one batched histogram (SC_HIST_BATCH_MAX_CELLS)
# the ray sensors (csrc/sc_rays.h): the most steps -- cells -- a ray may walk (kRayMaxSteps), the lanes of the wave that
# walks a ray (kRayBlock), the steps it takes at a time (kRayWaveSteps), the status values of counts[1] -- PAIRS_RANGE is
# the new one: a ray that would walk more than RAY_MAX_STEPS cells -- and the values of `hit` that are no particle: none,
# and wall s as RAY_WALL - s
RAY_MAX_STEPS = 8192
RAY_BLOCK, RAY_WAVE_STEPS = 64, 7
PAIRS_RANGE = -4
RAY_NONE, RAY_WALL = -1, -2
# the ray paths: the most bounces (SC_RAY_MAX_BOUNCES), and the values of `end` that are no status: every leg hit, a leg
# met nothing, the ray or its next leg is dead; PAIRS_DOMAIN and PAIRS_RANGE are the other two
RAY_MAX_BOUNCES = 15
RAY_END_ALL_HIT, RAY_END_NOTHING, RAY_END_DEAD = 0, 1, 2
ERR_ARG = -1
ERR_HIP = -2
ERR_CAPACITY = -3
ERR_STATE = -4
ERR_DOMAIN = -5
FLAG_SCAN_TIMEOUT = 64  # sc_stats.flags: the tick is abandoned (SC_FLAG_SCAN_TIMEOUT)


class NativeError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"libsandcrate_hip: {message} (code {code})")
        self.code = code


class Params(C.Structure):
    _fields_ = [(n, C.c_double) for n in (
        "dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
        "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure", "gravity_x", "gravity_y")]


class Body(C.Structure):
    _fields_ = [("position_x", C.c_double), ("position_y", C.c_double),
                ("center_velocity_x", C.c_double), ("center_velocity_y", C.c_double),
                ("angular_clockwise_velocity", C.c_double), ("n_segments", C.c_int32), ("reserved", C.c_int32)]


class TickInputs(C.Structure):
    _fields_ = [("params", Params), ("segments", C.POINTER(C.c_double)), ("padded", C.POINTER(C.c_double)),
                ("bodies", C.POINTER(Body)), ("n_segments", C.c_int32), ("n_bodies", C.c_int32)]


class Source(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("radius", "position_x", "position_y", "velocity_x", "velocity_y", "noise")] + [
        ("flow", C.c_int64)]


class View(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("zoom", C.c_double), ("center_x", C.c_double),
                ("center_y", C.c_double), ("particle_radius", C.c_double), ("segment_width", C.c_int32),
                ("reserved", C.c_int32)]


class Arrow(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("start_x", "start_y", "end_x", "end_y")]


class Stats(C.Structure):
    _fields_ = [("particles", C.c_int64), ("neighbor_slots", C.c_int64), ("max_neighbors", C.c_int32),
                ("wall_particles", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32)]


_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_I32 = C.POINTER(C.c_int32)

# name -> (restype, argtypes): every symbol include/sandcrate_hip.h declares
SIGNATURES = {
    "sc_last_error": (C.c_char_p, []),
    "sc_abi_version": (C.c_int, []),
    "sc_create": (C.c_int, [C.c_int, C.c_int64, C.POINTER(_P)]),
    "sc_destroy": (C.c_int, [_P]),
    "sc_set_stream": (C.c_int, [_P, _P]),
    "sc_use_own_stream": (C.c_int, [_P]),
    "sc_upload_state": (C.c_int, [_P, _D, _D, C.c_int64]),
    "sc_append_particles": (C.c_int, [_P, _D, _D, C.c_int64]),
    "sc_count": (C.c_int, [_P, _I64]),
    "sc_download_state": (C.c_int, [_P, _D, _D, _D, _I64, C.c_int64, _I64]),
    "sc_set_params": (C.c_int, [_P, C.POINTER(Params)]),
    "sc_set_segments": (C.c_int, [_P, _D, _D, C.c_int32, C.POINTER(Body), C.c_int32]),
    "sc_set_noise_mode": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "sc_set_next_inputs": (C.c_int, [_P, C.POINTER(Params), _D, C.c_int32, C.POINTER(Body), C.c_int32]),
    "sc_step_begin": (C.c_int, [_P]),
    "sc_step_stats": (C.c_int, [_P, C.POINTER(Stats)]),
    "sc_set_noise_host": (C.c_int, [_P, _D, C.c_int64]),
    "sc_step_finish": (C.c_int, [_P]),
    "sc_step": (C.c_int, [_P, C.c_int32]),
    "sc_tick": (C.c_int, [_P, C.POINTER(TickInputs), C.POINTER(TickInputs)]),
    "sc_synchronize": (C.c_int, [_P]),
    "sc_set_scan_patience": (C.c_int, [_P, C.c_int64]),
    "sc_download_sort": (C.c_int, [_P, _I64, _I64, C.c_int64, _I64]),
    "sc_download_neighbors": (C.c_int, [_P, _I64, _I32, _I64, _D, C.c_int64, _I64]),
    "sc_download_normals": (C.c_int, [_P, _D, C.c_int64, _I64]),
    "sc_download_pressure": (C.c_int, [_P, _D, C.c_int64, _I64]),
    "sc_neighbor_search": (C.c_int, [C.c_int, _D, C.c_int64, C.c_double, _I64, _I64, _I32, _I64]),
    "sc_points_to_segments": (C.c_int, [C.c_int, _D, C.c_int64, _D, C.c_int32, _D, _D]),
    "sc_pad_segments": (C.c_int, [_D, C.c_int32, C.c_double, _D]),
    "sc_enable_timing": (C.c_int, [_P, C.c_int]),
    "sc_reset_timing": (C.c_int, [_P]),
    "sc_get_timing": (C.c_int, [_P, _D, _I64]),
    "sc_kernel_name": (C.c_char_p, [C.c_int]),
    "sc_set_slab": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "sc_set_slab_axis": (C.c_int, [_P, C.c_int32]),
    "sc_set_band_flag": (C.c_int, [_P, C.c_int]),
    "sc_upload_state_ids": (C.c_int, [_P, _D, _D, _I64, C.c_int64]),
    "sc_append_particles_ids": (C.c_int, [_P, _D, _D, _I64, C.c_int64]),
    "sc_halo_pack": (C.c_int, [_P, _P, _P, C.c_int64]),
    "sc_halo_sizes": (C.c_int, [_P, C.c_int64, _I64, _I64, _I64, _I64]),
    "sc_halo_unpack": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64]),
    "sc_column_histogram": (C.c_int, [_P, C.c_int64, C.c_int32, _I64]),
    "sc_comm_available": (C.c_int, [C.c_char_p]),
    "sc_comm_unique_id": (C.c_int, [C.c_char_p, _P]),
    "sc_comm_init": (C.c_int, [_P, C.c_char_p, _P, C.c_int32, C.c_int32]),
    "sc_comm_destroy": (C.c_int, [_P]),
    "sc_halo_exchange": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, _P, C.c_int64, _P, C.c_int64, C.c_int32]),
    "sc_owned_count": (C.c_int, [_P, _I64]),
    "sc_set_halo_overlap": (C.c_int, [_P, C.c_int]),
    "sc_side_stream": (C.c_int, [_P, C.POINTER(_P)]),
    "sc_halo_overlap_begin": (C.c_int, [_P, _P]),
    "sc_halo_overlap_end": (C.c_int, [_P]),
    "sc_enable_force_monitor": (C.c_int, [_P, C.c_int]),
    "sc_get_force_monitor": (C.c_int, [_P, _D, _I64]),
    "sc_checkpoint_begin": (C.c_int, [_P]),
    "sc_checkpoint_finish": (C.c_int, [_P, _D, _D, _I64, C.c_int64, _I64, _I64, _I64, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_int32)]),
    "sc_restore_counters": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sc_rng_set_state": (C.c_int, [_P, C.POINTER(C.c_uint32), C.c_int32]),
    "sc_rng_get_state": (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "sc_emit_particles": (C.c_int, [_P, C.POINTER(Source), C.c_int32, C.c_double, C.c_int64]),
    "sc_render": (C.c_int, [_P, C.POINTER(View), _D, C.c_int32, _P]),
    "sc_render_device": (C.c_int, [_P, C.POINTER(View), _D, C.c_int32, _P]),
    "sc_jpeg_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "sc_jpeg_encode_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sc_render_jpeg": (C.c_int, [_P, C.POINTER(View), _D, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sc_gif_bound": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "sc_gif_encode_device": (C.c_int, [_P, _P, C.c_int32, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sc_render_gif": (C.c_int, [_P, C.POINTER(View), _D, C.c_int32, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "sc_set_hud": (C.c_int, [_P, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "sc_set_arrows": (C.c_int, [_P, C.c_int32, C.POINTER(Arrow), C.c_int64, C.c_double, C.c_int64]),
    "sc_probe_now": (C.c_int, [_P, C.c_int32, C.c_double, C.c_double, _D, _I32, _D]),
    "sc_probe_enable": (C.c_int, [_P, C.c_int64, C.c_int32, C.c_double, C.c_double]),
    "sc_probe_disable": (C.c_int, [_P]),
    "sc_probe_read": (C.c_int, [_P, _D, _I32, _D, C.c_int64, _I64, _I64]),
    "sc_track_bound": (C.c_int, [C.c_int64, C.c_int32, _I64]),
    "sc_track_capture": (C.c_int, [_P, _P, C.c_int64, _I64]),
    "sc_track_enable": (C.c_int, [_P, C.c_int64, C.c_int64]),
    "sc_track_disable": (C.c_int, [_P]),
    "sc_track_read": (C.c_int, [_P, _P, C.c_int64, _I64, _I64, _I64]),
    "sc_track_load": (C.c_int, [_P, _P, C.c_int64, C.c_int32]),
    "sc_traj_enable_device": (C.c_int, [_P, _P, _P, _P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32]),
    "sc_traj_capture": (C.c_int, [_P]),
    "sc_traj_disable": (C.c_int, [_P]),
    "sc_export_state_device": (C.c_int, [_P, _P, _P, _P, _P, C.c_int64, _P]),
    "sc_import_state_device": (C.c_int, [_P, _P, _P, _P, C.c_int64]),
    "sc_pairs_count_device": (C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_int32, _P, C.c_int64, _P]),
    "sc_pairs_fill_device": (C.c_int, [_P, _P, _P, C.c_int64]),
    "sc_pairs_set_batch_device": (C.c_int, [_P, _P, C.c_int64]),
    "sc_pairs_set_query_batch_device": (C.c_int, [_P, _P]),
    "sc_pairs_label_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P]),
    "sc_pairs_cluster_sums_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P]),
    "sc_pairs_nearest_device": (C.c_int, [_P, _P, C.c_int64, C.c_int32, _P, _P, _P, C.c_int64, _P]),
    "sc_pairs_sum_device": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _P, _P, C.c_int64,
                                      _P]),
    "sc_pairs_sum_grad_device": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int64, _P, C.c_int64, C.c_int32, _P, _P, C.c_int32,
                                           _P, C.c_int64, _P]),
    "sc_pairs_hist_device": (C.c_int, [_P, _P, C.c_int64, _D, C.c_int32, _P, _P, C.c_int64, _P]),
    "sc_pairs_rays_device": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_double, _D, C.c_int32, _P, _P, C.c_int64, _P]),
    "sc_pairs_ray_paths_device": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_double, C.c_double, _D, C.c_int32, _P, _P,
                                            _P, _P, _P, C.c_int64, _P]),
    # the batched forms: the label's with cluster_ptr before the counts, the histogram's with room_clouds behind room_rows
    "sc_pairs_label_batch_device": (C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_int64, _P, _P]),
    "sc_pairs_hist_batch_device": (C.c_int, [_P, _P, C.c_int64, _D, C.c_int32, _P, _P, C.c_int64, C.c_int64, _P]),
    "sc_pairs_rays_batch_device": (C.c_int, [_P, _P, _P, C.c_int64, C.c_double, C.c_double, _D, C.c_int32, _P, _P, C.c_int64,
                                             _P]),
    "sc_pairs_ray_paths_batch_device": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int32, C.c_double, C.c_double, _D, C.c_int32, _P,
                                                  _P, _P, _P, _P, C.c_int64, _P]),
}


def pairs_buckets(bound: int) -> int:
    """The size of the pair search's hashed table for a host bound of `bound` points."""
    t = PAIRS_MIN_BUCKETS
    while t < PAIRS_LOAD * bound:
        t *= 2
    return t


def pairs_bucket(cx: int, cy: int, buckets: int, cloud: int = 0) -> int:
    """The bucket of cell (cx, cy) -- of cloud `cloud` in the batched form -- in a table of `buckets` buckets
    (csrc/sc_pairs.h: pairs_bucket), in 32-bit arithmetic.  Cloud 0 hashes as an unbatched cell does."""
    m = 0xFFFFFFFF
    v = (((cx & m) * PAIRS_HASH_X) & m) ^ (((cy & m) * PAIRS_HASH_Y) & m) ^ (((cloud & m) * PAIRS_HASH_CLOUD) & m)
    v ^= v >> 15
    v = (v * PAIRS_HASH_MIX) & m
    v ^= v >> 13
    return v & (buckets - 1)


def nearest_slots(k: int) -> int:
    """The places per row in the LDS of the nearest-k kernel that serves a table of k places per row (csrc/sc_nearest.h)."""
    if not 1 <= k <= NEAREST_MAX_K:
        raise ValueError(f"k must be 1 .. {NEAREST_MAX_K}")
    return next(slots for slots in NEAREST_SLOTS if k <= slots)


def nearest_width(k: int) -> int:
    """The rows per workgroup of the nearest-k kernel for a table of k places per row: one wave for every k -- wider
    workgroups for a small k measured slower (profiles/nearest_time.txt)."""
    nearest_slots(k)
    return NEAREST_BLOCK


def fields_kernel_channels(channels: int) -> int:
    """The channels of the sum kernel that serves a call with `channels` channels (csrc/sc_fields.h); 0 runs the first."""
    if not 0 <= channels <= FIELDS_MAX_CHANNELS:
        raise ValueError(f"channels must be 0 .. {FIELDS_MAX_CHANNELS}")
    return next(c for c in FIELDS_KERNEL_CHANNELS if channels <= c)


def hist_slots(bins: int) -> int:
    """The bins per row of the search of the histogram kernel that serves a call with `bins` bins (csrc/sc_hist.h)."""
    if not 1 <= bins <= HIST_MAX_BINS:
        raise ValueError(f"bins must be 1 .. {HIST_MAX_BINS}")
    return next(slots for slots in HIST_SLOTS if bins <= slots)


def hist_squared_edges(edges) -> np.ndarray:
    """The squared edges sc_pairs_hist_device takes, from the B + 1 distances `edges` (tests/hist_spec.py): float64,
    ``e2[k] = edges[k] * edges[k]`` rounded once.  ValueError unless B is 1 .. HIST_MAX_BINS, the edges are finite,
    ``0 <= edges[0] < edges[1] < ...``, and the squares are still strictly ascending and finite (two edges one ulp apart
    may square to the same number, tiny ones to 0)."""
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.shape[0] <= HIST_MAX_BINS + 1:
        raise ValueError(f"edges must be a sequence of B + 1 distances, B 1 .. {HIST_MAX_BINS}")
    if not np.isfinite(e).all() or e[0] < 0 or not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be finite, not negative and strictly ascending")
    with np.errstate(over="ignore", under="ignore"):
        e2 = e * e
    if not np.isfinite(e2).all() or not (e2[1:] > e2[:-1]).all():
        raise ValueError("the squares of the edges must be finite and still strictly ascending")
    return e2


_lib = None


def load():
    """Loads the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise NativeError(-2, f"{LIB_PATH} is missing; build it with `python -m sand_crate_amd.build` "
                                  "(there is no CPU fallback)")
        lib = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        raise NativeError(rc, load().sc_last_error().decode("utf-8", "replace"))


def dptr(a: np.ndarray | None):
    # (ctypes.cast of the raw address: a quarter of `a.ctypes.data_as`'s time, and this runs several times per tick;
    # the caller keeps `a` alive)
    return None if a is None else C.cast(a.__array_interface__["data"][0], _D)


def i64ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(_I64)


def i32ptr(a: np.ndarray | None):
    return None if a is None else a.ctypes.data_as(_I32)


def f64(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float64)
