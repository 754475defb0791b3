"""The probe's vocabulary: the names of the sixteen observables the device reduces the state to (sc_probe_now,
sc_probe_enable / sc_probe_read in include/sandcrate_hip.h; the rule is tests/probe_spec.py), and the shapes `Crate`
hands them out in.  This is the single place the names live."""
from __future__ import annotations

import numpy as np

FIELDS = ("tick", "n", "sum_x", "sum_y", "sum_vx", "sum_vy", "sum_ke", "sum_p", "min_x", "max_x", "min_y", "max_y",
          "max_speed2", "max_p", "n_pressed", "n_binned")
MAX_BINS = 1024
MAX_ROWS = 1 << 20


def as_dict(rows, counts=None, tops=None, dropped=None) -> dict:
    """`rows` (16,) or (T, 16) as {name: value or T-long array}, plus `count` / `top` when there are bins and `dropped`
    when given."""
    rows = np.asarray(rows, dtype=np.float64)
    out = {name: (rows[..., k].copy() if rows.ndim > 1 else float(rows[k])) for k, name in enumerate(FIELDS)}
    if counts is not None and counts.shape[-1] > 0:
        out["count"] = counts
        out["top"] = tops
    if dropped is not None:
        out["dropped"] = int(dropped)
    return out


def concatenate(chunks, bins: int = 0) -> dict:
    """Several `Crate.observations()` results, oldest first, as one: arrays joined, `dropped` added up."""
    chunks = list(chunks)
    out = {name: np.concatenate([c[name] for c in chunks]) if chunks else np.zeros(0) for name in FIELDS}
    if bins > 0:
        out["count"] = np.concatenate([c["count"] for c in chunks]) if chunks else np.zeros((0, bins), dtype=np.int32)
        out["top"] = np.concatenate([c["top"] for c in chunks]) if chunks else np.zeros((0, bins))
    out["dropped"] = int(sum(c["dropped"] for c in chunks))
    return out
