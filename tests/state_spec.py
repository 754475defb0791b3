"""The rule of the device export (sc_export_state_device; `Engine.export_state`, `Crate.state_tensors`) in NumPy: from the
storage arrays as the device holds them to the arrays the caller receives -- what sc_download_state delivers to the host.

The device stores particles in cell-sorted order, one slot each, with a per-particle id.  `n_stored` slots are in use;
the pressures `P` belong to the first `n_ticked` slots, the ones the last finished tick left live, and only while
`pressure_valid` (no upload since).  No device, no reference."""
from __future__ import annotations

import numpy as np


def export(x, y, vx, vy, P, ids, n_stored, n_ticked, pressure_valid):
    """-> (particles (n, 2), velocities (n, 2), pressure (n,), ids (n,) int64): the stored slots whose x is finite, in
    ascending id order; a slot's pressure is P[slot] below min(n_stored, n_ticked) while the pressures are valid, else 0."""
    slots = np.arange(int(n_stored))
    slots = slots[np.isfinite(np.asarray(x, dtype=np.float64)[slots])]
    slots = slots[np.argsort(np.asarray(ids)[slots], kind="stable")]
    n_pressed = min(int(n_stored), int(n_ticked)) if pressure_valid else 0
    pressure = np.zeros(len(slots))
    pressed = slots < n_pressed
    pressure[pressed] = np.asarray(P, dtype=np.float64)[slots[pressed]]
    col = lambda a, b: np.stack([np.asarray(a, dtype=np.float64)[slots], np.asarray(b, dtype=np.float64)[slots]], axis=1)  # noqa: E731
    return col(x, y), col(vx, vy), pressure, np.asarray(ids)[slots].astype(np.int64)
