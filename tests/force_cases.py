"""Worlds in which one rule of the force pair's arithmetic decides the result (tests/test_gpu_force.py,
tests/test_force_cases_cpu.py).

Pass A's pair math (sc_tiled.h: step 4), pass B (pass_b_pairs, pass_b_finish) and pair_offset (sc_kernels.h) hold rules that a
uniform cloud with every force on never isolates:
  zero distance    rsqrt_nr(0) is NaN; fmax(NaN, 0) = 0 gives c = 0, overlap 1 and a finite pressure, while the NaN reaches
                   the normals, the pile's velocities and every particle that lists a pile member (crate.py:174, :270);
  upper clip       c = fmin(.., 1): noise pushes a listed neighbor beyond d; it adds nothing to P or to the normals, but
                   pass B still pushes along it.  Counter noise is folded as ((p_i + 2^31 e) - p_j) - u32 e;
  pressure clamp   P = C ? fmax((C - sum c) - ignored, 0) : 0: the clamp at sum w = ignored, an empty list with a negative
                   ignored_pressure;
  folded weights   k_ss = dt ss, k_pp = dt (1 + pamp), k_0 = -2 tp dt in one sum: each term alone, pamp = -1 (k_pp = 0,
                   where the reference cancels two sums), pamp = 0, ss = 0, tp = 0, viscosity = 0, dt viscosity C > 1;
  list length      nested_slots<0, 20> leaves at the count, the global-memory loop of pass A fetches four neighbors per
                   round trip and pads with `self`: every length 0 .. 20, lists cut at 20 (asymmetric), in a tile that
                   both passes hold in LDS, in one pass B gathers through 12-bit rows, in one of the 32-bit table;
  ids              noise_base casts the id through uint32_t: ids up to 2^31 - 2 with counter noise;
  walls            V = 1 and V = 2, P > 0, the dt pamp P U wall term and the bounce together.
Each builder returns a ForceCase whose inputs sit on the rule.  Where a case does not say otherwise its coefficients are
wall_cases.LIVELY and its walls the closed box.

Everything here is NumPy and the oracle: no device, no reference.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

import tile_cases as tc
import wall_cases as wc

D, R, DT = wc.D, wc.R, wc.DT        # 0.01012: not a power of two
D_LIST = 1.0 / 63                   # the graded cloud's diameter
SEED = 11                           # counter noise: the context's seed
HOST_SEED = 5                       # host noise: the generator the blocks are drawn from
TICKS = 2
PER = 12                            # neighbors per particle of a plain cloud
ID_MAX = 2 ** 31 - 2                # the largest id an upload takes

# the tolerances of the suite (tests/test_gpu_parity.py: test_single_tick_matches_reference): rtol, and atol per output
RTOL = 1e-9
ATOL = {"particles": 1e-12, "velocities": 1e-11, "pressure": 1e-12, "surface_normals": 1e-12}

OFF = dict(pressure_amplifier=0.0, ignored_pressure=1000.0, viscosity=0.0, surface_smoothing=0.0, target_pressure=0.0,
           gravity=[0.0, 0.0])      # no term at all: every pressure is 0 (ignored_pressure above any density)


@dataclass
class ForceCase(wc.Case):
    noises: tuple = ("none", "counter", "host")
    ids: np.ndarray = None          # ascending; None: particle i has id i
    upload_order: np.ndarray = None  # the order the particles are uploaded in (with `ids`)

    def __post_init__(self):
        if self.ids is None:
            self.ids = np.arange(len(self.p), dtype=np.int64)
        for a in (self.p, self.v, self.ids):
            a.setflags(write=False)

    @property
    def d(self):
        return 2 * self.coef["particle_radius"]


def lively(d=D, **changes):
    coef = dict(wc.LIVELY, particle_radius=d / 2, dt=0.002 * d / 0.01)
    coef.update(changes)
    return coef


def patch(rs, n, x0, y0, d=D, per=PER, aspect=1.0):
    """n uniform points in a rectangle at (x0, y0) whose density gives `per` neighbors each; aspect = width / height."""
    area = n * np.pi * d * d / per
    w, h = np.sqrt(area * aspect), np.sqrt(area / aspect)
    return np.column_stack((x0 + rs.rand(n) * w, y0 + rs.rand(n) * h))


def speeds(rs, n, cells_per_tick, d=D):
    return (rs.rand(n, 2) - 0.5) * cells_per_tick * d / (0.002 * d / 0.01)


# ------------------------------------------------------------------ zero distance
PILE_SIZES = (2, 3, 25)


@functools.lru_cache(maxsize=None)
def pile_pairs():
    """A calm cloud that rests on the floor, with piles of 2, 3 and 25 particles at one point each: 25 is more than a full
    list, so the pile's lists are cut (and hold reverse edges); the pile of 3 lies within 1.2 r of the floor."""
    rs = np.random.RandomState(701)
    cloud = patch(rs, 1400, 0.3, 0.35 * R, aspect=2.0)
    spots = np.array([[0.36, 0.11], [0.45, 0.55 * R], [0.53, 0.12]])   # 2 and 25 inside the cloud, 3 on the floor
    far = ((cloud[:, None] - spots[None]) ** 2).sum(2).min(1) > (0.05 * D) ** 2
    cloud = cloud[far]
    p = np.vstack([cloud] + [np.repeat(s[None], k, axis=0) for s, k in zip(spots, PILE_SIZES)])
    p = p[rs.permutation(len(p))]
    piles = [np.flatnonzero((p == s).all(1)) for s in spots]
    assert [len(k) for k in piles] == list(PILE_SIZES)
    return ForceCase("pile_pairs", [wc.BOX], lively(), p, speeds(rs, len(p), 0.2),
                     {"pile%d" % k: idx for k, idx in zip(PILE_SIZES, piles)})


def piles_of(case):
    return [idx for name, idx in sorted(case.marks.items()) if name.startswith("pile")]


# ------------------------------------------------------------------ upper clip
@functools.lru_cache(maxsize=None)
def clipped_noise(level):
    """A cloud whose noise is as large as the diameter (level 1) or four times it (level 4): most listed neighbors are
    pushed beyond d."""
    rs = np.random.RandomState(710 + int(level))
    p = patch(rs, 2000, 0.3, 0.3)
    return ForceCase("clipped_noise_%d" % level, [wc.BOX], lively(collider_noise_level=float(level)), p,
                     speeds(rs, len(p), 1.0), noises=("counter", "host"))


# ------------------------------------------------------------------ list length, in three regimes of the tiled passes
LIST_N = 1500
LIST_ROW = 28                       # the row that holds the ballast
REGIMES = {"lds": 0, "rows": 1300, "table": 4200}   # ballast particles


# lists of 0, 1 and 2 entries at the start of the ballast's row, left of the cloud (cells, row fraction): one alone, a pair,
# a chain of three whose ends are more than d apart
LIST_SHORT = np.array([[4.0, 0.5], [5.5, 0.3], [5.9, 0.7], [7.0, 0.1], [7.55, 0.5], [8.1, 0.1]])


def graded_cloud():
    rs = np.random.RandomState(720)
    u = rs.rand(LIST_N - len(LIST_SHORT))
    graded = np.column_stack((0.2 + 0.6 * u ** 2.2, 0.4 + 0.12 * rs.rand(len(u))))
    return np.vstack((graded, (LIST_SHORT + [0.0, LIST_ROW]) * D_LIST))


def ballast(m):
    """m particles in row LIST_ROW to the right of the cloud (nobody's neighbor there), on a lattice: sorted behind the
    row's cloud particles they lie between the first and the last slot that the lists of the block before them name.
    (41 levels in y: the 20 particles a list holds, the next ones in x, are each at least d / 51 away.)"""
    k = np.arange(m)
    return np.column_stack((0.84 + 0.12 * (k + 0.5) / max(m, 1), (LIST_ROW + 0.1 + 0.8 * ((7 * k) % 41) / 41) * D_LIST))


@functools.lru_cache(maxsize=None)
def list_lengths(regime):
    """The graded cloud x = 0.2 + 0.6 u^2.2 (every list length from 0 to 20, full and cut lists), alone ('lds': every
    tile within kTileCapB) or with a ballast in one row that puts the cloud's blocks around that row into a tile above
    kTileCapB whose reach stays within kRowSlotMax ('rows') or exceeds it ('table').  The ballast is as dense as a pile-up:
    the noise is kept below its spacing and the pressure amplifier low, so that none of it reaches a wall within the
    ticks of a test (particles stopped on a wall share x up to an ulp, and the order inside such a group is ill-conditioned)."""
    rs = np.random.RandomState(721)
    p = np.vstack((graded_cloud(), ballast(REGIMES[regime])))
    v = speeds(rs, len(p), 0.5, D_LIST)
    coef = lively(D_LIST, pressure_amplifier=2.0, collider_noise_level=0.02)
    return ForceCase("list_lengths_" + regime, [wc.BOX], coef, p, v, {"cloud": np.arange(LIST_N)})


def tile_regimes(points, d, counts, table):
    """Per block of the sorted order: (candidate entries, entries its lists reach) -- tile_cases' restated geometry."""
    total = tc.tile_totals(points, d).sum(1)
    reach = tc.reach_total(*tc.list_reach(points, d, counts, table))
    return total, reach


def regime_of(total, reach, cap_a=1100):
    """'lds': both passes hold the tile in LDS.  'rows': pass A searches through the window and runs its four-per-fetch
    pair loop (the reach does not fit the window either), pass B gathers through the 12-bit rows.  'table': the lists go
    to the 32-bit table.  None: another path (a tile trimmed to a reach that LDS holds)."""
    if total <= tc.TILE_CAP_B:
        return "lds"
    if total > cap_a and reach > tc.ROW_SLOT_MAX:
        return "table" if total <= tc.SLOT_MAX else None
    if total > cap_a and reach > cap_a:
        return "rows"
    return None


# ------------------------------------------------------------------ pressure clamp
@functools.lru_cache(maxsize=None)
def pressure_clamp(kind):
    """'median': ignored_pressure is the cloud's median sum of overlaps, so that the clamp acts on half of it.
    'negative': ignored_pressure = -0.5, and lone particles (C = 0: P = 0, not 0.5) beside a crowded cloud, a few of them
    touching the floor, where P enters the wall term."""
    rs = np.random.RandomState(730 + (kind == "negative"))
    p = patch(rs, 1500, 0.3, 0.3)
    if kind == "median":
        case = ForceCase("probe", [wc.BOX], lively(ignored_pressure=0.0, collider_noise_level=0.0), p, np.zeros_like(p))
        ignored = float(np.median(oracle_ticks(case, "none", 1)[0][1]["pressure"]))
        marks = {}
    else:
        ignored = -0.5
        k = np.arange(40)
        lone = np.column_stack((0.1 + 3.0 * D * (k % 20), np.where(k < 20, 1.1 * R, 0.2 + 0.0 * k)))
        p = np.vstack((p, lone))
        marks = {"lone": np.arange(1500, 1540), "lone_floor": np.arange(1500, 1520)}
    return ForceCase("pressure_clamp_" + kind, [wc.BOX], lively(ignored_pressure=ignored), p, speeds(rs, len(p), 1.0), marks)


# ------------------------------------------------------------------ one term at a time, and the corners of the folded weights
ONE_TERM = {
    # zero initial velocities (but for the viscosity) and exactly one term on: the tolerance applies to that term alone
    "smoothing": dict(OFF, surface_smoothing=80.0),
    "target_minus": dict(OFF, target_pressure=-1.0),
    "target_plus": dict(OFF, target_pressure=1.0),
    "pressure": dict(OFF, ignored_pressure=0.2, pressure_amplifier=30.0),
    "pressure_pamp_minus_1": dict(OFF, ignored_pressure=0.2, pressure_amplifier=-1.0),   # k_pp = 0: nothing moves
    "viscosity": dict(OFF, viscosity=4.0),
    "gravity": dict(OFF, gravity=[1.5, -9.8]),
    # every term on and moving particles, one coefficient on a corner
    "corner_pamp_minus_1": dict(pressure_amplifier=-1.0),
    "corner_pamp_0": dict(pressure_amplifier=0.0),
    "corner_ss_0": dict(surface_smoothing=0.0),
    "corner_tp_0": dict(target_pressure=0.0),
    "corner_viscosity_0": dict(viscosity=0.0),
    "corner_viscosity_overshoot": dict(viscosity=400.0),   # dt viscosity 20 = 16 > 1: the viscous step flips the sign
}


@functools.lru_cache(maxsize=None)
def one_term(name):
    rs = np.random.RandomState(740)
    p = patch(rs, 1200, 0.3, 0.3)
    moving = name.startswith("corner") or name == "viscosity"
    v = speeds(rs, len(p), 1.0) if moving else np.zeros_like(p)
    return ForceCase("one_term_" + name, [wc.BOX], lively(**ONE_TERM[name]), p, v, noises=("none", "counter"))


# ------------------------------------------------------------------ ids
@functools.lru_cache(maxsize=None)
def sparse_ids():
    """A cloud whose ids are spread over 0 .. 2^31 - 2 -- both ends among them -- and uploaded in a shuffled order."""
    rs = np.random.RandomState(750)
    p = patch(rs, 1500, 0.3, 0.3)
    special = np.array([0, 3, 65535, 65536, 2 ** 30, ID_MAX - 1, ID_MAX])
    drawn = np.setdiff1d(rs.randint(0, ID_MAX, 2 * len(p)), special)
    ids = np.sort(np.r_[special, rs.permutation(drawn)[:len(p) - len(special)]]).astype(np.int64)
    assert len(np.unique(ids)) == len(p)
    return ForceCase("sparse_ids", [wc.BOX], lively(), p, speeds(rs, len(p), 1.0), noises=("counter",), ids=ids,
                     upload_order=rs.permutation(len(p)))


# ------------------------------------------------------------------ walls
@functools.lru_cache(maxsize=None)
def floor_pile():
    """A lively cloud resting on the floor -- a row of particles within 1.2 r of it (V = 1), under pressure and moving into
    it -- and a group of three in the lower left corner of the box: one within r of both walls (V = 2), one beside it on
    the floor, one above it.  Only the corner particle is on the left wall: two particles of one row that the crossing
    check stops there would share x up to an ulp, and their order -- with it their slots in each other's lists -- would
    hang on the last bit."""
    rs = np.random.RandomState(760)
    cloud = patch(rs, 1400, 0.2, 0.3 * R, aspect=3.0)
    corner = np.array([[0.8 * R, 0.7 * R], [R + 0.8 * D, 0.9 * R], [R + 0.3 * D, R + 0.85 * D]])
    p = np.vstack((cloud, corner))
    v = np.vstack((speeds(rs, len(cloud), 2.0), [[-1.0, -1.5], [0.5, -1.0], [0.5, 0.5]]))
    return ForceCase("floor_pile", [wc.BOX], lively(), p, v, {"corner": np.array([len(cloud)])})


CASES = {"pile_pairs": pile_pairs, "clipped_noise_1": functools.partial(clipped_noise, 1),
         "clipped_noise_4": functools.partial(clipped_noise, 4), "pressure_clamp_median": functools.partial(pressure_clamp, "median"),
         "pressure_clamp_negative": functools.partial(pressure_clamp, "negative"), "sparse_ids": sparse_ids,
         "floor_pile": floor_pile}
CASES.update({"list_lengths_" + k: functools.partial(list_lengths, k) for k in REGIMES})
CASES.update({"one_term_" + k: functools.partial(one_term, k) for k in ONE_TERM})


def paths():
    """(case name, noise) of every run."""
    return [(name, noise) for name, build in CASES.items() for noise in build().noises]


# ------------------------------------------------------------------ the oracle on a case
def coefficients(case, noise):
    coef = dict(case.oracle().coef)
    if noise == "none":
        coef["collider_noise_level"] = 0.0
    return coef


def noise_of(noise, ids, tick, host):
    """tick_core's eta_u01 of one tick: counter noise by id and tick, or the next block of the generator `host`."""
    from oracle.tick import counter_noise_key, counter_noise_u01
    if noise == "none":
        return None
    if noise == "counter":
        return counter_noise_u01(ids, counter_noise_key(SEED, tick))
    return lambda total: host.rand(total, 2)


def oracle_tick(case, noise, tick, state, host, nudge=None):
    """-> (state after removal (p, v, ids), tick_core's output).  nudge: a function (p, v, ids) -> (p, v)."""
    from oracle.tick import remove_outside, tick_core
    orc = case.oracle()
    coef = coefficients(case, noise)
    p, v, ids = remove_outside(state[0], state[1], coef["particle_radius"], state[2])
    if nudge is not None:
        p, v = nudge(p, v, ids)
    with np.errstate(all="ignore"):
        out = tick_core(p, v, orc.segments, orc.body_states(), coef, eta_u01=noise_of(noise, ids, tick, host))
    return (p, v, ids), out


def oracle_ticks(case, noise, ticks=TICKS):
    """The oracle's own run: [(state, out)] per tick, each tick started from the finite rows of the one before."""
    host = np.random.RandomState(HOST_SEED)
    state, runs = (case.p, case.v, case.ids), []
    for t in range(ticks):
        state, out = oracle_tick(case, noise, t, state, host)
        runs.append((state, out))
        keep = ~np.isnan(out["particles"]).any(axis=1)
        state = (out["particles"][keep], out["velocities"][keep], state[2][keep])
    return runs


def nan_rows(case, out, state):
    """The rows a tick without noise leaves NaN, in closed form: the members of a pile, and every particle whose (cut)
    list holds one."""
    ids = state[2]
    members = np.isin(ids, np.concatenate([case.ids[k] for k in piles_of(case)]) if piles_of(case) else [])
    table = out["neighbor_table"]
    lists_one = (members[np.maximum(table, 0)] & (table >= 0)).any(axis=1)
    return members | lists_one


def asymmetric_entries(counts, table):
    """Entries (i, j) of the lists whose reverse (j, i) is in no list."""
    i = np.repeat(np.arange(len(counts)), counts)
    j = table[table >= 0]
    n = len(counts)
    have = set((i * n + j).tolist())
    return int(sum((b * n + a) not in have for a, b in zip(i.tolist(), j.tolist())))


def one_ulp(seed, groups=()):
    """A nudge for oracle_tick: every position and velocity component one ulp up or down, seeded; the particles of a
    group (an exact pile) move together."""
    def nudge(p, v, ids):
        rs = np.random.RandomState(seed)
        sp, sv = rs.randint(0, 2, p.shape) * 2.0 - 1.0, rs.randint(0, 2, v.shape) * 2.0 - 1.0
        for g in groups:
            rows = np.flatnonzero(np.isin(ids, g))
            if len(rows):
                sp[rows], sv[rows] = sp[rows[0]], sv[rows[0]]
        return np.nextafter(p, sp * np.inf), np.nextafter(v, sv * np.inf)
    return nudge


def tick_sensitivity(a, b, d):
    """Two outputs of tick_core for one tick, `b` from inputs one ulp away: -> (the largest change of a compared output in
    units of its tolerance, whether the decisions -- sort, lists, contacts, NaN rows -- are the same)."""
    from oracle.neighbors import strip_sort
    same = np.array_equal(a["neighbor_table"], b["neighbor_table"]) and np.array_equal(a["wall_count"], b["wall_count"])
    same &= all(np.array_equal(x, y) for x, y in zip(strip_sort(a["fixed_positions"], d), strip_sort(b["fixed_positions"], d)))
    worst = 0.0
    for key, atol in ATOL.items():
        x, y = a[key], b[key]
        same &= np.array_equal(np.isnan(x), np.isnan(y))
        fin = ~(np.isnan(x) | np.isnan(y))
        worst = max(worst, float((np.abs(x - y)[fin] / (atol + RTOL * np.abs(x[fin]))).max(initial=0.0)))
    return worst, bool(same)


def conditioning(case, noise, ticks=TICKS):
    """The worst ratio, over the ticks of the oracle's run and the outputs the device is compared on, of the change that
    one ulp in every input makes to the tolerance the device is given -- and whether the decisions (sort, lists,
    contacts, NaN rows) stayed the same.  Measured on the oracle alone."""
    groups = [case.ids[k] for k in piles_of(case)]
    worst, same = 0.0, True
    host_a, host_b = np.random.RandomState(HOST_SEED), np.random.RandomState(HOST_SEED)
    state = (case.p, case.v, case.ids)
    for t in range(ticks):
        st, a = oracle_tick(case, noise, t, state, host_a)
        _, b = oracle_tick(case, noise, t, state, host_b, nudge=one_ulp(1000 + t, groups))
        tick_worst, tick_same = tick_sensitivity(a, b, case.d)
        worst, same = max(worst, tick_worst), same and tick_same
        keep = ~np.isnan(a["particles"]).any(axis=1)
        state = (a["particles"][keep], a["velocities"][keep], st[2][keep])
    return worst, bool(same)
