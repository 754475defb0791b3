"""The worlds of tests/force_cases.py still mean what they claim (CPU only, on the oracle): the piles give exactly the NaN rows
their lists predict and nothing else ever gives one, the noise clips the share of pairs a case is named for, the graded
cloud has every list length in a block of the tile regime its variant is named for, the clamp acts on half a cloud, one
term moves the particles of a one-term world -- and every world is well-conditioned: one ulp in every position and velocity
leaves the sort, the lists, the contacts and the NaN rows as they are, and moves the outputs the device is compared on by
less than a tenth of the tolerance it is given (rtol 1e-9; atol 1e-12, velocities 1e-11).  tests/test_gpu_force.py asserts
each case's property again before it compares the device with the oracle.

The worst ratio of change to tolerance over the two ticks of the oracle's own run (test_well_conditioned; the cap is 0.1):

    case                                  none    counter    host
    pile_pairs                             0.0223   0.0165   0.0193
    clipped_noise_1                             -   0.0197   0.0229
    clipped_noise_4                             -   0.0143   0.0200
    pressure_clamp_median                  0.0190   0.0135   0.0150
    pressure_clamp_negative                0.0113   0.0152   0.0206
    sparse_ids                                  -   0.0166        -
    floor_pile                             0.0083   0.0117   0.0070
    list_lengths_lds                       0.0114   0.0180   0.0165
    list_lengths_rows                      0.0177   0.0585   0.0340
    list_lengths_table                     0.0675   0.0543   0.0426
    one_term_smoothing                     0.0168   0.0254        -
    one_term_target_minus                  0.0168   0.0149        -
    one_term_target_plus                   0.0168   0.0091        -
    one_term_pressure                      0.0187   0.0134        -
    one_term_pressure_pamp_minus_1         0.0168   0.0090        -
    one_term_viscosity                     0.0197   0.0090        -
    one_term_gravity                       0.0168   0.0090        -
    one_term_corner_pamp_minus_1           0.0239   0.0141        -
    one_term_corner_pamp_0                 0.0168   0.0141        -
    one_term_corner_ss_0                   0.0168   0.0090        -
    one_term_corner_tp_0                   0.0168   0.0090        -
    one_term_corner_viscosity_0            0.0168   0.0144        -
    one_term_corner_viscosity_overshoot    0.0610   0.0206        -
    worst: 0.0675
"""
import numpy as np
import pytest

import force_cases as fc
from oracle.neighbors import strip_sort

CAP = 0.1            # of the tolerance: what one ulp in the inputs may move an output by
CLOSEST = 1e-4       # of d: no listed pair is closer than this after the noise, an exact pile apart


@pytest.fixture(scope="module")
def runs():
    """(case name, noise) -> the oracle's own two ticks [(state, out)], computed once."""
    cache = {}

    def get(name, noise):
        if (name, noise) not in cache:
            cache[name, noise] = fc.oracle_ticks(fc.CASES[name](), noise)
        return cache[name, noise]
    return get


def listed(out):
    return np.arange(out["overlap"].shape[1])[None, :] < out["neighbor_counts"][:, None]


def has_nan(out):
    return any(np.isnan(out[k]).any() for k in ("particles", "velocities", "pressure", "surface_normals"))


# ------------------------------------------------------------------ zero distance
def check_piles(case, state, out):
    """The premise of pile_pairs without noise on one tick's output: -> the NaN rows."""
    n = len(state[2])
    want = fc.nan_rows(case, out, state)
    members = np.isin(state[2], np.concatenate(fc.piles_of(case)))
    assert np.array_equal(np.isnan(out["particles"]).any(axis=1), want)
    assert np.array_equal(np.isnan(out["velocities"]).any(axis=1), want)
    assert members.sum() == sum(fc.PILE_SIZES) and want.sum() > members.sum()   # ... and particles that list a member
    assert want.sum() < 0.1 * n
    assert np.isfinite(out["pressure"]).all()
    assert np.array_equal(np.isnan(out["surface_normals"]).any(axis=1), members)
    # a zero distance only inside a pile, and every other listed pair apart
    zero = (out["pair_distance"] == 0).any(axis=1)
    assert np.array_equal(zero, members)
    assert out["pair_distance"][out["pair_distance"] > 0].min() >= CLOSEST * case.d
    return want


def test_pile_pairs_gives_the_nan_rows_its_lists_predict(runs):
    case = fc.pile_pairs()
    (state, out), (state1, out1) = runs("pile_pairs", "none")
    check_piles(case, state, out)
    counts, table = out["neighbor_counts"], out["neighbor_table"]
    big, three = case.marks["pile25"], case.marks["pile3"]
    assert (counts[big] == 20).all()                                  # cut lists ...
    inside = np.isin(table[big], big).sum(axis=1)
    assert (inside >= 1).all() and (inside == 20).any()               # ... which hold pile members, forward and reverse
    assert fc.asymmetric_entries(counts, table) > 0
    assert (out["wall_count"][three] == 1).all()                      # the pile on the floor
    assert len(state1[2]) == len(state[2]) - fc.nan_rows(case, out, state).sum() and not has_nan(out1)


@pytest.mark.parametrize("name,noise", [p for p in fc.paths() if p != ("pile_pairs", "none")])
def test_nothing_else_gives_a_nan(runs, name, noise):
    """`keep = ~isnan` of the device test hides no row: with noise the piles stay finite, and no other world has a NaN."""
    for state, out in runs(name, noise):
        assert not has_nan(out) and len(state[2]) == len(fc.CASES[name]().p)


# ------------------------------------------------------------------ upper clip
CLIPPED_SHARE = {1: 0.2, 4: 0.6}


def check_clipped(level, out):
    clipped = (out["pair_distance"] >= fc.D)[listed(out)]
    assert clipped.mean() > CLIPPED_SHARE[level]
    assert np.array_equal(out["overlap"][listed(out)] == 0, clipped)
    assert (out["pressure"] > 0).mean() > 0.5                        # ... and enough left for pass B to push with


@pytest.mark.parametrize("noise", ["counter", "host"])
@pytest.mark.parametrize("level", list(CLIPPED_SHARE))
def test_noise_clips_the_share_of_pairs(runs, level, noise):
    for _, out in runs("clipped_noise_%d" % level, noise):
        check_clipped(level, out)


# ------------------------------------------------------------------ list length
def check_list_lengths(regime, out):
    case = fc.list_lengths(regime)
    fx, counts, table = out["fixed_positions"], out["neighbor_counts"], out["neighbor_table"]
    assert np.array_equal(fx, case.p)                                 # nobody touches a wall: the tiles are the ones built
    total, reach = fc.tile_regimes(fx, case.d, counts, table)
    _, order = strip_sort(fx, case.d)
    cloud = np.isin(order, case.marks["cloud"])
    in_regime = np.zeros(len(order), dtype=bool)
    for b in range(len(total)):
        if fc.regime_of(total[b], reach[b]) == regime:
            in_regime[b * fc.tc.TILE:(b + 1) * fc.tc.TILE] = True
    if regime == "lds":
        assert (total <= fc.tc.TILE_CAP_B).all()
    lengths = counts[order[in_regime & cloud]]
    hist = np.bincount(lengths, minlength=21)
    assert (hist > 0).all(), hist.tolist()                            # every length 0 .. 20 (so every residue mod 4) ...
    assert hist[20] >= 50                                             # ... full lists, cut ones among them
    assert fc.asymmetric_entries(counts, table) > 1000


@pytest.mark.parametrize("regime", list(fc.REGIMES))
def test_graded_cloud_has_every_list_length_in_its_tile_regime(runs, regime):
    check_list_lengths(regime, runs("list_lengths_" + regime, "none")[0][1])


# ------------------------------------------------------------------ pressure clamp
def check_clamp(kind, out):
    case = fc.pressure_clamp(kind)
    P, C = out["pressure"], out["neighbor_counts"]
    if kind == "median":
        assert ((P > 0) & (C > 0)).mean() > 0.3 and ((P == 0) & (C > 0)).mean() > 0.3
    else:
        assert case.coef["ignored_pressure"] == -0.5
        lone = case.marks["lone"]
        assert (C[lone] == 0).all() and (P[lone] == 0).all()          # not max(0 - 0 + 0.5, 0)
        assert (out["wall_count"][case.marks["lone_floor"]] == 1).all()
        rest = np.setdiff1d(np.arange(len(P)), lone)
        assert (C[rest] > 0).mean() > 0.95 and (P[rest][C[rest] > 0] >= 0.5).all()


@pytest.mark.parametrize("kind", ["median", "negative"])
def test_pressure_clamp_acts_where_the_case_says(runs, kind):
    check_clamp(kind, runs("pressure_clamp_" + kind, "none")[0][1])


# ------------------------------------------------------------------ one term
def check_one_term(name, state, out):
    case = fc.one_term(name)
    coef = case.coef
    dt = coef["dt"]
    v0 = state[1]
    moved = lambda a, b: np.abs(a - b).max(axis=1) > 0  # noqa: E731
    tension = moved(out["v_after_tension"], v0)
    pressure = moved(out["v_after_pressure"], out["v_after_tension"] + dt * np.asarray(coef["gravity"])[None])
    viscous = moved(out["v_after_viscosity"], out["v_after_pressure"])
    on = {"smoothing": (1, 0, 0), "target_minus": (1, 0, 0), "target_plus": (1, 0, 0), "pressure": (1, 1, 0),
          "viscosity": (0, 0, 1), "gravity": (0, 0, 0)}
    if name in on:
        for phase, want in zip((tension, pressure, viscous), on[name]):
            assert phase.mean() > 0.9 if want else not phase.any(), name
        assert (out["pressure"] > 0).all() if name == "pressure" else (out["pressure"] == 0).all()
        assert bool(np.any(coef["gravity"])) == (name == "gravity")
    if name.endswith("pamp_minus_1"):
        assert dt * (1 + coef["pressure_amplifier"]) == 0.0 and (out["pressure"] > 0).mean() > 0.9
        # tension's pressure part and the pressure phase cancel: what is left of the two is rounding
        both = out["v_after_pressure"] - dt * np.asarray(coef["gravity"])[None] - v0
        if name == "pressure_pamp_minus_1":
            assert tension.mean() > 0.9 and np.abs(both).max() < 1e-13
    if name == "corner_viscosity_overshoot":
        assert dt * coef["viscosity"] * 20 > 1 and (dt * coef["viscosity"] * out["neighbor_counts"] > 1).mean() > 0.9
    for key, value in fc.ONE_TERM[name].items():
        assert coef[key] == value


@pytest.mark.parametrize("name", list(fc.ONE_TERM))
def test_one_term_worlds_move_by_that_term(runs, name):
    state, out = runs("one_term_" + name, "none")[0]
    check_one_term(name, state, out)


# ------------------------------------------------------------------ ids
def check_sparse_ids():
    case = fc.sparse_ids()
    ids = case.ids
    assert ids.min() == 0 and ids.max() == fc.ID_MAX == 2 ** 31 - 2 and (np.diff(ids) > 0).all()
    assert (ids >= 2 ** 16).mean() > 0.99 and (ids >= 2 ** 30).mean() > 0.3      # the top bits are in use
    assert len(np.unique(ids & 0xFFFF)) < len(ids)                                # ... and the low 16 do not tell ids apart
    assert not np.array_equal(case.upload_order, np.arange(len(ids)))
    assert sorted(case.upload_order.tolist()) == list(range(len(ids)))


def test_sparse_ids_span_31_bits():
    check_sparse_ids()


# ------------------------------------------------------------------ walls
def check_floor_pile(out):
    case = fc.floor_pile()
    V, P = out["wall_count"], out["pressure"]
    assert set(V.tolist()) == {0, 1, 2}
    corner = case.marks["corner"][0]
    assert V[corner] == 2 and P[corner] > 0 and (V == 2).sum() == 1
    assert ((V == 1) & (P > 0)).sum() >= 30
    wall_term = np.abs(P[:, None] * out["wall_u"].sum(axis=1)).max(axis=1)   # of dt pamp P U
    assert (wall_term[V > 0] > 0).sum() >= 30 and wall_term[corner] > 0
    bounced = (out["v_after_bounce"] != out["v_after_viscosity"]).any(axis=1)
    assert bounced[V == 1].sum() >= 10 and not bounced[V == 0].any()


def test_floor_pile_touches_bounces_and_is_pushed_by_the_wall(runs):
    check_floor_pile(runs("floor_pile", "none")[0][1])


PREMISES = {}  # case name -> the check of its property on the first tick's (state, out), with the first noise the case has
PREMISES["pile_pairs"] = lambda state, out: check_piles(fc.pile_pairs(), state, out)
PREMISES["floor_pile"] = lambda state, out: check_floor_pile(out)
PREMISES["sparse_ids"] = lambda state, out: check_sparse_ids()
for _level in CLIPPED_SHARE:
    PREMISES["clipped_noise_%d" % _level] = lambda state, out, k=_level: check_clipped(k, out)
for _kind in ("median", "negative"):
    PREMISES["pressure_clamp_" + _kind] = lambda state, out, k=_kind: check_clamp(k, out)
for _regime in fc.REGIMES:
    PREMISES["list_lengths_" + _regime] = lambda state, out, k=_regime: check_list_lengths(k, out)
for _name in fc.ONE_TERM:
    PREMISES["one_term_" + _name] = lambda state, out, k=_name: check_one_term(k, state, out)


# ------------------------------------------------------------------ conditioning
@pytest.mark.parametrize("name,noise", fc.paths())
def test_well_conditioned(runs, name, noise):
    case = fc.CASES[name]()
    worst, same = fc.conditioning(case, noise)
    print(f"{name} {noise}: {worst:.4f}")
    assert same                                  # the sort, the lists, the contacts and the NaN rows
    assert worst < CAP
    members = np.concatenate(fc.piles_of(case)) if fc.piles_of(case) and noise == "none" else np.zeros(0, dtype=np.int64)
    for state, out in runs(name, noise):
        dist = out["pair_distance"]
        exact = np.isin(state[2], case.ids[members])
        assert not (dist[~exact] == 0).any()
        assert dist[dist > 0].min() >= CLOSEST * case.d
