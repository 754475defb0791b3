"""Every world of tests/slab_cases.py is what it claims to be -- columns, wall counts, fixes along the slab axis, spans,
who is whose neighbor after the fix, by the oracle alone -- and the product's slab logic (`SlabChain` over the oracle
backend, which takes the decisions of the HIP path: pack rule, kept band, reach check) either equals the single domain bit
for bit or reports the fix that went too far.  No tolerances: equality, or the named error."""
import numpy as np
import pytest

import slab_cases as sc_cases
from slab_cases import CASES, CROSSED, D, EQUAL, HALO, R, REACH
from slab_oracle_backend import OracleSlabBackend, SlabCrossedError, SlabReachError

AXES = ("x", "y")


# ------------------------------------------------------------------ helpers
def premises(case, axis="x"):
    """What the oracle says of the world before anything moves: per particle the column before and after the hard wall
    fix, the wall count, the fix along the slab axis in units of d, and the neighbor sets after the fix."""
    from oracle.neighbors import as_python_lists, neighbor_lists
    from oracle.scene import OracleCrate
    from oracle.tick import hard_wall_fix, wall_contacts
    from oracle.world import World
    bodies, coef, p, v = case.world(axis)
    orc = OracleCrate(World(bodies, [], coef))
    a = 1 if axis == "y" else 0
    V, u, _ = wall_contacts(p, orc.segments, orc.body_states(), R)
    fixed = hard_wall_fix(p, V, u, R)
    counts, table = neighbor_lists(fixed, D)
    return dict(p=p, v=v, before=p[:, a], after=fixed[:, a], col=np.floor(p[:, a] / D).astype(np.int64),
                col_after=np.floor(fixed[:, a] / D).astype(np.int64), walls=V, fix=(fixed[:, a] - p[:, a]) / D,
                neighbors=[set(l) for l in as_python_lists(counts, table)])


def describe(case, pr, names=None):
    m = case.marks
    names = names or list(m)
    return "; ".join(f"{n}: col {pr['col'][m[n]]}->{pr['col_after'][m[n]]} walls {pr['walls'][m[n]]} fix {pr['fix'][m[n]]:+.3f} d"
                     for n in names)


def oracle_chain(case, axis, noise, reach_check=True):
    from sand_crate_amd.load_config import WorldConfig
    from sand_crate_amd.slab import SlabChain
    bodies, coef, p, v = case.world(axis)

    def backend(k):
        b = OracleSlabBackend(halo_capacity=len(p), noise=noise, noise_seed=9)
        b.reach_check = reach_check
        return b
    return SlabChain(WorldConfig(bodies, [], coef), p, v, case.n_slabs, noise=noise, noise_seed=9, cuts=case.cuts,
                     backend_factory=backend, axis=axis, rebalance_every=case.rebalance_every, overlap=False)


def single_tick(case, axis, noise, p, v, ids, t):
    from oracle.scene import OracleCrate
    from oracle.tick import counter_noise_key, counter_noise_u01, remove_outside, tick_core
    from oracle.world import World
    bodies, coef, _, _ = case.world(axis)
    orc = OracleCrate(World(bodies, [], coef))
    p, v, ids = remove_outside(p, v, R, ids)
    eta = None if noise == "none" else counter_noise_u01(ids, counter_noise_key(9, t))
    out = tick_core(p, v, orc.segments, orc.body_states(), orc.coef, eta_u01=eta)
    return out["particles"], out["velocities"], out["pressure"], ids


def run_against_single(case, axis, noise, ticks, reach_check=True):
    """Tick by tick; the single domain restarts every tick from the chain's state.  -> first mismatch as text, or None"""
    chain = oracle_chain(case, axis, noise, reach_check)
    _, _, p, v = case.world(axis)
    ids = np.arange(len(p))
    for t in range(ticks):
        chain.run(1)
        chain.synchronize()
        sp, sv, spr, sids = single_tick(case, axis, noise, p, v, ids, t)
        gp, gv, gpr, gids = chain.gather_state()
        if not np.array_equal(gids, sids):
            return f"tick {t}: ids differ ({len(gids)} vs {len(sids)})"
        for name, g, s in (("velocities", gv, sv), ("positions", gp, sp), ("pressure", gpr, spr)):
            if not np.array_equal(g, s):
                bad = np.flatnonzero((g != s).reshape(len(g), -1).any(1))
                k = int(bad[0])
                return f"tick {t}: {name} differ for ids {gids[bad].tolist()}: id {gids[k]} chain {g[k]} single {s[k]}"
        p, v, ids = gp, gv, gids
    return None


# ------------------------------------------------------------------ the worlds are what they claim
def senders(case, col):
    """Per particle: how many slabs own it, and to how many left / right neighbors its owner's pack rule sends it."""
    bounds = [-2 ** 40] + list(case.cuts) + [2 ** 40]
    own = np.zeros(len(col), int)
    to_left, to_right = np.zeros(len(col), int), np.zeros(len(col), int)
    for k in range(case.n_slabs):
        lo, hi = bounds[k], bounds[k + 1]
        mine = (col >= lo) & (col < hi)
        own += mine
        if k > 0:
            to_left += mine & (col < lo + HALO)
        if k < case.n_slabs - 1:
            to_right += mine & (col >= hi - HALO)
    return own, to_left, to_right


@pytest.mark.parametrize("axis", AXES)
def test_on_the_cut_premises(axis):
    case = CASES["on_the_cut"]()
    pr, m = premises(case, axis), case.marks
    d, inv = D, 1.0 / D
    x = {n: pr["before"][k] for n, k in m.items()}
    assert x["at"] == 12 * d and x["below"] == np.nextafter(x["at"], 0) and x["above"] == np.nextafter(x["at"], 1)
    assert [int(np.floor(x[n] / d)) for n in ("below", "at", "above")] == [11, 12, 12]
    assert [int(np.floor(x[n] / d)) for n in ("band_below", "band_at", "band_above")] == [8, 9, 9]
    # the product floors differently just below either edge: floor_div must take its fallback there
    assert np.floor(x["below"] * inv) == 12 and np.floor(x["band_below"] * inv) == 9
    own, to_left, _ = senders(case, pr["col"])
    assert (own == 1).all()
    assert [int(to_left[m[n]]) for n in ("band_below", "band_at", "band_above", "below", "at")] == [0, 0, 0, 0, 1]
    assert (pr["walls"] == 0).all()
    for n, k in m.items():
        assert {k + 1, k + 2} <= pr["neighbors"][k]
    print(describe(case, pr))


@pytest.mark.parametrize("axis", AXES)
def test_band_edges_premises(axis):
    case = CASES["band_edges"]()
    pr, m = premises(case, axis), case.marks
    assert (pr["walls"] == 0).all()
    assert [int(pr["col"][m[f"right_{w}"]]) for w in "ijklm"] == [9, 10, 11, 12, 13]
    assert [int(pr["col"][m[f"left_{w}"]]) for w in "ijklm"] == [10, 9, 8, 7, 6]
    for side in ("right", "left"):
        i, j, k, l, mm = (m[f"{side}_{w}"] for w in "ijklm")
        assert pr["neighbors"][i] == {j} and pr["neighbors"][j] == {i, k} and pr["neighbors"][k] == {j, l}
        assert pr["neighbors"][l] == {k, mm}
        assert abs(pr["before"][k] - pr["before"][i]) < 2 * D < abs(pr["before"][l] - pr["before"][i])
    print(describe(case, pr))


@pytest.mark.parametrize("axis", AXES)
def test_single_contact_reach_premises(axis):
    case = CASES["single_contact_reach"]()
    pr, m = premises(case, axis), case.marks
    for side, cols in (("right", [9, 11, 12]), ("left", [10, 8, 7])):
        i, j, k = (m[f"{side}_{w}"] for w in "ijk")
        assert [int(pr["col"][q]) for q in (i, j, k)] == cols
        assert [int(pr["walls"][q]) for q in (i, j, k)] == [1, 0, 1]
        assert 0.48 < abs(pr["fix"][i]) < 0.5 and 0.48 < abs(pr["fix"][k]) < 0.5 and pr["fix"][i] * pr["fix"][k] < 0
        span = abs(pr["before"][k] - pr["before"][i]) / D
        assert 2.96 < span < 3.0 and abs(pr["after"][k] - pr["after"][i]) < 2 * D
        assert pr["neighbors"][j] == {i, k}
        print(side, "span", span, "d")
    print(describe(case, pr))


def due_reports(case, pr):
    """The rule of the wall pass, restated from its derivation on the premises: (particle, owning slab, arm) of every owned
    particle whose fix exceeds r and that is put beyond (edge + 0.5 - 0.01) d on its way out of its slab ("out"), or comes
    from the fourth column or beyond to less than (2.5 + 0.01) d from an edge it shares ("in")."""
    bounds = [-2 ** 40] + list(case.cuts) + [2 ** 40]
    out = set()
    for q in range(len(pr["col"])):
        s = int(np.searchsorted(case.cuts, pr["col"][q], side="right"))
        lo, hi, f, a, col = bounds[s], bounds[s + 1], pr["fix"][q], pr["after"][q] / D, pr["col"][q]
        if f > 0.5 and s < case.n_slabs - 1:
            out |= {(q, s, "out")} if a > hi + 0.49 else set()
            out |= {(q, s, "in")} if col < hi - HALO and a > hi - HALO + 0.49 else set()
        if f < -0.5 and s > 0:
            out |= {(q, s, "out")} if a < lo - 0.49 else set()
            out |= {(q, s, "in")} if col >= lo + HALO and a < lo + HALO - 0.49 else set()
    return out


JOINT_WORLDS = {  # name: wall counts of i, j, k; columns before; positions after in d (lower bound, upper bound); k a neighbor of j
    "joint_reach": ([2, 0, 2], [9, 11, 13], [(10.88, 10.90), (11.84, 11.84), (12.78, 12.80)], True),
    "joint_reach_one_side": ([2, 0, 1], [9, 11, 13], [(10.88, 10.90), (11.84, 11.84), (12.78, 12.80)], True),
    "missed_one_reports": ([1, 0, 2], [9, 11, 13], [(10.43, 10.45), (11.39, 11.39), (12.33, 12.35)], True),
    "joint_reach_not_neighbors": ([2, 0, 2], [9, 11, 13], [(10.88, 10.90), (11.84, 11.84), (13.08, 13.10)], False),
    "out_just_over": ([2, 0, 2], [9, 11, 13], [(10.50, 10.52), (11.84, 11.84), (12.78, 12.80)], True),
    "out_just_under": ([2, 0, 2], [9, 11, 13], [(10.46, 10.48), (11.84, 11.84), (12.78, 12.80)], True),
    "in_just_under": ([1, 0, 2], [9, 11, 13], [(10.43, 10.45), (11.39, 11.39), (12.48, 12.50)], False),
    "in_just_over": ([1, 0, 2], [9, 11, 13], [(10.43, 10.45), (11.39, 11.39), (12.52, 12.54)], False),
    "joint_lands_short": ([2, 0, 2], [9, 11, 13], [(10.28, 10.30), (11.84, 11.84), (12.78, 12.80)], True),
    "joint_inside_window": ([2, 0, 2], [3, 5, 7], [(4.88, 4.90), (5.84, 5.84), (6.78, 6.80)], True),
    "joint_outside_window": ([2, 0, 2], [2, 4, 6], [(3.88, 3.90), (4.84, 4.84), (5.78, 5.80)], True),
}
JOINT_NAMES = list(JOINT_WORLDS) + [n + "_mirrored" for n in JOINT_WORLDS if n + "_mirrored" in CASES]


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", JOINT_NAMES)
def test_joint_premises(axis, name):
    case = CASES[name]()
    mirrored = name.endswith("_mirrored")
    walls, cols, after, k_is_neighbor = JOINT_WORLDS[name[:-len("_mirrored")] if mirrored else name]
    pr, m = premises(case, axis), case.marks
    i, j, k = m["i"], m["j"], m["k"]
    flip = (lambda x: 20 - x) if mirrored else (lambda x: x)
    assert [int(pr["walls"][q]) for q in (i, j, k)] == walls
    assert [int(pr["col"][q]) for q in (i, j, k)] == ([19 - c for c in cols] if mirrored else cols)
    for q, (lo, hi) in zip((i, j, k), after):
        assert min(flip(lo), flip(hi)) - 1e-9 <= pr["after"][q] / D <= max(flip(lo), flip(hi)) + 1e-9, (q, pr["after"][q] / D)
    assert (k in pr["neighbors"][j]) == k_is_neighbor
    span = abs(pr["before"][k] - pr["before"][i]) / D
    assert span > 3
    # which particle is due to be reported, and by which slab: the case says so, and the rule's derivation agrees
    assert due_reports(case, pr) == {(m[who], slab, arm) for who, slab, arm in case.raisers}
    assert (case.expect == EQUAL) == (not case.raisers)
    chain = oracle_chain(case, axis, "none")
    chain.run(1)
    assert [mem.backend.reach_flag for mem in chain.members] == [any(s == n for _, s, _ in case.raisers) for n in range(case.n_slabs)]
    print(name, "span %.2f d;" % span, describe(case, pr), "; reports:", case.raisers)


def test_joint_reach_is_the_reported_reproduction():
    case = CASES["joint_reach"]()
    pr = premises(case)
    assert np.array_equal(pr["before"][:3], [0.4995, 0.592, 0.6845]) and pr["walls"][:3].tolist() == [2, 0, 2]
    assert 0.5444 < pr["after"][0] < 0.5446 and pr["after"][1] == 0.592 and 0.6394 < pr["after"][2] < 0.6396


@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name,start,end,through", [("migrant_across_a_slab", 5, 15, 1), ("migrant_across_a_slab_mirrored", 14, 4, 1)])
def test_migrant_across_a_slab_premises(axis, name, start, end, through):
    case = CASES[name]()
    pr = premises(case, axis)
    bodies, coef, p, v = case.world(axis)
    a = 1 if axis == "y" else 0
    q = case.marks["runner"]
    assert case.cuts == [6, 14] and (pr["walls"] == 0).all() and not pr["neighbors"][q]
    assert int(pr["col"][q]) == start and int(np.floor((p[q, a] + v[q, a] * coef["dt"]) / D)) == end
    owner = lambda c: int(np.searchsorted(case.cuts, c, side="right"))  # noqa: E731
    assert abs(owner(end) - owner(start)) == 2 and through == 1
    chain = oracle_chain(case, axis, "none")
    chain.run(1)
    assert sum(chain.owned_counts()) == len(p) and not any(mem.backend.crossed_flag for mem in chain.members)
    chain.run(1)
    assert [mem.backend.crossed_flag for mem in chain.members] == [False, True, False]  # the slab it crossed reports
    assert sum(chain.owned_counts()) == len(p) - 1  # (what the report is about)


@pytest.mark.parametrize("axis", AXES)
def test_thin_slab_premises(axis):
    case = CASES["thin_slab"]()
    pr = premises(case, axis)
    assert case.cuts == [6, 14] and case.cuts[1] - case.cuts[0] == 2 * HALO + 2
    assert set(range(1, 19)) <= set(pr["col"].tolist()) and (pr["walls"] == 0).all() and len(pr["col"]) < 300
    own, to_left, to_right = senders(case, pr["col"])
    assert (own == 1).all() and (to_left + to_right <= 1).all()        # a ghost of one neighbor at most
    middle = (pr["col"] >= 6) & (pr["col"] < 14)
    assert to_left[middle].sum() >= 9 and to_right[middle].sum() >= 9    # both bands of the thin slab are in use
    assert (to_left + to_right)[middle & (pr["col"] >= 9) & (pr["col"] < 11)].sum() == 0
    assert min(len(s) for s, c in zip(pr["neighbors"], pr["col"]) if 2 <= c <= 17) >= 2


@pytest.mark.parametrize("axis", AXES)
def test_migrants_premises(axis):
    case = CASES["migrants"]()
    pr, m = premises(case, axis), case.marks
    bodies, coef, p, v = case.world(axis)
    a = 1 if axis == "y" else 0
    assert (pr["walls"] == 0).all()
    for n in (1, 3, 4, 5):
        for side, start, sign in (("right", 9, 1), ("left", 10, -1)):
            k = m[f"{side}_{n}"]
            assert int(pr["col"][k]) == start and len(pr["neighbors"][k]) == 0
            # (the forces of one tick change the landing point by << 1 column: every migrant starts mid-column)
            assert int(np.floor((p[k, a] + v[k, a] * coef["dt"]) / D)) == start + sign * n
    print(describe(case, pr))


@pytest.mark.parametrize("axis", AXES)
def test_ghost_pushed_out_premises(axis):
    case = CASES["ghost_pushed_out"]()
    pr, m = premises(case, axis), case.marks
    g = m["ghost"]
    assert int(pr["walls"][g]) == 3 and 1.34 < pr["fix"][g] < 1.36
    assert int(pr["col"][g]) == 10 + HALO - 1            # slab 0's last band column ...
    assert int(pr["col_after"][g]) == 10 + HALO + 1      # ... and beyond the slack column 13 of its local grid
    assert [int(pr["walls"][m[n]]) for n in ("i", "j", "lands_beside")] == [0, 0, 0]
    assert pr["neighbors"][m["i"]] == {m["j"]} and pr["neighbors"][m["j"]] == {m["i"]}
    assert pr["neighbors"][g] == {m["lands_beside"]}
    print(describe(case, pr))


def test_rebalance_over_a_cluster_premises():
    from sand_crate_amd.slab import rebalanced_cuts
    case = CASES["rebalance_over_a_cluster"]()
    pr = premises(case)
    cluster = (pr["col"] >= 10) & (pr["col"] <= 12)
    assert cluster.sum() >= 48 and (pr["walls"] == 0).all()
    hist = np.bincount(pr["col"] + 4, minlength=28)
    new = rebalanced_cuts(hist, -4, [(-2 ** 40, 10), (10, 2 ** 40)], budget=10 ** 6)
    assert 10 < new[0][1] <= 12  # the cut moves into the cluster


# ------------------------------------------------------------------ the slab logic on these worlds
@pytest.mark.parametrize("ticks", [1, 3])
@pytest.mark.parametrize("noise", ["counter", "none"])
@pytest.mark.parametrize("axis", AXES)
@pytest.mark.parametrize("name", list(CASES))
def test_chain_on_the_oracle_backend(name, axis, noise, ticks):
    case = CASES[name]()
    if case.expect == EQUAL or ticks <= case.first_report_tick:
        assert run_against_single(case, axis, noise, ticks) is None
        return
    with pytest.raises({REACH: SlabReachError, CROSSED: SlabCrossedError}[case.expect], match=sc_cases.MESSAGES[case.expect]):
        run_against_single(case, axis, noise, ticks)


@pytest.mark.parametrize("axis", AXES)
def test_without_the_report_joint_reach_is_silently_wrong(axis):
    """The decisions of the code before F_HALO_REACH: the owned particle next to the cut gets another velocity than in the
    single domain (0.0246284 there, 0.0305164 in the chain, along the slab axis), and nothing says so."""
    for name in ("joint_reach", "joint_reach_one_side", "missed_one_reports"):
        for mirrored in ("", "_mirrored"):
            case = CASES[name + mirrored]()
            what = run_against_single(case, axis, "none", 1, reach_check=False)
            assert what is not None and what.startswith("tick 0: velocities differ for ids [0]"), what
            print(name + mirrored, axis, what)


@pytest.mark.parametrize("axis", AXES)
def test_the_report_can_be_needless(axis):
    """The check judges a particle by the fix it got; the neighbor lists do not exist yet.  Where k ends up nobody's
    neighbor the chain would have equalled the single domain: with the report switched off it does."""
    assert run_against_single(CASES["joint_reach_not_neighbors"](), axis, "counter", 3, reach_check=False) is None


@pytest.mark.parametrize("axis", AXES)
def test_migrants_land_where_they_should(axis):
    case = CASES["migrants"]()
    chain = oracle_chain(case, axis, "none")
    chain.run(1)
    gp, _, _, gids = chain.gather_state()
    a = 1 if axis == "y" else 0
    col = np.floor(gp[:, a] / D).astype(np.int64)
    for n in (1, 3, 4, 5):
        assert col[case.marks[f"right_{n}"]] == 9 + n and col[case.marks[f"left_{n}"]] == 10 - n
    assert len(gids) == len(case.points) + 2 and chain.owned_counts() == [len(gids) // 2, len(gids) // 2]
    chain.run(1)  # the exchange: every migrant has one owner, on the other side
    assert sum(chain.owned_counts()) == len(gids)
    owners = [set(mem.owned_state()[3].tolist()) for mem in chain.members]
    assert not owners[0] & owners[1]
    for n in (1, 3, 4, 5):
        assert case.marks[f"right_{n}"] in owners[1] and case.marks[f"left_{n}"] in owners[0]


def test_rebalance_moves_the_cut_into_the_cluster():
    case = CASES["rebalance_over_a_cluster"]()
    chain = oracle_chain(case, "x", "counter")
    chain.run(3)
    assert chain.members[0].rebalances >= 1 and 10 < chain.slabs[0][1] <= 12
