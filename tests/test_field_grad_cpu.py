"""CPU tests of the rule and the cases of the weighted sums' gradients: every case of tests/field_grad_cases.py has the
property it is named for; `position_grad` of tests/field_grad_spec.py and the swapped `field` equal torch's own autograd
(CPU, float64) of a dense all-pairs formulation on every well-conditioned case, within a bound that is derived, not
chosen; the chunked form with one group is the rule; the header, the ctypes row and the kernels agree.

The bound.  Both routes compute, per row, k * sum_j s_rj m_rj dx_rj with s a sum of 2 + 2C addends at most, each term a
few roundings on top -- sequentially here, in torch's order there.  To first order a sum of p terms is off by at most
(p - 1) 2^-53 times the sum of the terms' absolute values whatever the order, each term carries at most 2C + 2 roundings
from s and about six from d2, t, m and the products, k one more, and both routes round: so
    |spec - dense| <= (partners_r + 2C + 16) 2^-53 |k| sum_j S_rj m_rj |dx_rj|,   S_rj = |row_s| + |part_s| + sum_c |row_a part_b|
with the addends of s in absolute value, which covers cancellation inside s.  The values' gradient has the like bound over
sum |w G|.  (Measured with the rule alone: the worst error is 0.27 of the bound.)"""
import re
from pathlib import Path

import numpy as np
import pytest

import field_cases as FK
import field_grad_cases as GK
import field_grad_spec as GS
import field_spec as FS
from sand_crate_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent
EPS = 2.0 ** -53
INSIDE = [name for name in GK.cases() if name not in GK.OUTSIDE]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def near_the_radius(case):
    """Is there a pair with |d2 - r2| <= 1e-9 r2?"""
    p = case.points
    q = p if case.queries is None else case.queries
    r2 = np.float64(case.radius) ** 2
    with np.errstate(all="ignore"):
        d2 = (q[:, None, 0] - p[None, :, 0]) ** 2 + (q[:, None, 1] - p[None, :, 1]) ** 2
    return bool((np.abs(d2 - r2) <= 1e-9 * r2).any())


def well_conditioned(name):
    case = GK.cases()[name]
    arrays = [a for a in (case.points, case.queries, case.values, case.G, case.gw) if a is not None]
    return all(np.isfinite(a).all() for a in arrays) and (name in GK.AT_THE_RADIUS or not near_the_radius(case))


def dense_grads(case):
    """torch's autograd of the all-pairs formulation, float64 on the CPU -> the dict of `field_grad_cases.grads_of`."""
    import torch
    P = torch.tensor(np.array(case.points), dtype=torch.float64, requires_grad=True)
    Q = P if case.queries is None else torch.tensor(np.array(case.queries), dtype=torch.float64, requires_grad=True)
    V = GK.values_of(case)
    V = None if V is None else torch.tensor(np.array(V), dtype=torch.float64, requires_grad=True)
    r2 = float(np.float64(case.radius) ** 2)
    dx, dy = Q[:, None, 0] - P[None, :, 0], Q[:, None, 1] - P[None, :, 1]
    d2 = dx * dx + dy * dy
    mask = d2.detach() <= r2
    if case.queries is None and not case.include_self:
        mask &= ~torch.eye(len(P), dtype=torch.bool)
    t = 1.0 - d2 / r2
    w = torch.where(mask, t ** case.power if case.power else torch.ones_like(t), torch.zeros_like(t))
    loss = torch.zeros((), dtype=torch.float64)
    if V is not None and case.G is not None:
        loss = loss + (torch.tensor(np.array(GK.two_dimensional(case.G))) * (w @ V)).sum()
    if case.gw is not None:
        loss = loss + (torch.tensor(np.array(case.gw)) * w.sum(dim=1)).sum()
    if not loss.requires_grad:
        return {}
    loss.backward()
    out = {"points": P}
    if case.queries is not None:
        out["queries"] = Q
    if V is not None and case.G is not None:
        out["values"] = V
    return {key: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.numpy() for key, t in out.items()}


def position_bound(case, use):
    rows_xy, pts, a, b, row_s, part_s, self_form = use
    q = pts if self_form else rows_xy
    C = 0 if case.values is None else GK.two_dimensional(case.values).shape[1]
    r2 = np.float64(case.radius) ** 2
    k = abs(2.0 * case.power / r2)
    out = np.zeros((len(q), 2))
    for r, (js, d2) in enumerate(FS.partners_of(pts, case.radius, False, None if self_form else q)):
        S = np.zeros(len(js))
        if row_s is not None:
            S += abs(row_s[r])
        if part_s is not None:
            S += np.abs(part_s[js])
        if a is not None:
            S += np.abs(a[r][None, :] * b[js]).sum(axis=1)
        m = FS.weights(d2, r2, case.power - 1)
        for axis in range(2):
            out[r, axis] = (len(js) + 2 * C + 16) * EPS * k * (S * m * np.abs(q[r, axis] - pts[js, axis])).sum()
    return out


def values_bound(case):
    G = GK.two_dimensional(case.G)
    C = G.shape[1]
    r2 = np.float64(case.radius) ** 2
    if case.queries is None:
        partners = FS.partners_of(case.points, case.radius, case.include_self)
    else:
        partners = FS.partners_of(case.queries, case.radius, True, case.points)
    out = np.zeros((len(case.points), C))
    for r, (js, d2) in enumerate(partners):
        w = FS.weights(d2, r2, case.power)
        out[r] = (len(js) + 2 * C + 16) * EPS * (w[:, None] * np.abs(G[js])).sum(axis=0)
    return out


# ---- 1. the cases

def test_every_case_has_the_property_it_is_named_for():
    cases = GK.cases()
    assert set(GK.TAKEN) <= set(cases) and all(name in FK.cases() for name in GK.TAKEN)
    for name, case in cases.items():
        rows = GK.rows_of(case)
        assert case.gw is None or case.gw.shape == (rows,)
        if case.G is not None:
            assert GK.two_dimensional(case.G).shape == (rows, GK.two_dimensional(case.values).shape[1])
    # the upstream gradients span decades, so the order of a sum shows
    gw = np.abs(cases[GK.ORDER].gw)
    assert gw.max() / gw[gw > 0].min() > 1e8
    row0 = FS.partners_of(cases[GK.ORDER].points, cases[GK.ORDER].radius, False)[0][0]
    assert len(row0) == 108 and not (np.diff(row0) < 0).any()
    for name in GK.PILE:                                                            # coincident: every dx is 0
        assert cases[name].power == int(name[-1]) and (cases[name].points == cases[name].points[0]).all()
    for name in GK.AT_THE_RADIUS:                                                   # d2 == r2 exactly: t = 0
        case = cases[name]
        js, d2 = FS.partners_of(case.points, case.radius, False)[0]
        assert case.power == int(name[-1]) and list(js) == [1] and d2[0] == case.radius ** 2
    for name, case in cases.items():
        if name.startswith(GK.COINCIDENT):
            rows = FS.partners_of(case.points, case.radius, False)
            assert any((d2 == 0).any() and (d2 > 0).any() for _, d2 in rows)
    assert len(FS.partners_of(cases["isolated_self_0"].points, cases["isolated_self_0"].radius, False)[0][0]) == 0
    assert [len(cases[name].points) for name in GK.SMALL] == [0, 1, 2]
    for name in ("non_finite", "non_finite_p1"):
        assert not np.isfinite(cases[name].points).all()
    assert not np.isfinite(cases["values_not_finite"].values).all()
    assert not np.isfinite(cases["query_not_finite_p3"].queries).all() and cases["query_not_finite_p3"].power == 3
    assert [GK.rows_of(cases[name]) for name in GK.ROWS] == list(FK.ROWS) * 2
    assert all(cases[name].queries is None for name in GK.ROWS[:6]) and all(cases[name].queries is not None for name in GK.ROWS[6:])
    # the widths: in the self form the dot product has twice the channels -- every kernel guarded and unguarded, and one,
    # two, three and five groups
    widths = [cases[name].values.shape[1] for name in GK.WIDTHS]
    assert widths == list(range(1, 10)) + [17]
    doubled = [2 * w for w in widths]
    assert {N.fields_kernel_channels(min(w, 8)) for w in doubled} == {2, 4, 8}
    assert {-(-w // 8) for w in doubled} == {1, 2, 3, 5}
    assert {N.fields_kernel_channels(cases[name].values.shape[1]) for name in ("channels_1", "queries_63", "query_on_a_point")} == {1, 2}
    assert all(cases[name].values is None and cases[name].G is None and cases[name].gw is not None for name in GK.ONLY_GW)
    assert all(cases[name].gw is None and cases[name].G is not None for name in GK.NO_GW)
    assert cases["no_G"].G is None and cases["no_G"].values is not None
    assert {cases[name].include_self for name in (GK.ORDER, GK.ORDER + "_with_self")} == {False, True}
    for name in GK.OUTSIDE:
        assert not FS.in_domain(cases[name].points, cases[name].radius, cases[name].queries)
    assert all(FS.in_domain(cases[name].points, cases[name].radius, cases[name].queries) for name in INSIDE)


def test_the_order_of_the_sum_shows_in_the_bits():
    case = GK.cases()[GK.ORDER]
    want = GK.grads_of(case)["points"]
    back = GK.Case(case.points[::-1], case.radius, case.values[::-1], case.power, case.include_self, None, case.G[::-1],
                   case.gw[::-1])
    assert bits(GK.grads_of(back)["points"][::-1]) != bits(want)                     # descending j: other bits
    np.testing.assert_allclose(GK.grads_of(back)["points"][::-1], want, rtol=1e-6, atol=1e-3 * np.abs(want).max())


def test_include_self_plays_no_part_in_the_position_gradient():
    case = GK.cases()[GK.ORDER]
    a = GK.grads_of(case)["points"]
    b = GK.grads_of(case._replace(include_self=not case.include_self))["points"]
    assert bits(a) == bits(b)
    assert bits(GK.grads_of(case)["values"]) != bits(GK.grads_of(case._replace(include_self=True))["values"])


def test_power_0_and_rows_without_partners():
    for name in ("power_0", "pile_70_p0", "partner_count"):
        grads = GK.spec(name)
        assert bits(grads["points"]) == bits(np.zeros_like(grads["points"]))        # +0.0 everywhere
    grads = GK.spec("isolated_self_0")
    assert (grads["points"][0] == 0).all()
    case = GK.cases()["non_finite"]
    grads = GK.grads_of(case)
    bad = ~np.isfinite(case.points).all(axis=1)
    assert bad.any() and (grads["points"][bad] == 0).all() and np.isfinite(grads["points"]).all()
    assert (grads["values"][bad] == 0).all()                                        # ... gives and gets nothing, both sides
    for name in GK.PILE[1:]:                                                        # dx = dy = 0: a zero gradient
        assert (GK.spec(name)["points"] == 0).all()
    case = GK.cases()["at_the_radius_p1"]                                           # m = 1 at t = 0: the one-sided value
    assert (GK.grads_of(case)["points"] != 0).all()
    for name in ("at_the_radius_p2", "at_the_radius_p3"):
        assert (GK.spec(name)["points"] == 0).all()


# ---- 2. the rule against torch's autograd of the dense formulation

@pytest.mark.parametrize("name", [name for name in INSIDE if well_conditioned(name)])
def test_rule_equals_dense_autograd_within_the_derived_bound(name):
    case = GK.cases()[name]
    want, got = dense_grads(case), GK.spec(name)
    assert set(got) <= set(want) or not want
    worst = 0.0
    for key, use in GK.uses(case).items():
        bound = position_bound(case, use)
        err = np.abs(got[key] - want[key]) if want else np.abs(got[key])
        assert (err <= bound).all(), (key, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    if "values" in got:
        bound = values_bound(case)
        err = np.abs(got["values"] - want["values"])
        assert (err <= bound).all(), ("values", float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{name}: worst position error {worst:.3f} of the bound")


def test_the_well_conditioned_cases_are_most_of_them():
    names = [name for name in INSIDE if well_conditioned(name)]
    assert len(names) >= 45 and set(GK.AT_THE_RADIUS) <= set(names) and GK.ORDER in names and "long_rows" in names


# ---- 3. the chunked form, the binding and the header

@pytest.mark.parametrize("name", ["channels_3", "queries_65", "density", "channels_17"])
def test_chunked_with_one_group_is_the_rule(name):
    case = GK.cases()[name]
    with np.errstate(all="ignore"):
        for rows_xy, pts, a, b, row_s, part_s, self_form in GK.uses(case).values():
            whole = GS.position_grad(rows_xy, pts, case.radius, case.power, a, b, row_s, part_s, self_form)
            one = GS.position_grad_chunked(rows_xy, pts, case.radius, case.power, a, b, row_s, part_s, self_form, group=10 ** 6)
            assert bits(whole) == bits(one)
            eights = GS.position_grad_chunked(rows_xy, pts, case.radius, case.power, a, b, row_s, part_s, self_form)
            if a is not None and a.shape[1] > GS.GROUP:
                assert bits(eights) != bits(whole)                                  # the groups round differently
                np.testing.assert_allclose(eights, whole, rtol=1e-6, atol=1e-9 * np.abs(whole).max())
            else:
                assert bits(eights) == bits(whole)


def test_the_binding_mirrors_the_header_and_the_kernels():
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    kernels = (ROOT / "sand_crate_amd" / "csrc" / "sc_fields_grad.h").read_text()
    host = (ROOT / "sand_crate_amd" / "csrc" / "sc_host_state.h").read_text()
    assert "int sc_pairs_sum_grad_device(sc_ctx* ctx," in header and "#define SC_ABI_VERSION 5" in header
    declaration = header[header.index("int sc_pairs_sum_grad_device(sc_ctx* ctx,"):]
    declaration = re.sub(r"/\*.*?\*/", "", declaration[:declaration.index(";")], flags=re.S)
    params = [p.strip() for p in declaration[declaration.index("(") + 1:declaration.rindex(")")].split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == [
        "ctx", "dev_queries", "n_queries", "dev_row_a", "row_a_rows", "dev_part_b", "part_b_rows", "channels", "dev_row_s",
        "dev_part_s", "power", "dev_grad", "room_rows", "dev_counts"]
    res, args = N.SIGNATURES["sc_pairs_sum_grad_device"]
    assert len(args) == len(params) == 14
    import ctypes as C
    for p, a in zip(params, args):
        want = C.c_void_p if "*" in p else C.c_int64 if p.startswith("int64_t") else C.c_int32
        assert a is want or (want is C.c_void_p and a is N._P), (p, a)
    assert GS.GROUP == N.FIELDS_MAX_CHANNELS
    assert all(f"fields_grad_launch<{c}>" in host for c in N.FIELDS_KERNEL_CHANNELS)
    assert "atomicAdd" not in kernels and "__syncthreads" not in kernels             # an OR on the flag is the only atomic
    assert '#include "sc_fields_grad.h"' in (ROOT / "sand_crate_amd" / "csrc" / "sandcrate_hip.hip").read_text()
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "field_function" in (ROOT / doc).read_text()
