"""CPU tests of the weighted sums' rule and cases: tests/field_spec.py is the sequential sum over the rows of
tests/pairs_spec.py; every case of tests/field_cases.py has the property it is named for -- above all, the order-matters
case changes bits when summed in the order the device's walk meets the partners --; 0 <= t <= 1 for every partner; the
torch helpers of `sand_crate_amd.pairs`; the binding's constants and the header agree."""
import re
from pathlib import Path

import numpy as np
import pytest

import field_cases as FK
import field_spec as FS
import nearest_cases as NK
import pairs_spec as S
from sand_crate_amd import _native as N

ROOT = Path(__file__).resolve().parent.parent


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def loop_sum(ws, vs):
    """The rule as a plain Python loop over float64 scalars: -> (out (C,), wsum)."""
    wsum = np.float64(0.0)
    out = np.zeros(vs.shape[1], dtype=np.float64)
    with np.errstate(all="ignore"):
        for w, v in zip(ws, vs):
            wsum = wsum + w
            for c in range(len(out)):
                out[c] = out[c] + w * v[c]
    return out, wsum


def two_dimensional(case):
    v = case.values
    return None if v is None else v.reshape(len(case.points), -1 if v.ndim == 1 else v.shape[1])


# ---- 1. the spec

def test_cumsum_adds_left_to_right():
    rs = np.random.RandomState(1)
    terms = rs.randn(500, 3) * 10.0 ** rs.randint(-8, 9, size=(500, 1))
    acc = np.zeros(3)
    for row in terms:
        acc = acc + row
    assert bits(FS.sequential(terms)) == bits(acc)
    assert bits(FS.sequential(terms)) != bits(terms.sum(axis=0)) or bits(FS.sequential(terms[::-1])) != bits(acc)
    assert bits(FS.sequential(np.zeros((0, 2)))) == bits(np.zeros(2))
    assert not np.signbit(FS.sequential(np.array([-0.0])))                          # from +0.0: 0.0 + -0.0 is +0.0


@pytest.mark.parametrize("name", [FK.ORDER, "long_rows_p0", "non_finite_p1", "lattice_0.25_p2", "channels_5", "pile_70_p3"])
def test_spec_is_the_sequential_sum_over_the_pair_list(name):
    case = FK.cases()[name]
    values = two_dimensional(case)
    offsets, partners, d2 = S.pairs(case.points, case.radius)
    out, wsum = FS.field(case.points, case.radius, values, case.power, False)
    r2 = np.float64(case.radius) * np.float64(case.radius)
    for r in range(len(case.points)):
        js = partners[offsets[r]:offsets[r + 1]]
        ws = FS.weights(d2[offsets[r]:offsets[r + 1]], r2, case.power)
        want = loop_sum(ws, values[js])
        assert bits(out[r]) == bits(want[0]) and bits(wsum[r]) == bits(want[1])


def test_include_self_puts_the_point_in_its_place_in_index_order():
    case = FK.cases()[FK.ORDER]
    without = FS.partners_of(case.points, case.radius, False)
    with_self = FS.partners_of(case.points, case.radius, True)
    for r, ((js, _), (ks, d2)) in enumerate(zip(without, with_self)):
        assert ks.tolist() == sorted(js.tolist() + [r]) and d2[ks.tolist().index(r)] == 0.0
    queries = case.points[:5]
    for include_self in (True, False):                                              # with queries it means nothing
        got = FS.partners_of(case.points, case.radius, include_self, queries)
        assert all(a[0].tolist() == b[0].tolist() for a, b in zip(got, with_self[:5]))


@pytest.mark.parametrize("name", list(FK.cases()))
def test_every_partner_has_t_in_0_1(name):
    case = FK.cases()[name]
    r2 = np.float64(case.radius) * np.float64(case.radius)
    for js, d2 in FS.partners_of(case.points, case.radius, case.include_self, case.queries):
        t = np.float64(1.0) - d2 / r2
        assert ((0.0 <= t) & (t <= 1.0)).all()
        for power in range(4):
            w = FS.weights(d2, r2, power)
            assert ((0.0 <= w) & (w <= 1.0)).all()


# ---- 2. the cases

def test_the_order_matters():
    case = FK.cases()[FK.ORDER]
    assert case.power == 3 and not case.include_self
    arrival = NK.arrival(case.points, case.radius, case.points[0], self_index=0)
    js, d2 = FS.partners_of(case.points, case.radius, False)[0]
    assert len(js) == 108 and sorted(arrival) == js.tolist() and arrival != js.tolist()
    r2 = np.float64(case.radius) * np.float64(case.radius)
    w = dict(zip(js.tolist(), FS.weights(d2, r2, 3)))
    rule = FS.field(case.points, case.radius, case.values, 3, False)
    assert bits(rule[0][0]) == bits(loop_sum([w[j] for j in js.tolist()], case.values[js])[0])
    walked = loop_sum([w[j] for j in arrival], case.values[arrival])
    assert bits(walked[1]) != bits(rule[1][0])                                      # wsum[0] in the walk's order
    assert all(bits(walked[0][c]) != bits(rule[0][0, c]) for c in range(case.values.shape[1]))   # ... and every channel
    exponents = np.floor(np.log10(np.abs(case.values[js]).max(axis=1)))
    assert exponents.max() - exponents.min() >= 12                                  # magnitudes far apart in one row


def test_named_properties():
    cases = FK.cases()
    for power in range(4):
        case = cases[f"pile_70_p{power}"]
        rows = FS.partners_of(case.points, case.radius, case.include_self)
        assert all((d2 == 0).all() and len(js) == 70 - (not case.include_self) for js, d2 in rows)
        out, wsum = FS.field(*case[:5])
        assert (wsum == 70 - (not case.include_self)).all()                         # every w is 1
        case = cases[f"at_the_radius_p{power}"]
        (js, d2), _ = FS.partners_of(case.points, case.radius, False)
        assert js.tolist() == [1] and d2[0] == np.float64(case.radius) ** 2
        out, wsum = FS.field(*case[:5])
        assert wsum[0] == (1.0 if power == 0 else 0.0) and (out[0] == (case.values[1] if power == 0 else 0.0)).all()
        with np.errstate(all="ignore"):
            out, wsum = FS.field(*cases[f"at_the_radius_inf_p{power}"][:5])
        assert np.isinf(out[0, 0]) if power == 0 else np.isnan(out[0, 0])           # 0 * inf
        assert out[0, 1] == (-2.0 if power == 0 else 0.0)
    lone, bare = cases["isolated_self_1"], cases["isolated_self_0"]
    assert FS.partners_of(lone.points, lone.radius, True)[0][0].tolist() == [0]
    assert FS.partners_of(bare.points, bare.radius, False)[0][0].tolist() == []
    out, wsum = FS.field(*lone[:5])
    assert wsum[0] == 1.0 and bits(out[0]) == bits(lone.values[0])
    out, wsum = FS.field(*bare[:5])
    assert wsum[0] == 0.0 and bits(out[0]) == bits(np.zeros(1))
    assert [len(cases[f"rows_{n}"].points) for n in FK.ROWS] == list(FK.ROWS) == [63, 64, 65, 255, 256, 257]
    assert [len(cases[f"queries_{n}"].queries) for n in FK.ROWS] == list(FK.ROWS)
    assert sorted({N.fields_kernel_channels(cases[f"channels_{w}"].values.shape[1]) for w in FK.WIDTHS if w <= 8}) == [1, 2, 4, 8]
    assert cases["one_dimensional"].values.ndim == 1 and cases["density"].values is None
    assert len(cases["n_0_p0"].points) == 0 and len(cases["n_1_p1"].points) == 1 and len(cases["q_0"].queries) == 0
    for name, case in cases.items():
        assert FS.in_domain(case.points, case.radius, case.queries) == (name not in FK.OUTSIDE), name
        assert max(len(case.points), 0 if case.queries is None else len(case.queries)) <= 5000
    assert FS.in_domain(cases[FK.OUTSIDE[1]].points, cases[FK.OUTSIDE[1]].radius)   # the query is what lies outside


def test_rows_that_are_not_finite_and_values_that_are_not():
    case = FK.cases()["query_not_finite"]
    out, wsum = FS.field(case.points, case.radius, two_dimensional(case), case.power, case.include_self, case.queries)
    dead = ~np.isfinite(case.queries).all(axis=1)
    assert dead.sum() == 4 and (wsum[dead] == 0).all() and (out[dead] == 0).all() and (wsum[~dead] > 0).any()
    case = FK.cases()["non_finite_p1"]
    out, wsum = FS.field(*case[:5])
    dead = ~np.isfinite(case.points).all(axis=1)
    assert dead.sum() == 60 and (wsum[dead] == 0).all() and (out[dead] == 0).all()
    rows = FS.partners_of(case.points, case.radius, case.include_self)
    assert not set(np.concatenate([js for js, _ in rows]).tolist()) & set(np.nonzero(dead)[0].tolist())
    case = FK.cases()["values_not_finite"]
    out, wsum = FS.field(*case[:5])
    assert np.isnan(out).any() and np.isinf(out).any() and np.isfinite(out).any() and np.isfinite(wsum).all()


# ---- 3. the helpers

def test_normalized():
    import torch
    from sand_crate_amd import pairs
    sums = torch.tensor([[2.0, -4.0], [0.0, 0.0], [3.0, 9.0]], dtype=torch.float64)
    wsum = torch.tensor([4.0, 0.0, 3.0], dtype=torch.float64)
    assert pairs.normalized(sums, wsum).tolist() == [[0.5, -1.0], [0.0, 0.0], [1.0, 3.0]]
    assert pairs.normalized(sums[:, 0], wsum).tolist() == [0.5, 0.0, 1.0]
    assert pairs.normalized(sums[:0], wsum[:0]).shape == (0, 2)


def test_grid_queries():
    import torch
    from sand_crate_amd import pairs
    q = pairs.grid_queries(0.0, 4.0, 10.0, 16.0, 4, 3)
    assert q.dtype == torch.float64 and q.shape == (12, 2)
    assert q[:, 0].tolist() == [0.5, 1.5, 2.5, 3.5] * 3                              # x runs fastest: row-major
    assert q[:, 1].tolist() == [11.0] * 4 + [13.0] * 4 + [15.0] * 4
    assert q.reshape(3, 4, 2)[2, 1].tolist() == [1.5, 15.0]
    assert pairs.grid_queries(0.0, 1.0, 0.0, 1.0, 0, 5).shape == (0, 2)
    assert pairs.grid_queries(0.0, 1.0, 0.0, 1.0, 1, 1).tolist() == [[0.5, 0.5]]
    with pytest.raises(ValueError):
        pairs.grid_queries(0.0, 1.0, 0.0, 1.0, -1, 1)


# ---- 4. the binding and the header

def test_the_binding_mirrors_the_header_and_the_kernels():
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    kernels = (ROOT / "sand_crate_amd" / "csrc" / "sc_fields.h").read_text()
    assert re.search(r"enum \{ SC_FIELDS_MAX_CHANNELS = (\d+), SC_FIELDS_SELF = (\d+) \};", header).groups() == (
        str(N.FIELDS_MAX_CHANNELS), str(N.FIELDS_SELF))
    assert f"kFieldsMaxChannels = {N.FIELDS_MAX_CHANNELS};" in kernels
    assert "int sc_pairs_sum_device(sc_ctx* ctx," in header and "#define SC_ABI_VERSION 5" in header
    res, args = N.SIGNATURES["sc_pairs_sum_device"]
    assert len(args) == 12
    assert [N.fields_kernel_channels(c) for c in range(9)] == [1, 1, 2, 4, 4, 8, 8, 8, 8]
    assert all(f"fields_launch<{c}>" in (ROOT / "sand_crate_amd" / "csrc" / "sc_host_state.h").read_text()
               for c in N.FIELDS_KERNEL_CHANNELS)
    with pytest.raises(ValueError):
        N.fields_kernel_channels(9)
    assert "atomicAdd" not in kernels                                               # an OR on the flag is the only atomic
