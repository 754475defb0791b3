"""GPU tests of the gradients of the device weighted sums (sc_pairs_sum_grad_device, `Engine.pairs_sum_grad`,
`Crate.field_function`): the position gradient equals tests/field_grad_spec.py bit for bit -- every row of every case of
tests/field_grad_cases.py in all three uses of the rule, NaN where the rule has NaN --, two calls give the same bits, rows
past the row count stay untouched, the domain error and short arrays write the status and nothing else, the errors come
back before anything is launched, the workspace of the count is left as it is; `field_function` is `field_tensors` bit
for bit in the forward, state form included, and its backward gives the rule's gradients for values, points and queries,
singly and together; a tick between forward and backward changes nothing; a raster through `pairs.normalized` is
back-propagated to the values and equals torch's dense float64 autograd.

The raster's bound.  values.grad[j] = sum_r w_rj G_r with G_r = target_r / wsum_r: the bound of the values' gradient in
tests/test_field_grad_cpu.py, (Q_j + 2C + 16) 2^-53 sum_r |w_rj G_r| with Q_j the queries that reach point j -- and G_r
itself differs between the two routes by the error of wsum_r, a sum of P_r positive weights (relative error at most
(P_r + 3) 2^-53 on each side) and one division: so the factor is (Q_j + 2 max_r P_r + 2C + 24)."""
import numpy as np
import pytest

import field_cases as FK
import field_grad_cases as GK
import field_grad_spec as GS
import gpu_support as U
import pairs_spec as S
from gpu_support import crate, sc  # noqa: F401

pytestmark = pytest.mark.gpu

CASES = [name for name in GK.cases() if name not in GK.OUTSIDE]
GROUP = GS.GROUP


def groups_of(use):
    """A use of the rule cut into the launches of at most eight channels, the scalars with the first."""
    rows_xy, pts, a, b, row_s, part_s, self_form = use
    if a is None:
        return [use]
    return [(rows_xy, pts, a[:, at:at + GROUP], b[:, at:at + GROUP], row_s if at == 0 else None, part_s if at == 0 else None,
             self_form) for at in range(0, a.shape[1], GROUP)]


def through_the_engine(eng, use, radius, power, *, half=False, spare=8, row_rows=None, part_rows=None):
    """count + gradient of one launch through the engine into a sentinel-filled tensor with `spare` rows of room beyond
    the rows -> (grad, counts), synchronised."""
    import torch
    rows_xy, pts, a, b, row_s, part_s, self_form = use
    dev = torch.device("cuda", eng.device)
    n = len(pts)
    rows = n if self_form else len(rows_xy)
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    grad = U.full((rows + spare, 2), dev, U.SENTINEL_F)
    held = [U.tensor(pts, 2), None if self_form else U.tensor(rows_xy, 2),
            U.tensor(a, None), U.tensor(b, None), U.tensor(row_s, None), U.tensor(part_s, None)]
    eng.pairs_count(held[0], radius=radius, offsets=offsets, counts=counts, half=half)
    assert eng.pairs_sum_grad(grad, held[2], held[3], held[4], held[5], power=power, queries=held[1], counts=out,
                              row_rows=row_rows, part_rows=part_rows) is out
    eng.synchronize()
    return grad, out


def run_function(crate, case, needs, *, weight_sums=None, state=False):
    """`field_function` of a case with `needs` (a subset of "values", "points", "queries") requiring grad, then the
    gradients of the case's upstream G and gw -> (outputs, {name: gradient or None})."""
    import torch
    values = U.tensor(case.values, None, requires_grad="values" in needs)
    points = U.tensor(case.points, 2, requires_grad="points" in needs)
    queries = U.tensor(case.queries, 2, requires_grad="queries" in needs)
    want_wsum = case.gw is not None if weight_sums is None else weight_sums
    out = crate.field_function(values, case.radius, power=case.power, include_self=case.include_self,
                               points=None if state else points, queries=queries, weight_sums=want_wsum)
    inputs = {name: t for name, t in (("values", values), ("points", points), ("queries", queries)) if name in needs}
    pairs = []
    if case.values is not None and case.G is not None:
        G = U.tensor(case.G, None)
        pairs.append((out[0], G.view(-1) if out[0].dim() == 1 else G))
    if case.gw is not None:
        pairs.append((out[-1], U.tensor(case.gw, None)))
    grads = torch.autograd.grad([o for o, _ in pairs], list(inputs.values()), [g for _, g in pairs], allow_unused=True)
    return out, dict(zip(inputs, grads))


def needs_of(case):
    return (("values",) if case.values is not None else ()) + ("points",) + (("queries",) if case.queries is not None else ())


def check_gradients(case, want, grads):
    for name, got in grads.items():
        if name == "values" and "values" not in want:                               # (no G: nothing flows to the values)
            assert got is None
            continue
        rule = want[name]
        if name == "values" and case.values.ndim == 1:
            rule = rule[:, 0]
        if case.power == 0 and name != "values":
            assert got is None or U.same_bits_or_nan(got, rule)
            continue
        assert got is not None and U.same_bits_or_nan(got, rule), name


# ---- 1. the kernel against the rule: every case, every use, every group

@pytest.mark.parametrize("name", CASES)
def test_engine_equals_the_spec(crate, name):
    case = GK.cases()[name]
    for at, (key, use) in enumerate(GK.uses(case).items()):
        rows = len(use[1]) if use[6] else len(use[0])
        total = None
        for group in groups_of(use):
            with np.errstate(all="ignore"):
                want = GS.position_grad(group[0], group[1], case.radius, case.power, *group[2:])
            grad, counts = through_the_engine(crate.engine, group, case.radius, case.power, half=bool(at))
            assert counts.cpu().tolist() == [rows, 0]
            assert U.same_bits_or_nan(grad[:rows], want) and U.untouched(grad[rows:])
            total = grad[:rows] if total is None else total + grad[:rows]
        assert U.same_bits_or_nan(total, GK.spec(name)[key])                        # the groups add up to the chunked rule


def test_two_calls_give_identical_bits(crate):
    case = GK.cases()[GK.ORDER]
    use = GK.uses(case)["points"]
    a, _ = through_the_engine(crate.engine, use, case.radius, case.power)
    other = GK.cases()["queries_257"]
    through_the_engine(crate.engine, GK.uses(other)["queries"], other.radius, other.power)   # another grid in between
    b, _ = through_the_engine(crate.engine, use, case.radius, case.power)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- 2. the status

@pytest.mark.parametrize("name", GK.OUTSIDE)
def test_outside_the_domain_writes_the_status_only(crate, name):
    case = GK.cases()[name]
    for key, use in GK.uses(case).items():
        grad, counts = through_the_engine(crate.engine, use, case.radius, case.power)
        assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(grad)
    with pytest.raises(ValueError, match="domain"):
        run_function(crate, case, needs_of(case))


def test_short_arrays_write_the_status_only(crate):
    case = GK.cases()["queries_65"]
    n, q = len(case.points), len(case.queries)
    for key, (rows, partners) in (("queries", (q, n)), ("points", (n, q))):
        use = GK.uses(case)[key]
        for kw in (dict(row_rows=rows - 1), dict(part_rows=partners - 1)):
            grad, counts = through_the_engine(crate.engine, use, case.radius, case.power, **kw)
            assert counts.cpu().tolist() == [U.SENTINEL, -2] and U.untouched(grad)
        grad, counts = through_the_engine(crate.engine, use, case.radius, case.power, row_rows=rows, part_rows=partners)
        assert counts.cpu().tolist() == [rows, 0] and U.same_bits_or_nan(grad[:rows], GK.spec("queries_65")[key])
    case = GK.cases()["channels_3"]
    n = len(case.points)
    use = GK.uses(case)["points"]
    for kw in (dict(row_rows=n - 1), dict(part_rows=n - 1)):
        grad, counts = through_the_engine(crate.engine, use, case.radius, case.power, **kw)
        assert counts.cpu().tolist() == [U.SENTINEL, -2] and U.untouched(grad)
    # the scalars alone are counted too, and the domain wins over the rows
    only = GK.uses(GK.cases()["density"])["points"]
    grad, counts = through_the_engine(crate.engine, only, case.radius, case.power, part_rows=n - 1)
    assert counts.cpu().tolist() == [U.SENTINEL, -2] and U.untouched(grad)
    outside = GK.cases()[GK.OUTSIDE[1]]
    grad, counts = through_the_engine(crate.engine, GK.uses(outside)["queries"], outside.radius, outside.power,
                                      part_rows=len(outside.points) - 1)
    assert counts.cpu().tolist() == [U.SENTINEL, -1] and U.untouched(grad)


# ---- 3. the workspace is left as it is

def test_the_pair_list_is_the_same_before_and_after(crate):
    import torch
    case = GK.cases()["long_rows"]
    points, radius = case.points, case.radius
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    n = len(points)
    want = S.pairs(points, radius)
    total = len(want[1])
    offsets, counts, out = U.full(n + 1, dev), U.full(2, dev), U.full(2, dev)
    before, after = [U.full(total, dev), U.full(total, dev, U.SENTINEL_F)], [U.full(total, dev), U.full(total, dev, U.SENTINEL_F)]
    _, _, a, b, row_s, part_s, _ = GK.uses(case)["points"]
    held = [U.tensor(points, 2), U.tensor(a, None), U.tensor(b, None), U.tensor(row_s, None),
            U.tensor(points[:40] + 0.25 * radius, 2)]
    grad, probe_grad = U.full((n, 2), dev, U.SENTINEL_F), U.full((40, 2), dev, U.SENTINEL_F)
    eng.pairs_count(held[0], radius=radius, offsets=offsets, counts=counts)
    eng.pairs_fill(*before)
    eng.pairs_sum_grad(grad, held[1], held[2], held[3], held[3], power=3, counts=out)
    eng.pairs_sum_grad(probe_grad, None, None, None, held[3], power=2, queries=held[4], counts=out)
    eng.pairs_fill(*after)
    eng.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before, after))
    assert U.same_bits_or_nan(after[0], want[1]) and U.same_bits_or_nan(after[1], want[2])
    assert U.same_bits_or_nan(grad, GS.position_grad(None, points, radius, 3, a, b, row_s, part_s, True))
    assert U.same_bits_or_nan(probe_grad,
                              GS.position_grad(points[:40] + 0.25 * radius, points, radius, 2, None, None, None, part_s))


# ---- 4. errors

def test_argument_state_and_capacity_errors(sc):
    import torch
    from sand_crate_amd import _native as N
    n, width = 300, 3
    eng = sc.Engine(capacity=n + 64)
    lib, ctx = eng._lib, eng._ctx
    dev = torch.device("cuda", eng.device)
    points = np.random.RandomState(3).rand(n, 2)
    t = U.tensor(points, 2)
    a, b = U.tensor(FK.make_values(4, n, width), None), U.tensor(FK.make_values(5, n, width), None)
    s = U.tensor(FK.make_values(6, n), None)
    offsets, counts = U.full(n + 1, dev), U.full(2, dev)
    grad, out = U.full((n, 2), dev, U.SENTINEL_F), U.full(2, dev)
    torch.cuda.synchronize()
    ptr = lambda x: N._P(x.data_ptr())  # noqa: E731
    fn = lib.sc_pairs_sum_grad_device
    args = lambda **kw: tuple({**dict(ctx=ctx, q=None, nq=0, a=ptr(a), arows=n, b=ptr(b), brows=n, c=width, rs=ptr(s),  # noqa: E731
                                      ps=ptr(s), power=3, grad=ptr(grad), room=n, counts=ptr(out)), **kw}.values())
    assert fn(*args()) == N.ERR_STATE                                               # no count yet
    assert U.code_of(eng.pairs_sum_grad, grad, a, b, counts=out) == N.ERR_STATE
    eng.pairs_count(t, radius=0.05, offsets=offsets, counts=counts)
    assert fn(*args(ctx=None)) == N.ERR_ARG
    assert fn(*args(counts=None)) == N.ERR_ARG
    assert fn(*args(grad=None)) == N.ERR_ARG
    for bad in (-1, N.FIELDS_MAX_CHANNELS + 1):
        assert fn(*args(c=bad)) == N.ERR_ARG
    assert fn(*args(a=None)) == N.ERR_ARG                                           # channels without row_a
    assert fn(*args(b=None)) == N.ERR_ARG                                           # ... or without part_b
    for bad in (-1, 4):
        assert fn(*args(power=bad)) == N.ERR_ARG
    assert fn(*args(room=-1)) == N.ERR_ARG
    assert fn(*args(arows=-1)) == N.ERR_ARG
    assert fn(*args(brows=-1)) == N.ERR_ARG
    assert fn(*args(q=ptr(t), nq=-1)) == N.ERR_ARG
    assert fn(*args(q=N._P(t.data_ptr() + 8), nq=n - 1)) == N.ERR_ARG               # misaligned queries
    assert fn(*args(grad=N._P(grad.data_ptr() + 8), room=n - 1)) == N.ERR_ARG       # ... and gradient
    assert fn(*args(room=n - 1)) == N.ERR_CAPACITY                                  # a short gradient, self form
    assert fn(*args(q=ptr(t), nq=n, room=n - 1)) == N.ERR_CAPACITY                  # ... and for the queries
    assert fn(*args(q=ptr(t), nq=(1 << 28) + 1, room=(1 << 28) + 1)) == N.ERR_CAPACITY
    assert U.code_of(eng.pairs_sum_grad, grad[:n - 1], a, b, counts=out) == N.ERR_CAPACITY
    assert lib.sc_last_error()
    for call in (lambda: eng.pairs_sum_grad(grad, a, b, power=4, counts=out), lambda: eng.pairs_sum_grad(grad, a, None, counts=out),
                 lambda: eng.pairs_sum_grad(grad, a, b[:, :2], counts=out), lambda: eng.pairs_sum_grad(grad, a, b, s[:n - 1], counts=out),
                 lambda: eng.pairs_sum_grad(grad, a, b, room=n + 1, counts=out), lambda: eng.pairs_sum_grad(grad, a, b, row_rows=n + 1, counts=out),
                 lambda: eng.pairs_sum_grad(grad[:, :1], a, b, counts=out), lambda: eng.pairs_sum_grad(grad, a, b, part_rows=n + 1, counts=out)):
        with pytest.raises(ValueError):
            call()
    eng.synchronize()
    assert U.untouched(grad, out)
    assert fn(*args()) == 0                                                         # and as it should be: fine
    eng.synchronize()
    A, B, sv = a.cpu().numpy(), b.cpu().numpy(), s.cpu().numpy()
    assert out.cpu().tolist() == [n, 0] and U.same_bits_or_nan(grad, GS.position_grad(None, points, 0.05, 3, A, B, sv, sv, True))
    assert fn(*args(q=ptr(t), nq=10, room=10, a=None, b=None, c=0, ps=None)) == 0   # row_s alone, few queries
    eng.synchronize()
    assert U.same_bits_or_nan(grad[:10], GS.position_grad(points[:10], points, 0.05, 3, None, None, sv, None))
    eng.upload(points, np.zeros_like(points))                                       # an upload since the count
    assert fn(*args()) == N.ERR_STATE
    eng.close()


# ---- 5. field_function: the forward is field_tensors, the backward is the rule

@pytest.mark.parametrize("name", ["channels_3", "channels_17", "one_dimensional", "density", "queries_257", "query_density",
                                  "values_not_finite", "n_0_p0"])
def test_forward_is_field_tensors_bit_for_bit(crate, name):
    import torch
    case = GK.cases()[name]
    kw = dict(power=case.power, include_self=case.include_self, points=U.tensor(case.points, 2),
              queries=U.tensor(case.queries, 2), weight_sums=True)
    want = crate.field_tensors(U.tensor(case.values, None), case.radius, **kw)
    plain = crate.field_function(U.tensor(case.values, None), case.radius, **kw)
    assert all(t.grad_fn is None and not t.requires_grad for t in plain)            # requires_grad nowhere: no graph
    out, _ = run_function(crate, case, needs_of(case), weight_sums=True)
    assert all(t.requires_grad for t in out)
    for got in (plain, out):
        assert len(got) == len(want)
        assert all(a.shape == b.shape and torch.equal(a.detach().view(torch.int64), b.view(torch.int64)) for a, b in zip(got, want))
    with torch.no_grad():
        quiet = crate.field_function(U.tensor(case.values, None, requires_grad=case.values is not None), case.radius, **kw)
    assert all(t.grad_fn is None for t in quiet)
    with pytest.raises(ValueError, match="power"):
        crate.field_function(U.tensor(case.values, None), case.radius, power=4,
                             points=U.tensor(case.points, 2, requires_grad=True))


@pytest.mark.parametrize("name", CASES)
def test_backward_equals_the_spec(crate, name):
    case = GK.cases()[name]
    _, grads = run_function(crate, case, needs_of(case))
    check_gradients(case, GK.spec(name), grads)


@pytest.mark.parametrize("name", [GK.ORDER, "channels_9", "queries_65", "query_on_a_point", "density", "no_gw", "no_G_queries"])
def test_backward_singly_equals_together(crate, name):
    case = GK.cases()[name]
    for need in needs_of(case):
        _, grads = run_function(crate, case, (need,))
        assert list(grads) == [need]
        check_gradients(case, GK.spec(name), grads)


def test_include_self_plays_no_part_in_the_position_gradient(crate):
    case = GK.cases()[GK.ORDER]
    a = run_function(crate, case, ("points",))[1]["points"]
    b = run_function(crate, case._replace(include_self=True), ("points",))[1]["points"]
    assert U.same_bits_or_nan(a, b.cpu().numpy()) and U.same_bits_or_nan(a, GK.spec(GK.ORDER)["points"])


def test_state_form_and_a_tick_between_forward_and_backward(sc):
    import torch
    crate = sc.Crate(U.scene(sc))
    for _ in range(40):
        crate.physics_tick()
    particles, velocities = crate.state_tensors(pressure=False)
    n = len(particles)
    assert n > 100
    points, v = particles.cpu().numpy(), velocities.cpu().numpy()
    G, gw = FK.make_values(12, n, 2), FK.make_values(13, n)
    radius = 2.0 * crate.diameter
    want_forward = crate.field_tensors(velocities, radius, power=2, weight_sums=True)

    def run(tick):
        values = velocities.clone().requires_grad_()
        torch.cuda.synchronize()
        out = crate.field_function(values, radius, power=2, weight_sums=True)       # the state form
        forward = [t.detach().clone() for t in out]
        if tick:
            crate.physics_tick()
        grad, = torch.autograd.grad(list(out), [values], [U.tensor(G, None), U.tensor(gw, None)])
        return forward, grad

    forward, grad = run(False)
    assert all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(forward, want_forward))
    assert U.same_bits_or_nan(grad, GS.values_grad(points, radius, G, 2, True))
    forward_t, grad_t = run(True)
    assert all(torch.equal(a, b) for a, b in zip(forward, forward_t)) and torch.equal(grad, grad_t)
    assert not torch.equal(crate.state_tensors(pressure=False)[0], particles)   # the tick did move them
    # probes over the state, the gradient with respect to the probes
    probes = U.tensor(points[:50] + 0.3 * crate.diameter, 2, requires_grad=True)
    crate_points = crate.state_tensors(pressure=False)[0].cpu().numpy()
    vel = crate.state_tensors(pressure=False)[1]
    sums, wsum = crate.field_function(vel, radius, queries=probes, weight_sums=True)
    g, = torch.autograd.grad([sums, wsum], [probes], [U.tensor(G[:50], None), U.tensor(gw[:50], None)])
    assert U.same_bits_or_nan(g, GS.query_queries_grad(crate_points, radius, vel.cpu().numpy(), 3, probes.detach().cpu().numpy(),
                                                       G[:50], gw[:50]))


def test_raster_through_normalized_back_to_the_values(crate):
    import torch
    from sand_crate_amd import pairs
    case = GK.cases()["queries_257"]
    points, radius, C = case.points, 1.5 * case.radius, 2
    n = len(points)
    nx, ny = 16, 12
    target = np.random.RandomState(21).randn(ny * nx, C)
    grid = pairs.grid_queries(0.0, 1.0, 0.0, 1.0, nx, ny, "cuda")
    values = U.tensor(case.values, None, requires_grad=True)
    sums, wsum = crate.field_function(values, radius, points=U.tensor(points, 2), queries=grid, weight_sums=True)
    image = pairs.normalized(sums, wsum)
    (image * U.tensor(target, None)).sum().backward()
    got = values.grad.cpu().numpy()
    assert np.isfinite(got).all() and (got != 0).any()
    # torch's dense float64 autograd of the same raster, on the CPU
    P, Q = torch.tensor(points), grid.cpu()
    V = torch.tensor(np.array(case.values), requires_grad=True)
    d2 = (Q[:, None, 0] - P[None, :, 0]) ** 2 + (Q[:, None, 1] - P[None, :, 1]) ** 2
    r2 = radius * radius
    w = torch.where(d2 <= r2, (1.0 - d2 / r2) ** 3, torch.zeros_like(d2))
    dense_w = w.sum(dim=1)
    (pairs.normalized(w @ V, dense_w) * torch.tensor(target)).sum().backward()
    want = V.grad.numpy()
    w, dense_w = w.numpy(), dense_w.numpy()
    G = np.where(dense_w[:, None] == 0, 0.0, target / np.where(dense_w == 0, 1.0, dense_w)[:, None])
    reach = (w > 0)
    factor = reach.sum(axis=0) + 2 * reach.sum(axis=1).max() + 2 * C + 24
    bound = factor[:, None] * 2.0 ** -53 * (w[:, :, None] * np.abs(G)[:, None, :]).sum(axis=0)
    err = np.abs(got - want)
    print("raster: worst error", float((err[bound > 0] / bound[bound > 0]).max()), "of the bound")
    assert (err <= bound).all()
