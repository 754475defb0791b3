"""`Crate.field_tensors` under torch autograd: `field_function`, the weighted neighbourhood sums with gradients with
respect to the values, the points and the queries.  The forward is `field_tensors` itself; the backward runs on the same
grid kernels -- the values' gradient is the same sum with rows and partners swapped (the weight depends on the squared
distance only, which has the same bits from either end), the positions' gradient is sc_pairs_sum_grad_device
(csrc/sc_fields_grad.h).  tests/field_grad_spec.py is the rule, bit for bit.  torch is imported on first use."""
from __future__ import annotations

from . import _native as N
from .neighbourhood import _Search, _field_values

_function = None


def position_grad(crate, points, radius: float, power: int, row_a=None, part_b=None, row_s=None, part_s=None, *,
                  queries=None, batch=None, query_batch=None):
    """One use of the position rule (`position_grad_chunked` of tests/field_grad_spec.py) -> float64 (rows, 2): counts
    the pairs among `points`, then launches sc_pairs_sum_grad_device once per eight channels of `row_a` / `part_b`, the
    scalars `row_s` / `part_s` with the first, and adds the results in ascending order.  The rows are the points (the
    self form) or `queries`.  `batch` cuts `points` -- the grid -- into clouds and `query_batch` the `queries`, as in
    `field_tensors`.  Synchronises torch's stream before enqueuing and the library's at the end, as
    `field_tensors(sync=True)` does (`neighbourhood._Search`)."""
    import torch
    points = points.contiguous()
    queries = None if queries is None else queries.contiguous()
    call = _Search(crate, "field_function", radius, points=points, queries=queries, batch=batch, query_batch=query_batch,
                   short="an upstream gradient or the values has fewer rows than there are points")
    if power == 0:  # (the weights are constant: nothing runs)
        return torch.zeros((call.rows, 2), dtype=torch.float64, device=call.dev)
    step = N.FIELDS_MAX_CHANNELS
    width = 0 if row_a is None else int(row_a.shape[1])
    if width <= step:
        groups = [(None if row_a is None else row_a.contiguous(), None if part_b is None else part_b.contiguous())]
    else:
        groups = [(row_a[:, at:at + step].contiguous(), part_b[:, at:at + step].contiguous()) for at in range(0, width, step)]
    row_s = None if row_s is None else row_s.contiguous()
    part_s = None if part_s is None else part_s.contiguous()
    parts = [torch.empty((call.rows, 2), dtype=torch.float64, device=call.dev) for _ in groups]
    call.count()
    for at, ((a, b), part) in enumerate(zip(groups, parts)):
        call.eng.pairs_sum_grad(part, a, b, row_s if at == 0 else None, part_s if at == 0 else None, power=power,
                                queries=queries, counts=call.counts, query_batch=query_batch)
    call.read()
    total = parts[0]
    for part in parts[1:]:
        total = total + part
    return total


def _make_function():
    import torch
    from torch.autograd.function import once_differentiable

    class FieldFunction(torch.autograd.Function):
        """(values (n, C) or None, points (n, 2), queries (q, 2) or None) -> the tuple of `field_tensors(sync=True)`."""

        @staticmethod
        def forward(ctx, crate, radius, power, include_self, weight_sums, batch, query_batch, values, points, queries):
            out = crate.field_tensors(values, radius, power=power, include_self=include_self, points=points, queries=queries,
                                      weight_sums=weight_sums, batch=batch, query_batch=query_batch)
            ctx.crate, ctx.radius, ctx.power, ctx.include_self = crate, radius, power, include_self
            ctx.batch, ctx.query_batch = batch, query_batch
            ctx.has_sums = values is not None
            ctx.save_for_backward(*(t for t in (values, points, queries) if t is not None))
            ctx.set_materialize_grads(False)  # (an output nobody used has no gradient: nothing is launched for it)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            saved = list(ctx.saved_tensors)
            values = saved.pop(0) if ctx.has_sums else None
            points = saved.pop(0)
            queries = saved.pop(0) if saved else None
            crate, radius, power = ctx.crate, ctx.radius, ctx.power
            batch, query_batch = ctx.batch, ctx.query_batch
            G = grads[0] if ctx.has_sums else None
            gw = grads[-1] if len(grads) > int(ctx.has_sums) else None
            G = None if G is None else G.contiguous()
            gw = None if gw is None else gw.contiguous()
            need_values, need_points, need_queries = ctx.needs_input_grad[7:10]
            g_values = g_points = g_queries = None
            n = int(points.shape[0])
            if need_values and G is not None:
                if queries is None:
                    g_values, = crate.field_tensors(G, radius, power=power, include_self=ctx.include_self, points=points,
                                                    batch=batch)
                else:  # (rows and partners swap, and their offsets with them)
                    g_values, = crate.field_tensors(G, radius, power=power, points=queries, queries=points,
                                                    batch=query_batch, query_batch=batch)
                if values.shape[0] > n:  # (rows of values beyond the points were never read)
                    g_values = torch.cat([g_values, g_values.new_zeros((values.shape[0] - n, values.shape[1]))])
            dot = G is not None  # (without G -- or without values, which has no G -- s has no dot product)
            V = values[:n] if dot else None
            if need_points and (dot or gw is not None):
                if queries is None:
                    g_points = position_grad(crate, points, radius, power, torch.cat([G, V], dim=1) if dot else None,
                                             torch.cat([V, G], dim=1) if dot else None, gw, gw, batch=batch)
                else:  # (the grid is over the queries, cut by their offsets; the rows are the points)
                    g_points = position_grad(crate, queries, radius, power, V, G, None, gw, queries=points,
                                             batch=query_batch, query_batch=batch)
            if need_queries and (dot or gw is not None):
                g_queries = position_grad(crate, points, radius, power, G, V, gw, None, queries=queries, batch=batch,
                                          query_batch=query_batch)
            return None, None, None, None, None, None, None, g_values, g_points, g_queries

    return FieldFunction


def field_function(crate, values=None, radius=None, *, power: int = 3, include_self: bool = True, points=None, queries=None,
                   weight_sums: bool = False, batch=None, query_batch=None):
    """`crate.field_tensors(values, radius, power=, include_self=, points=, queries=, weight_sums=, sync=True)` attached
    to torch's autograd graph: the same arguments, the same tuple ``(sums[, wsum])``, the same bits -- and when `values`,
    `points` or `queries` requires grad, a backward that gives their gradients, computed on the GPU over the pair
    search's grid without the pair list and without floating-point atomics: a pure function of its inputs, bit for bit
    the rule of tests/field_grad_spec.py.  When nothing requires grad it is `field_tensors` and nothing more.

    With ``points=None`` (the crate's state) and a gradient to come, the positions are taken once from `state_tensors()`,
    the forward runs with them as `points` -- which gives the bits of the state form -- and they are kept for the
    backward: a tick between forward and backward changes nothing.  The backward computes only the gradients that are
    asked for and re-counts the grid each time (anything may have counted in between): for the values one count -- over
    the queries in the query form -- and one sum with rows and partners swapped; for the points and for the queries a
    count and sc_pairs_sum_grad_device, eight channels per launch.  Each of these synchronises torch's stream before it
    enqueues and the library's stream at the end, as `field_tensors(sync=True)` does: right with the crate on its own
    stream or on torch's.  ValueError for a coordinate outside the domain and for arrays with too few rows, as in the
    forward.  A point is never its own partner in the gradient with respect to the points, whatever `include_self`:
    its weight is constant.

    `batch` and `query_batch` are `field_tensors`' and reach every count of the backward: where rows and partners swap
    -- the values' gradient and the points' gradient of the query form, whose grid is over the queries -- the two swap too.

    Once differentiable: no second derivatives.  No gradient with respect to `radius`, and no `sync=False` form."""
    global _function
    import torch
    tensors = [t for t in (values, points, queries) if t is not None]
    if not torch.is_grad_enabled() or not any(getattr(t, "requires_grad", False) for t in tensors):
        return crate.field_tensors(values, radius, power=power, include_self=include_self, points=points, queries=queries,
                                   weight_sums=weight_sums, batch=batch, query_batch=query_batch)
    power = int(power)
    if not 0 <= power <= 3:
        raise ValueError("power must be 0 .. 3")
    radius = float(crate.diameter if radius is None else radius)
    values, flat = _field_values(values)
    if batch is not None and points is None:
        raise ValueError("field_function: batch needs points, the state is one cloud")
    if points is None:
        points = crate.state_tensors(pressure=False)[0]
    if _function is None:
        _function = _make_function()
    out = _function.apply(crate, radius, power, bool(include_self), bool(weight_sums), batch, query_batch, values, points,
                          queries)
    return (out[0].view(-1), *out[1:]) if flat else out
