"""What the Python neighbourhood calls ask of the engine, call by call: `Crate.pair_tensors`, `cluster_tensors`,
`cluster_sums`, `cluster_observables`, `neighbor_tensors`, `field_tensors`, `field_function` (with its backward) and
`distance_histogram`, each in its forms -- synchronising or not, with `points`, with `queries`, with `batch` and
`query_batch` -- against a list written down here.  The results are other files' business (test_gpu_pairs.py and its
kin); this one pins the protocol above the kernels: which engine methods run, in which order, with which keywords, where
torch's stream and the library's are synchronised, and how often the host reads from the device.

The engine's `pairs_*` methods and `synchronize` are wrapped on the instance, so calls one engine method makes of another
(`pairs_count` sets the batch, `pairs_sum` the query offsets) are seen too.  A call is logged when it RETURNS: that is
the order in which the library was entered, whichever Python method did the entering.  An entry is (name, positional
arguments, keywords): a positional tensor is "tensor", None stays None; of the keywords those are kept that are neither
tensors nor None.  `Stream.synchronize` of torch is logged as "torch_stream".  Device-to-host reads -- `.cpu()`,
`.item()`, `.tolist()` and `int()`, `float()`, `bool()` or an index made of a CUDA tensor -- are counted; a form may read
less than the number written here, never more."""
import contextlib
from pathlib import Path

import numpy as np
import pytest

from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
RADIUS = 1.5
LINE = np.stack([1.0 + np.arange(8.0), np.full(8, 2.0)], axis=1)    # 8 points at spacing 1.0
PROBES = np.array([[1.5, 2.0], [4.0, 2.25], [7.75, 2.0]])           # 3 queries
CLOUDS, PROBE_CLOUDS = [0, 4, 8], [0, 2, 3]                         # two clouds of 4 points; their queries
CAPACITY = 64
READS = ("cpu", "item", "tolist", "__int__", "__index__", "__float__", "__bool__")


@pytest.fixture(scope="module")
def crate(sc):
    crate = sc.Crate(sc.load_config(ROOT / "config" / "wave_machine.yaml").world_config, noise="none", capacity=CAPACITY)
    crate.particles = LINE
    return crate


def inputs():
    """The tensors the forms are called with, by name."""
    import torch
    made = dict(points=torch.from_numpy(LINE.copy()).cuda(), queries=torch.from_numpy(PROBES.copy()).cuda(),
                batch=torch.tensor(CLOUDS, dtype=torch.int64).cuda(),
                query_batch=torch.tensor(PROBE_CLOUDS, dtype=torch.int64).cuda(),
                values=torch.from_numpy(np.arange(16.0).reshape(8, 2)).cuda(), column=torch.from_numpy(np.arange(8.0)).cuda(),
                wide=torch.from_numpy(np.arange(8.0 * 17).reshape(8, 17)).cuda())
    torch.cuda.synchronize()
    return made


def note(value):
    if hasattr(value, "is_cuda"):
        return "tensor"
    if isinstance(value, np.ndarray):
        return tuple(value.tolist())
    return value


@contextlib.contextmanager
def traced(engine):
    """-> (calls, reads): the log of the engine's calls, and a one-element list with the count of device-to-host reads."""
    import torch
    calls, reads = [], [0]

    def logged(name, method):
        def call(*args, **kw):
            try:
                return method(*args, **kw)
            finally:
                given = {k: note(v) for k, v in kw.items()}
                calls.append((name, tuple(note(v) for v in args if not isinstance(v, torch.cuda.Stream)),
                              {k: v for k, v in given.items() if v is not None and v != "tensor"}))
        return call

    def counted(method):
        def call(self, *args, **kw):
            reads[0] += bool(self.is_cuda)
            return method(self, *args, **kw)
        return call

    names = [name for name in dir(type(engine)) if name.startswith("pairs_") or name == "synchronize"]
    kept = {name: getattr(torch.Tensor, name) for name in READS}
    own = [name for name in READS if name in vars(torch.Tensor)]
    stream_synchronize = torch.cuda.Stream.synchronize
    for name in names:
        setattr(engine, name, logged(name, getattr(engine, name)))
    for name, method in kept.items():
        setattr(torch.Tensor, name, counted(method))
    torch.cuda.Stream.synchronize = logged("torch_stream", stream_synchronize)
    try:
        yield calls, reads
    finally:
        torch.cuda.Stream.synchronize = stream_synchronize
        for name, method in kept.items():
            if name in own:
                setattr(torch.Tensor, name, method)
            else:
                delattr(torch.Tensor, name)
        for name in names:
            delattr(engine, name)


@contextlib.contextmanager
def on_torch_stream(engine):
    import torch
    engine.set_stream(torch.cuda.current_stream(torch.device("cuda", engine.device)).cuda_stream)
    try:
        yield
    finally:
        engine.use_own_stream()


def grads(t, *names):
    """The inputs with fresh leaves that require grad in the places of `names`."""
    return {**t, **{name: t[name].clone().requires_grad_() for name in names}}


def function_form(crate, t, *wanted, given):
    """`field_function` with the inputs named in `given`, `wanted` requiring grad, and the backward of the sum of what it
    returns."""
    t = grads(t, *wanted)
    out = crate.field_function(t["values"], RADIUS, weight_sums=True, **{name: t[name] for name in given})
    (out[0].sum() + out[1].sum()).backward()


def observables_unsynchronised(crate, t):
    with on_torch_stream(crate.engine):
        crate.cluster_observables(RADIUS, max_clusters=4)


FORMS = {
    "pair_tensors: state": lambda c, t: c.pair_tensors(RADIUS),
    "pair_tensors: state, half, d2": lambda c, t: c.pair_tensors(RADIUS, half=True, squared_distances=True),
    "pair_tensors: state, max_pairs": lambda c, t: c.pair_tensors(RADIUS, max_pairs=32),
    "pair_tensors: points": lambda c, t: c.pair_tensors(RADIUS, points=t["points"]),
    "pair_tensors: points, batch": lambda c, t: c.pair_tensors(RADIUS, points=t["points"], batch=t["batch"]),
    "pair_tensors: points, batch, max_pairs": lambda c, t: c.pair_tensors(RADIUS, points=t["points"], batch=t["batch"], half=True,
                                                                       max_pairs=32),
    "cluster_tensors: state": lambda c, t: c.cluster_tensors(RADIUS),
    "cluster_tensors: state, max_clusters": lambda c, t: c.cluster_tensors(RADIUS, max_clusters=4),
    "cluster_tensors: points": lambda c, t: c.cluster_tensors(RADIUS, points=t["points"]),
    "cluster_sums: state": lambda c, t: c.cluster_sums(t["values"], RADIUS),
    "cluster_sums: state, extrema, max_clusters": lambda c, t: c.cluster_sums(t["column"], RADIUS, extrema=True, max_clusters=4),
    "cluster_sums: points, extrema": lambda c, t: c.cluster_sums(t["values"], RADIUS, points=t["points"], extrema=True),
    "cluster_observables": lambda c, t: c.cluster_observables(RADIUS),
    "cluster_observables: max_clusters": observables_unsynchronised,
    "neighbor_tensors: state": lambda c, t: c.neighbor_tensors(3, RADIUS, squared_distances=True, partner_counts=True),
    "neighbor_tensors: state, no sync": lambda c, t: c.neighbor_tensors(3, RADIUS, sync=False),
    "neighbor_tensors: state, queries": lambda c, t: c.neighbor_tensors(3, RADIUS, queries=t["queries"]),
    "neighbor_tensors: state, queries, no sync": lambda c, t: c.neighbor_tensors(3, RADIUS, queries=t["queries"], sync=False),
    "neighbor_tensors: points, queries": lambda c, t: c.neighbor_tensors(3, RADIUS, points=t["points"], queries=t["queries"]),
    "neighbor_tensors: points, batch": lambda c, t: c.neighbor_tensors(3, RADIUS, points=t["points"], batch=t["batch"]),
    "neighbor_tensors: points, queries, batch, query_batch":
        lambda c, t: c.neighbor_tensors(3, RADIUS, points=t["points"], queries=t["queries"], batch=t["batch"],
                                        query_batch=t["query_batch"]),
    "neighbor_tensors: points, queries, batch, query_batch, no sync":
        lambda c, t: c.neighbor_tensors(3, RADIUS, points=t["points"], queries=t["queries"], batch=t["batch"],
                                        query_batch=t["query_batch"], sync=False),
    "field_tensors: state": lambda c, t: c.field_tensors(t["values"], RADIUS, weight_sums=True),
    "field_tensors: state, density": lambda c, t: c.field_tensors(None, RADIUS, power=2, include_self=False),
    "field_tensors: state, no sync": lambda c, t: c.field_tensors(t["column"], RADIUS, sync=False),
    "field_tensors: state, queries": lambda c, t: c.field_tensors(t["values"], RADIUS, queries=t["queries"]),
    "field_tensors: state, queries, no sync": lambda c, t: c.field_tensors(t["values"], RADIUS, queries=t["queries"], sync=False),
    "field_tensors: points, 17 columns": lambda c, t: c.field_tensors(t["wide"], RADIUS, points=t["points"], weight_sums=True),
    "field_tensors: points, batch": lambda c, t: c.field_tensors(t["values"], RADIUS, points=t["points"], batch=t["batch"]),
    "field_tensors: points, queries, batch, query_batch, 17 columns":
        lambda c, t: c.field_tensors(t["wide"], RADIUS, points=t["points"], queries=t["queries"], batch=t["batch"],
                                     query_batch=t["query_batch"], weight_sums=True),
    "field_tensors: points, queries, batch, query_batch, no sync":
        lambda c, t: c.field_tensors(t["values"], RADIUS, points=t["points"], queries=t["queries"], batch=t["batch"],
                                     query_batch=t["query_batch"], sync=False),
    "field_function: nothing requires grad": lambda c, t: c.field_function(t["values"], RADIUS, points=t["points"]),
    "field_function: state, values": lambda c, t: function_form(c, t, "values", given=()),
    "field_function: points; values and points": lambda c, t: function_form(c, t, "values", "points", given=("points",)),
    "field_function: points, queries; all three":
        lambda c, t: function_form(c, t, "values", "points", "queries", given=("points", "queries")),
    "field_function: points, queries, batch, query_batch; all three":
        lambda c, t: function_form(c, t, "values", "points", "queries", given=("points", "queries", "batch", "query_batch")),
    "field_function: points, batch, 17 columns; points":
        lambda c, t: function_form(c, {**t, "values": t["wide"]}, "points", given=("points", "batch")),
    "distance_histogram: state": lambda c, t: c.distance_histogram([0.0, 1.0, RADIUS]),
    "distance_histogram: state, per_row, no sync": lambda c, t: c.distance_histogram([0.0, 1.0, RADIUS], per_row=True, sync=False),
    "distance_histogram: state, queries": lambda c, t: c.distance_histogram([0.0, 1.0, RADIUS], queries=t["queries"], per_row=True),
    "distance_histogram: state, queries, no sync":
        lambda c, t: c.distance_histogram([0.0, 1.0, RADIUS], queries=t["queries"], per_row=True, totals=False, sync=False),
    "distance_histogram: points, queries":
        lambda c, t: c.distance_histogram([0.5, RADIUS], points=t["points"], queries=t["queries"]),
}


def trace_of(crate, name):
    """-> (the device-to-host reads, the logged calls) of one form."""
    t = inputs()
    with traced(crate.engine) as (calls, reads):
        FORMS[name](crate, t)
    crate.engine.synchronize()  # (the forms that do not synchronise leave work queued)
    return reads[0], calls


# ---- what the forms do: written down from the code as it was before the protocol was written once

T = "tensor"
TORCH, SYNC = ("torch_stream", (), {}), ("synchronize", (), {})
QUERY_BATCH = ("pairs_set_query_batch", (T,), {})
LABEL = ("pairs_label", (T, T, T), {})


def count(points=T, half=True, batch=None):
    return [("pairs_set_batch", (batch,), {}), ("pairs_count", (points,), {"radius": RADIUS, "half": half})]


def whole(*readers, points=T, batch=None):
    """A synchronising call: torch's stream, the count with half=True, the readers, the library's stream."""
    return [TORCH, *count(points, batch=batch), *readers, SYNC]


def fill(*tensors):
    return ("pairs_fill", tensors, {})


def cluster_sums(*tensors):
    return ("pairs_cluster_sums", tensors, {})


def nearest(*tensors):
    return ("pairs_nearest", tensors, {"k": 3})


def summed(*tensors, power=3, include_self=True):
    return ("pairs_sum", tensors, {"power": power, "include_self": include_self})


def grad(*tensors):
    return ("pairs_sum_grad", tensors, {"power": 3})


def hist(*tensors, edges=(0.0, 1.0, RADIUS)):
    return ("pairs_hist", tensors, {"edges": edges})


# form -> (the most device-to-host reads it may make, the calls it makes)
EXPECTED = {
    "pair_tensors: state": (1, [TORCH, *count(None, half=False), SYNC, fill(T, None), SYNC]),
    "pair_tensors: state, half, d2": (1, [TORCH, *count(None), SYNC, fill(T, T), SYNC]),
    "pair_tensors: state, max_pairs": (0, [*count(None, half=False), fill(T, None)]),
    "pair_tensors: points": (1, [TORCH, *count(half=False), SYNC, fill(T, None), SYNC]),
    "pair_tensors: points, batch": (1, [TORCH, *count(half=False, batch=T), SYNC, fill(T, None), SYNC]),
    "pair_tensors: points, batch, max_pairs": (0, [*count(batch=T), fill(T, None)]),
    "cluster_tensors: state": (1, whole(LABEL, points=None)),
    "cluster_tensors: state, max_clusters": (0, [*count(None), LABEL]),
    "cluster_tensors: points": (1, whole(LABEL)),
    "cluster_sums: state": (1, whole(LABEL, cluster_sums(T, T), points=None)),
    "cluster_sums: state, extrema, max_clusters": (0, [*count(None), LABEL, cluster_sums(T, T, T, T)]),
    "cluster_sums: points, extrema": (1, whole(LABEL, cluster_sums(T, T, T, T))),
    "cluster_observables": (2, [TORCH, SYNC, *whole(LABEL, cluster_sums(T, T, T, T), points=None)]),  # (state_tensors first)
    "cluster_observables: max_clusters": (0, [*count(None), LABEL, cluster_sums(T, T, T, T)]),
    "neighbor_tensors: state": (1, whole(nearest(T, T, T), points=None)),
    "neighbor_tensors: state, no sync": (0, [*count(None), nearest(T, None, None)]),
    "neighbor_tensors: state, queries": (2, whole(nearest(T, None, None), points=None)),
    "neighbor_tensors: state, queries, no sync": (0, [*count(None), nearest(T, None, None)]),
    "neighbor_tensors: points, queries": (1, whole(nearest(T, None, None))),
    "neighbor_tensors: points, batch": (1, whole(nearest(T, None, None), batch=T)),
    "neighbor_tensors: points, queries, batch, query_batch": (1, whole(QUERY_BATCH, nearest(T, None, None), batch=T)),
    "neighbor_tensors: points, queries, batch, query_batch, no sync": (0, [*count(batch=T), QUERY_BATCH, nearest(T, None, None)]),
    "field_tensors: state": (1, whole(summed(T, T, T), points=None)),
    "field_tensors: state, density": (1, whole(summed(None, None, T, power=2, include_self=False), points=None)),
    "field_tensors: state, no sync": (0, [*count(None), summed(T, T, None)]),
    "field_tensors: state, queries": (2, whole(summed(T, T, None), points=None)),
    "field_tensors: state, queries, no sync": (0, [*count(None), summed(T, T, None)]),
    "field_tensors: points, 17 columns": (1, whole(summed(T, T, T), summed(T, T, None), summed(T, T, None))),  # (wsum once)
    "field_tensors: points, batch": (1, whole(summed(T, T, None), batch=T)),
    "field_tensors: points, queries, batch, query_batch, 17 columns":  # (every launch is given the query offsets)
        (1, whole(QUERY_BATCH, summed(T, T, T), QUERY_BATCH, summed(T, T, None), QUERY_BATCH, summed(T, T, None), batch=T)),
    "field_tensors: points, queries, batch, query_batch, no sync": (0, [*count(batch=T), QUERY_BATCH, summed(T, T, None)]),
    "field_function: nothing requires grad": (1, whole(summed(T, T, None))),
    "field_function: state, values": (3, [TORCH, SYNC, *whole(summed(T, T, T)), *whole(summed(T, T, None))]),  # (state_tensors)
    "field_function: points; values and points":
        (3, [*whole(summed(T, T, T)), *whole(summed(T, T, None)), *whole(grad(T, T, T, T, T))]),
    "field_function: points, queries; all three":
        (4, [*whole(summed(T, T, T)), *whole(summed(T, T, None)), *whole(grad(T, T, T, None, T)), *whole(grad(T, T, T, T, None))]),
    "field_function: points, queries, batch, query_batch; all three":
        (4, [*whole(QUERY_BATCH, summed(T, T, T), batch=T), *whole(QUERY_BATCH, summed(T, T, None), batch=T),
             *whole(QUERY_BATCH, grad(T, T, T, None, T), batch=T), *whole(QUERY_BATCH, grad(T, T, T, T, None), batch=T)]),
    "field_function: points, batch, 17 columns; points":  # (34 channels: five launches, the scalars with the first)
        (2, [*whole(summed(T, T, T), summed(T, T, None), summed(T, T, None), batch=T),
             *whole(grad(T, T, T, T, T), *[grad(T, T, T, None, None)] * 4, batch=T)]),
    "distance_histogram: state": (1, whole(hist(None, T), points=None)),
    "distance_histogram: state, per_row, no sync": (0, [*count(None), hist(T, T)]),
    "distance_histogram: state, queries": (2, whole(hist(T, T), points=None)),
    "distance_histogram: state, queries, no sync": (0, [*count(None), hist(T, None)]),
    "distance_histogram: points, queries": (1, whole(hist(None, T, edges=(0.5, RADIUS)))),
}


def test_every_form_is_written_down():
    assert sorted(EXPECTED) == sorted(FORMS)


@pytest.mark.parametrize("name", sorted(FORMS))
def test_trace(crate, name):
    reads, calls = trace_of(crate, name)
    most, want = EXPECTED[name]
    print(name, reads, calls)
    assert calls == want
    assert reads <= most
