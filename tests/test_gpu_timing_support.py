"""GPU test of the timing scripts' shared module (scripts/timing_support.py): the bookkeeping of `device_times` -- names,
events and the stream the engine is left on -- and the two states every script times on.  64 and 256 particles are
enough: what can go wrong here is events, streams and arguments, not a kernel."""
import math
import sys
from pathlib import Path

import pytest

import gpu_support as U
from gpu_support import sc  # noqa: F401

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scripts"))

import timing_support as T  # noqa: E402

pytestmark = pytest.mark.gpu


def test_device_times_gives_reps_spans_per_call_in_order_and_hands_the_stream_back(sc):  # noqa: F811
    import torch
    crate = T.bench_crate(64, 2)
    eng = crate.engine
    dev = torch.device("cuda", eng.device)
    offsets = torch.empty(eng.capacity + 1, dtype=torch.int64, device=dev)
    counts = torch.empty(2, dtype=torch.int64, device=dev)
    eng.pairs_count(None, radius=crate.diameter, offsets=offsets, counts=counts)
    eng.synchronize()
    total = int(counts[1])
    partners = torch.empty(total, dtype=torch.int64, device=dev)
    d2 = torch.empty(total, dtype=torch.float64, device=dev)
    made = []
    calls = {"count": lambda: (made.append("count"), eng.pairs_count(None, radius=crate.diameter, offsets=offsets, counts=counts)),
             "fill": lambda: (made.append("fill"), eng.pairs_fill(partners, d2))}
    assert eng.stream is None
    times = T.device_times(eng, calls, reps=3, warmup=2)
    assert eng.stream is None                                                        # on its own stream again
    assert list(times) == ["count", "fill"]
    assert made == ["count", "fill"] * 5                                             # 2 rounds of warm-up, 3 recorded
    for series in times.values():
        assert len(series) == 3 and all(math.isfinite(t) and t > 0 for t in series)
    assert counts.tolist() == [crate.particle_count, total]                          # the calls ran, on a stream torch sees
    crate.close()


def test_the_two_states_are_the_ones_the_scripts_built_by_hand(sc):  # noqa: F811
    """The benchmark's state holds the particles asked for when it is made; two ticks later it is, byte for byte, what
    the lines the scripts used to spell out give (in a world of 256 a particle or two has left the box by then: the
    count after the ticks is the hand-built crate's, not 256)."""
    crate = T.bench_crate(256, 0)
    assert crate.particle_count == 256 and crate.tick == 0 and crate._noise == "counter"
    assert crate.engine.capacity == 256 + 1024
    crate.close()
    by_hand = U.m2_crate(sc, 256)
    by_hand.run(2)
    by_hand.synchronize()
    crate = T.bench_crate(256, 2)
    assert crate.tick == 2 and crate._noise == "counter" and 0 < crate.particle_count == by_hand.particle_count <= 256
    for got, want in zip(crate.engine.download(), by_hand.engine.download()):
        U.same_bytes(got, want)
    crate.close()
    by_hand.close()

    by_hand = sc.Crate(U.scene(sc))
    for _ in range(2):
        by_hand.physics_tick()
    by_hand.synchronize()
    crate = T.viewer_crate(2)
    assert crate.tick == 2 and crate._noise == "host"
    assert crate.particle_count == by_hand.particle_count > 0
    assert len(crate.engine.download()[0]) == crate.particle_count
    crate.close()
    by_hand.close()
