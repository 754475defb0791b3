"""The worlds of tests/slab_cases.py (each proved on the CPU by tests/test_slab_cases_cpu.py) through `SlabChain` on the
HIP backend against a single-domain `Crate`: bit for bit, or the report of a wall fix that went too far beside a cut
(F_HALO_REACH) or of a particle that crossed a whole slab (F_HALO_CROSSED): SC_ERR_DOMAIN at the next synchronising call.  Tick by tick -- every tick packs with k_halo_pack and
unpacks plainly -- and as run(3), where the force kernel's epilogue packs and the unpack is fused; with and without
noise; without halo overlap everywhere, with it where the particles stay within the band margin."""
import pytest

import slab_cases
from gpu_support import sc  # noqa: F401
from slab_cases import CASES, EQUAL
from test_gpu_slabs import assert_chain_equals_single, single_domain

pytestmark = pytest.mark.gpu
TICKS = 3


_single = {}


def single_for(sc, name, axis, noise):
    """The single-domain result of a world after TICKS ticks: computed once, shared, never changed."""
    key = (name, axis, noise)
    if key not in _single:
        from sand_crate_amd.load_config import WorldConfig
        bodies, coef, p, v = CASES[name]().world(axis)
        out, _ = single_domain(sc, WorldConfig(bodies, [], coef), p, v, TICKS, noise=noise, seed=1)
        for a in out:
            a.setflags(write=False)
        _single[key] = out
    return _single[key]


def modes():
    out = []
    for name, build in CASES.items():
        for overlap in ((False, True) if build().overlap_ok else (False,)):
            out.append(pytest.param(name, overlap, id=f"{name}-{'overlap' if overlap else 'plain'}"))
    return out


@pytest.mark.parametrize("stepping", ["tick_by_tick", "look_ahead"])
@pytest.mark.parametrize("noise", ["counter", "none"])
@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("name,overlap", modes())
def test_slab_case(sc, name, overlap, axis, noise, stepping):
    from sand_crate_amd._native import NativeError
    from sand_crate_amd.load_config import WorldConfig
    from sand_crate_amd.slab import SlabChain
    case = CASES[name]()
    bodies, coef, p, v = case.world(axis)
    chain = SlabChain(WorldConfig(bodies, [], coef), p, v, case.n_slabs, noise=noise, noise_seed=1, cuts=case.cuts,
                      overlap=overlap, axis=axis, rebalance_every=case.rebalance_every, halo_capacity=512, capacity=4096)
    assert all(m.overlap == overlap for m in chain.members)
    def run():
        if stepping == "look_ahead":
            chain.run(TICKS)
        else:
            for _ in range(TICKS):
                chain.run(1)
        chain.synchronize()

    try:
        if case.expect == EQUAL:
            run()
            assert sum(chain.owned_counts()) == len(p)
            assert_chain_equals_single(chain, single_for(sc, name, axis, noise))
            if case.rebalance_every:
                assert chain.members[0].rebalances >= 1 and chain.slabs[0][1] > case.cuts[0]
        else:
            assert case.first_report_tick < TICKS
            with pytest.raises(NativeError, match=slab_cases.MESSAGES[case.expect]):
                run()
    finally:
        for m in chain.members:
            m.engine.close()
