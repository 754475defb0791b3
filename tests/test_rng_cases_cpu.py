"""The BTPE cases of tests/rng_cases.py reach every branch of NumPy's legacy BTPE binomial.

A copy of oracle/rng.py:binomial_btpe that records the branches it takes replays the GPU sweep's stream exactly --
each case's seed, CALLS calls, every call a binomial then 2 x rand(count, 2) -- and equals
`np.random.RandomState(seed).binomial` draw for draw."""
import math

import numpy as np
import pytest

from oracle.rng import MT19937, binomial_btpe_setup
from rng_cases import CALLS, SWEEP, seed_of, takes_btpe

BRANCHES = ("triangle", "parallelogram accept", "parallelogram reject", "left tail", "right tail", "ratio m < y",
            "ratio m > y", "squeeze accept", "squeeze reject", "stirling")


def binomial_btpe_tagged(rng: MT19937, n: int, p: float, hit: set) -> int:
    """oracle/rng.py:binomial_btpe, adding the name of every branch it takes to `hit`."""
    k_ = binomial_btpe_setup(n, p)
    r, q, m, p1, xm, xl, xr, c = (k_[x] for x in ("r", "q", "m", "p1", "xm", "xl", "xr", "c"))
    laml, lamr, p2, p3, p4, nrq = (k_[x] for x in ("laml", "lamr", "p2", "p3", "p4", "nrq"))
    while True:
        u = rng.next_double() * p4
        v = rng.next_double()
        if u <= p1:
            hit.add("triangle")
            return int(math.floor(xm - p1 * v + u))
        if u <= p2:
            x = xl + (u - p1) / c
            v = v * c + 1.0 - abs(m - x + 0.5) / p1
            if v > 1.0:
                hit.add("parallelogram reject")
                continue
            hit.add("parallelogram accept")
            y = int(math.floor(x))
        elif u <= p3:
            hit.add("left tail")
            if v == 0.0:
                continue
            y = int(math.floor(xl + math.log(v) / laml))
            if y < 0:
                continue
            v = v * (u - p2) * laml
        else:
            hit.add("right tail")
            if v == 0.0:
                continue
            y = int(math.floor(xr - math.log(v) / lamr))
            if y > n:
                continue
            v = v * (u - p3) * lamr
        k = abs(y - m)
        if k > 20 and k < nrq / 2.0 - 1:
            rho = (k / nrq) * ((k * (k / 3.0 + 0.625) + 0.16666666666666666) / nrq + 0.5)
            t = -k * k / (2 * nrq)
            big_a = math.log(v)
            if big_a < t - rho:
                hit.add("squeeze accept")
                return y
            if big_a > t + rho:
                hit.add("squeeze reject")
                continue
            hit.add("stirling")
            x1, f1, z, w = y + 1, m + 1, n + 1 - m, n - y + 1
            x2, f2, z2, w2 = x1 * x1, f1 * f1, z * z, w * w
            if big_a > (xm * math.log(f1 / x1) + (n - m + 0.5) * math.log(z / w) + (y - m) * math.log(w * r / (x1 * q))
                        + (13680. - (462. - (132. - (99. - 140. / f2) / f2) / f2) / f2) / f1 / 166320.
                        + (13680. - (462. - (132. - (99. - 140. / z2) / z2) / z2) / z2) / z / 166320.
                        + (13680. - (462. - (132. - (99. - 140. / x2) / x2) / x2) / x2) / x1 / 166320.
                        + (13680. - (462. - (132. - (99. - 140. / w2) / w2) / w2) / w2) / w / 166320.):
                continue
            return y
        s = r / q
        a = s * (n + 1)
        f = 1.0
        if m < y:
            hit.add("ratio m < y")
            for i in range(m + 1, y + 1):
                f *= a / i - s
        elif m > y:
            hit.add("ratio m > y")
            for i in range(y + 1, m + 1):
                f /= a / i - s
        if v > f:
            continue
        return y


def replay(flow: int, dt: float):
    """The GPU sweep of one BTPE case: -> (the port's counts, NumPy's counts, the branches hit)."""
    rs = np.random.RandomState(seed_of(flow, dt))
    _, key, pos, _, _ = rs.get_state()
    mine = MT19937(key, pos)
    hit, got, want = set(), [], []
    for _ in range(CALLS):
        got.append(binomial_btpe_tagged(mine, flow, dt, hit))
        want.append(int(rs.binomial(flow, dt)))
        assert (mine.mt, mine.pos) == ([int(w) for w in rs.get_state()[1]], rs.get_state()[2])
        rs.rand(want[-1], 2)  # the jitter and the velocity noise of the emitted particles (the room never binds) ...
        rs.rand(want[-1], 2)
        _, key, pos, _, _ = rs.get_state()
        mine = MT19937(key, pos)  # ... skipped by NumPy: the port only restates the binomial
    return got, want, hit


def test_the_sweep_switches_branch_where_numpy_does():
    inversion = [c for c in SWEEP if not takes_btpe(*c)]
    btpe = [c for c in SWEEP if takes_btpe(*c)]
    assert (15000, 0.002) in inversion and (14999, 0.002) in inversion  # n p = 30.0 exactly stays on inversion
    assert (15001, 0.002) in btpe and (2000, 0.5) in btpe
    assert len(btpe) >= 6 and CALLS >= 300


@pytest.mark.parametrize("flow,dt", [c for c in SWEEP if takes_btpe(*c)])
def test_btpe_port_equals_numpy_on_the_sweep(flow, dt):
    got, want, _ = replay(flow, dt)
    assert got == want


def test_btpe_sweep_reaches_every_branch():
    hit_by_case = {c: replay(*c)[2] for c in SWEEP if takes_btpe(*c)}
    hit = set().union(*hit_by_case.values())
    assert hit == set(BRANCHES), f"not reached: {set(BRANCHES) - hit}"
    # the squeeze needs n p q > 44: the smallest cases stay out of it, the large ones go through it
    assert "squeeze accept" not in hit_by_case[(20000, 0.002)]
    for c in ((100000, 0.002), (1000, 0.5), (10 ** 6, 0.01)):
        assert {"squeeze accept", "squeeze reject", "stirling"} <= hit_by_case[c], c
