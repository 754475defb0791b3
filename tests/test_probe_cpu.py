"""CPU checks of the probe: tests/probe_spec.py against a second, deliberately naive formulation (Python loops and
math.fsum) on the cases of tests/probe_cases.py -- the sums within the spec's stated tolerance, everything else equal --,
the cases themselves (each has the property it is named for), and the plumbing that needs no GPU: the names, the ABI
table, the driver's --observe.  The device is held to probe_spec by tests/test_gpu_probe.py."""
import inspect
import math
import re
from pathlib import Path

import numpy as np
import pytest

import probe_cases as K
import probe_spec as S

ROOT = Path(__file__).resolve().parent.parent


def launch_sizes():
    from sand_crate_amd import _native as N
    return N.PROBE_BLOCK, N.PROBE_BLOCK * N.PROBE_BLOCKS


@pytest.fixture(scope="module")
def cases():
    return K.cases(*launch_sizes())


CASE_NAMES = sorted(K.cases(8, 64))  # (the names do not depend on the sizes)


def naive(xy, vxy, pressure, tick, n_bins, x0, x1):
    """The rule once more, particle by particle: exact sums (math.fsum), comparisons spelt out."""
    sums = {name: [] for name in S.SUMS}
    n = pressed = binned = 0
    lo_x = lo_y = math.inf
    hi_x = hi_y = -math.inf
    top_speed2 = top_p = 0.0
    count = [0] * n_bins
    top = [math.inf] * n_bins
    w = (x1 - x0) / n_bins if n_bins else 1.0

    def lower(a, b):
        return b if (b < a or b != b) else a

    def higher(a, b):
        return b if (b > a or b != b) else a

    for (x, y), (vx, vy), p in zip(xy.tolist(), vxy.tolist(), pressure.tolist()):
        if not abs(x) < 1e300:
            continue
        n += 1
        s2 = vx * vx + vy * vy
        for name, term in zip(S.SUMS, (x, y, vx, vy, 0.5 * s2, p)):
            sums[name].append(term)
        lo_x, hi_x, lo_y, hi_y = lower(lo_x, x), higher(hi_x, x), lower(lo_y, y), higher(hi_y, y)
        top_speed2, top_p = higher(top_speed2, s2), higher(top_p, p)
        pressed += p > 0
        if n_bins:
            k = math.floor((x - x0) / w)
            if 0 <= k < n_bins:
                binned += 1
                count[k] += 1
                if y == y and y < top[k]:
                    top[k] = y
    row = [tick, n] + [math.fsum(sums[name]) if not any(t != t for t in sums[name]) else math.nan for name in S.SUMS] + \
          [lo_x, hi_x, lo_y, hi_y, top_speed2, top_p, pressed, binned]
    return np.array(row, dtype=np.float64), np.array(count, dtype=np.int32), np.array(top, dtype=np.float64)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_spec_against_the_naive_rule(cases, name):
    c = cases[name]
    pressure = np.random.RandomState(len(c.xy)).rand(len(c.xy)) * (np.arange(len(c.xy)) % 3 > 0)  # a third are zero
    want_row, want_count, want_top = naive(c.xy, c.vxy, pressure, 7, c.bins, *c.x_range)
    S.compare_row(S.row(c.xy, c.vxy, pressure, 7, c.bins, *c.x_range), c.xy, c.vxy, pressure, 7, c.bins, *c.x_range,
                  want=want_row)
    count, top = S.profile(c.xy, c.bins, *c.x_range)
    assert count.dtype == np.int32 and top.dtype == np.float64 and count.shape == top.shape == (c.bins,)
    assert np.array_equal(count, want_count) and np.array_equal(top, want_top)
    assert int(want_row[15]) == count.sum()


def test_the_tolerance_is_tight():
    """What the bound allows is a few thousand ulp of the sum at most, and a sum that is wrong by one term fails."""
    xy, vxy = K.cloud(3, 5000)
    p = np.random.RandomState(4).rand(5000)
    row = S.row(xy, vxy, p, 0)
    tol = S.tolerances(xy, vxy, p)
    for k, name in enumerate(S.SUMS):
        assert 0 < tol[name] < 2.5e-12 * np.abs(S.terms(xy, vxy, p)[name]).sum()
    S.compare_row(row, xy, vxy, p, 0)
    wrong = row.copy()
    wrong[2] -= np.abs(xy[:, 0]).min()
    with pytest.raises(AssertionError):
        S.compare_row(wrong, xy, vxy, p, 0)
    for k in (1, 8, 12, 14):  # the exact fields: one ulp is too much
        wrong = row.copy()
        wrong[k] = np.nextafter(wrong[k], np.inf)
        with pytest.raises(AssertionError):
            S.compare_row(wrong, xy, vxy, p, 0)


def test_sizes_are_the_ones_named(cases):
    block, threads = launch_sizes()
    assert [len(cases[n].xy) for n in ("empty", "one", "n63", "n64", "n65")] == [0, 1, 63, 64, 65]
    assert [len(cases[n].xy) for n in ("block-1", "block+0", "block+1")] == [block - 1, block, block + 1]
    assert len(cases["second_turn"].xy) == threads + 1
    assert {cases[n].bins for n in ("bins_1", "bins_1024", "no_bins")} == {1, 1024, 0}
    assert cases["sub_range"].x_range == (0.25, 0.75) and cases["edges_sub_range"].x_range == (0.25, 0.75)
    assert sum(c.tick for c in cases.values()) == 1 and len(cases["after_tick"].xy) == 400


def test_launch_sizes_are_the_kernels():
    from sand_crate_amd import _native as N
    from sand_crate_amd.engine import Engine
    text = (ROOT / "sand_crate_amd" / "csrc" / "sc_probe.h").read_text()
    assert int(re.search(r"kProbeBlock = (\d+);", text).group(1)) == N.PROBE_BLOCK
    assert int(re.search(r"kProbeBlocks = (\d+);", text).group(1)) == N.PROBE_BLOCKS
    assert Engine.PROBE_LAUNCH_THREADS == N.PROBE_BLOCK * N.PROBE_BLOCKS
    header = (ROOT / "include" / "sandcrate_hip.h").read_text()
    assert int(re.search(r"#define SC_PROBE_FIELDS (\d+)", header).group(1)) == N.PROBE_FIELDS == len(S.FIELDS)
    assert int(re.search(r"#define SC_PROBE_MAX_BINS (\d+)", header).group(1)) == N.PROBE_MAX_BINS == S.MAX_BINS


def test_empty_and_one(cases):
    r = S.as_dict(S.row(cases["empty"].xy, cases["empty"].vxy, None, 0, 8))
    assert r["n"] == 0 and r["min_x"] == r["min_y"] == math.inf and r["max_x"] == r["max_y"] == -math.inf
    assert r["max_speed2"] == r["max_p"] == r["sum_ke"] == 0.0
    count, top = S.profile(cases["empty"].xy, 8, 0.0, 1.0)
    assert not count.any() and np.isposinf(top).all()
    r = S.as_dict(S.row(cases["one"].xy, cases["one"].vxy, None, 3, 8))
    assert (r["tick"], r["n"], r["sum_x"], r["min_x"], r["max_x"], r["n_binned"]) == (3, 1, 0.3, 0.3, 0.3, 1)
    assert r["max_speed2"] == 0.25 * 0.25 + 1.5 * 1.5 and r["sum_ke"] == 0.5 * r["max_speed2"]


def test_one_bin_case(cases):
    c = cases["one_bin"]
    count, top = S.profile(c.xy, c.bins, *c.x_range)
    assert count[c.claims["bin"]] == len(c.xy) == count.sum()
    assert top[c.claims["bin"]] == c.claims["top"] < 0.1 and (c.xy[:, 1] == 0.1).sum() == 2
    assert np.isposinf(np.delete(top, c.claims["bin"])).all()


@pytest.mark.parametrize("name", ["edges", "edges_sub_range"])
def test_edge_particles_land_where_the_case_says(cases, name):
    c = cases[name]
    want = c.claims["bins"]
    assert np.array_equal(S.bins_of(c.xy[:, 0], c.bins, *c.x_range), want)
    assert want[0] == 0 and want[c.bins] == -1 and want[c.bins + 1] == c.bins - 1       # x0, x1, one ulp below x1
    assert (want[c.bins + 2:] == -1).all() and (want[:c.bins] >= 0).all()
    assert all(k - 1 <= b <= k for k, b in enumerate(want[:c.bins]))  # an edge falls into its bin or, rounded, the one below
    r = S.as_dict(S.row(c.xy, c.vxy, None, 0, c.bins, *c.x_range))
    assert r["n"] == len(c.xy) and r["n_binned"] == (want >= 0).sum() < r["n"]        # counted in the row, not in a bin


def test_not_finite_cases(cases):
    c = cases["inf_x"]
    r = S.as_dict(S.row(c.xy, c.vxy, None, 0, c.bins))
    assert np.isinf(c.xy[:, 0]).sum() == 1 and r["n"] == len(c.xy) - 1 and math.isfinite(r["sum_x"]) and r["max_x"] < 1
    c = cases["nan_velocity"]
    r = S.as_dict(S.row(c.xy, c.vxy, None, 0, c.bins))
    assert r["n"] == r["n_binned"] == len(c.xy)                      # it counts ...
    assert math.isnan(r["sum_vx"]) and math.isnan(r["sum_ke"]) and math.isnan(r["max_speed2"])  # ... and propagates
    assert math.isfinite(r["sum_vy"]) and math.isfinite(r["sum_x"])


def test_the_batch_holds_contraction_sensitive_pairs(cases):
    batch = K.contraction_batch()
    sensitive = K.contraction_sensitive(batch)
    assert 50 < sensitive.sum() < len(batch)
    c = cases["contraction"]
    assert len(c.vxy) == sensitive.sum() and K.contraction_sensitive(c.vxy).all()
    k = int(np.argmax(c.vxy[:, 0] ** 2 + c.vxy[:, 1] ** 2))
    vx, vy = c.vxy[k]
    exact = S.row(c.xy, c.vxy, None, 0)[12]
    assert exact == vx * vx + vy * vy and exact in (vx * vx + vy * vy,) and \
        (K.fma(vx, vx, vy * vy) != exact or K.fma(vy, vy, vx * vx) != exact)   # a contracted maximum is another number


def test_names_agree():
    from sand_crate_amd import probe
    assert probe.FIELDS == S.FIELDS and len(probe.FIELDS) == 16 and len(set(probe.FIELDS)) == 16
    assert probe.MAX_BINS == S.MAX_BINS
    import sand_crate_amd
    assert sand_crate_amd.probe is probe


def test_header_and_binding_list_the_calls():
    from sand_crate_amd import _native
    from sand_crate_amd.engine import Engine
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "sandcrate_hip.h").read_text(), flags=re.S)
    for name in ("sc_probe_now", "sc_probe_enable", "sc_probe_disable", "sc_probe_read"):
        assert re.search(rf"\bint {name}\s*\(", text) and name in _native.SIGNATURES
    for name in ("probe_now", "probe_enable", "probe_disable", "probe_read"):
        assert callable(getattr(Engine, name))
    assert "#define SC_ABI_VERSION 5" in text and "#define SC_NUM_KERNELS 12" in text


def test_library_exports_the_calls():
    import ctypes
    from sand_crate_amd import build
    lib = ctypes.CDLL(str(build.build()))
    for name in ("sc_probe_now", "sc_probe_enable", "sc_probe_disable", "sc_probe_read"):
        assert hasattr(lib, name)


def test_crate_surface():
    from sand_crate_amd import Crate
    p = inspect.signature(Crate.measure).parameters
    assert (p["bins"].default, p["x_range"].default) == (0, (0.0, 1.0))
    p = inspect.signature(Crate.observe).parameters
    assert (p["on"].default, p["capacity"].default, p["bins"].default, p["x_range"].default) == (True, 4096, 0, (0.0, 1.0))
    assert p["capacity"].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(Crate.observations)      # (that a growth keeps the log: tests/test_addons_cpu.py, by behaviour)


def test_concatenate_and_as_dict():
    from sand_crate_amd import probe
    rows = np.arange(32, dtype=np.float64).reshape(2, 16)
    a = probe.as_dict(rows, np.ones((2, 3), dtype=np.int32), np.zeros((2, 3)), dropped=1)
    b = probe.as_dict(rows[:1] + 100, np.ones((1, 3), dtype=np.int32), np.zeros((1, 3)), dropped=2)
    both = probe.concatenate([a, b], 3)
    assert both["dropped"] == 3 and both["count"].shape == (3, 3) and both["n"].tolist() == [1.0, 17.0, 101.0]
    none = probe.concatenate([], 4)
    assert none["dropped"] == 0 and none["count"].shape == (0, 4) and none["tick"].shape == (0,)
    one = probe.as_dict(rows[0])
    assert one["sum_x"] == 2.0 and "count" not in one and "dropped" not in one


# ---- the driver

class StubPlayback:
    made = []

    def __init__(self, config, recording_dir_path=None, **kw):
        self.kw = kw
        self.recording_dir_path = recording_dir_path
        self.seconds = 0.5
        self.crate = type("C", (), {"tick": 20, "particle_count": 123})()
        self.observables = {"sum_ke": np.array([2.0, 1.5]), "max_speed2": np.array([0.5, 0.25]), "n": np.array([120.0, 123.0])}
        StubPlayback.made.append(self)

    def run_live_simulation(self, ticks=None):
        self.ticks = ticks


def test_driver_accepts_observe(monkeypatch, capsys):
    from sand_crate_amd import main as M
    ap = M.argument_parser()
    assert ap.parse_args(["config/wave_machine.yaml"]).observe is None
    assert ap.parse_args(["config/wave_machine.yaml", "out", "--observe"]).observe == 0
    assert ap.parse_args(["config/wave_machine.yaml", "out", "--observe", "64", "--variants", "1"]).observe == 64
    assert inspect.signature(M.main).parameters["observe"].default is None
    assert inspect.signature(M.HeadlessPlayback.__init__).parameters["observe"].default is None

    monkeypatch.setattr(M, "HeadlessPlayback", StubPlayback)
    StubPlayback.made.clear()
    plain = M.main(ROOT / "config" / "wave_machine.yaml", None, variants=2, ticks=20)
    line = capsys.readouterr().out.splitlines()[0]
    assert [sorted(s) for s in plain] == [["coefficients", "particles", "seconds", "ticks", "variant"]] * 2
    assert line == "variant 0: 20 ticks, 123 particles, 0.50 s -> None"
    assert all("observe" not in p.kw for p in StubPlayback.made)
    seen = M.main(ROOT / "config" / "wave_machine.yaml", None, variants=1, ticks=20, observe=16)
    line = capsys.readouterr().out.splitlines()[0]
    assert StubPlayback.made[-1].kw["observe"] == 16
    assert (seen[0]["sum_ke"], seen[0]["max_speed2"], seen[0]["n"]) == (1.5, 0.25, 123.0)
    assert {k: seen[0][k] for k in plain[0]} == plain[0]
    assert line == "variant 0: 20 ticks, 123 particles, 0.50 s, sum_ke 1.5, max_speed2 0.25, n 123 -> None"
