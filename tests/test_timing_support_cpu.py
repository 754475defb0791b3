"""The measuring protocol the timing scripts share (scripts/timing_support.py): what `stats` reports, the order in which
`alternate` calls its cases, and when `use_library` points the package at another build.  No GPU, no library loaded."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "scripts"))

import timing_support as T  # noqa: E402
from sand_crate_amd import _native  # noqa: E402


def test_stats_reports_the_upper_median_and_the_minimum_to_two_digits():
    times = [40.126, 10.004, 30.0, 20.555]                                           # sorted: element 4 // 2 is 30.0
    assert T.stats(times) == {"median_us": 30.0, "min_us": 10.0}
    assert T.stats(times, "wall_") == {"wall_median_us": 30.0, "wall_min_us": 10.0}
    assert T.stats([3.14159, 2.71828, 1.41421]) == {"median_us": 2.72, "min_us": 1.41}
    assert times == [40.126, 10.004, 30.0, 20.555]                                   # (the caller's list is left as it was)
    assert T.median(times) == 30.0


def test_stats_serves_the_variants_of_the_scripts():
    times = [40.126, 10.004, 30.0, 20.5554]
    assert T.stats(times, "d_", maximum=True) == {"d_median_us": 30.0, "d_min_us": 10.0, "d_max_us": 40.13}
    assert T.stats(times, digits=3) == {"median_us": 30.0, "min_us": 10.004}
    assert T.stats(times, "ticks_per_s_", 1, maximum=True, unit="") == {
        "ticks_per_s_median": 30.0, "ticks_per_s_min": 10.0, "ticks_per_s_max": 40.1}


def test_alternate_warms_up_first_then_runs_each_case_once_per_repetition_in_order(monkeypatch):
    calls = []
    cases = {"b": lambda: calls.append("b"), "a": lambda: calls.append("a"), "c": lambda: calls.append("c")}
    clock = iter(range(1000))
    monkeypatch.setattr(T.time, "perf_counter", lambda: next(clock))                 # every recorded call "takes" 1 s
    out = T.alternate(cases, reps=4, warmup=2)
    assert calls == ["b", "a", "c"] * 6
    assert list(out) == ["b", "a", "c"]
    assert all(series == [1e6] * 4 for series in out.values())                       # reps samples each, the warm-up unrecorded
    assert next(clock) == 2 * 3 * 4                                                  # ... and untimed: two readings per sample


def test_alternate_without_warm_up_records_every_call():
    calls = []
    out = T.alternate({"only": lambda: calls.append(1)}, reps=3, warmup=0)
    assert len(calls) == 3 and len(out["only"]) == 3 and all(t >= 0 for t in out["only"])


def test_with_wall_appends_one_time_per_call():
    into, calls = [], []
    run = T.with_wall(lambda: calls.append(1), into)
    run()
    run()
    assert len(calls) == 2 and len(into) == 2 and all(t >= 0 for t in into)


def test_use_library_without_a_path_changes_nothing(monkeypatch):
    monkeypatch.delenv(T.LIB_ENV, raising=False)
    monkeypatch.setattr(_native, "_lib", None)
    before = _native.LIB_PATH
    assert T.use_library(None) is None and T.use_library() is None and T.use_library("") is None
    assert _native.LIB_PATH == before


def test_use_library_sets_the_resolved_path(monkeypatch, tmp_path):
    monkeypatch.delenv(T.LIB_ENV, raising=False)
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", _native.LIB_PATH)                       # (put back afterwards)
    monkeypatch.chdir(tmp_path)
    assert T.use_library("variants/../other.so") == tmp_path.resolve() / "other.so"
    assert _native.LIB_PATH == tmp_path.resolve() / "other.so"


def test_use_library_honours_the_environment_and_the_argument_wins(monkeypatch, tmp_path):
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", _native.LIB_PATH)
    monkeypatch.setenv(T.LIB_ENV, str(tmp_path / "from_env.so"))
    assert T.use_library() == (tmp_path / "from_env.so").resolve()
    assert T.use_library(str(tmp_path / "from_arg.so")) == (tmp_path / "from_arg.so").resolve()
    assert _native.LIB_PATH == (tmp_path / "from_arg.so").resolve()


def test_use_library_raises_once_a_library_is_loaded(monkeypatch, tmp_path):
    monkeypatch.delenv(T.LIB_ENV, raising=False)
    monkeypatch.setattr(_native, "_lib", object())
    before = _native.LIB_PATH
    with pytest.raises(RuntimeError, match="already loaded"):
        T.use_library(str(tmp_path / "late.so"))
    assert _native.LIB_PATH == before
    assert T.use_library(None) is None                                               # (nothing asked for: nothing to refuse)
