"""GPU tests of the trajectory log (`Crate.record_trajectory`, sand_crate_amd/trajectory.py; sc_traj_* in
csrc/sc_traj.h).  The rule is tests/trajectory_spec.py, the worlds tests/trajectory_cases.py, their premises
tests/test_trajectory_cpu.py.

Expected frames come from the existing download path (`Engine.download()`) fed through the spec, never from the recorder,
and are compared byte for byte: the recording is a copy."""
import copy

import numpy as np
import pytest

import gpu_support as U
import growth_cases as G
import recovery_cases as rc
import trajectory_cases as K
import trajectory_spec as T
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu


def world(sc, max_particles=3000):
    return sc.WorldConfig(rigid_bodies=G.far_wall(), particle_sources=[], coefficients=G.lively(max_particles=max_particles))


def quiet_crate(sc, capacity=1024, **kw):
    return sc.Crate(world(sc, **kw), noise="counter", noise_seed=G.SEED, capacity=capacity)


def load(crate, xy, vxy, ids):
    import torch
    dev = torch.device("cuda", crate.engine.device)
    tensors = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (xy, vxy, np.asarray(ids, dtype=np.int64))]
    torch.cuda.current_stream(dev).synchronize()
    crate.load_state_tensors(*tensors)


def numpy_of(got):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}


def check_frame(got, k, crate, window, tick, where=""):
    """Frame k of what `read()` gave against the spec fed by the crate's download, as the state stands."""
    states, press, count, outside = T.frame_of_export(*crate.engine.download(), window[0], window[1] - window[0])
    U.same_bytes(got["states"][k], states, where)
    if "pressure" in got:
        U.same_bytes(got["pressure"][k], press, where)
    assert (got["ticks"][k], got["counts"][k], got["outside"][k]) == (tick, count, outside), where
    return states, count, outside


def check_log(got, log, where=""):
    """All of what `read()` gave against a spec log."""
    want = log.read()
    assert got["dropped"] == want["dropped"] and len(got["ticks"]) == len(want["ticks"]), where
    for name in ("states", "pressure", "ticks", "counts", "outside"):
        if name in want:
            U.same_bytes(got[name], want[name], f"{where}: {name}")


# ---------------------------------------------------------------- 1. rows at the edges
@pytest.mark.parametrize("rows", K.ROWS)
def test_rows_at_the_edges(sc, rows):
    """Windows one below, at and one above a wave and a workgroup of the clear; 0, 1 and 257 live particles; ids on both
    sides of both ends; before a tick (storage order is upload order, no pressure) and after one (cell-sorted)."""
    window = (K.EDGE_ID0, K.EDGE_ID0 + rows)
    crate = quiet_crate(sc)
    for n in K.LIVE_COUNTS:
        if n:
            load(crate, *K.edge_state(n, K.EDGE_ID0, rows))
        rec = crate.record_trajectory(2, ids=window, pressure=True)
        assert (rec.id0, rec.rows, rec.frames, rec.every) == (K.EDGE_ID0, rows, 2, 1)
        got = numpy_of(rec.read())
        assert got["states"].shape == (1, rows, 4) and got["ids"].tolist() == list(range(*window)) and got["dropped"] == 0
        states, count, outside = check_frame(got, 0, crate, window, crate.tick, f"n {n}")
        assert count == n and T.present(states).sum() == n - outside
        if n == 1:
            assert T.present(states).tolist() == [True] + [False] * (rows - 1) and outside == 0
        if n > 1:
            assert outside > 0 and T.present(states)[[0, -1]].all()
            U.same_bytes(got["pressure"][0][T.present(states)], np.zeros(n - outside))   # just loaded: no pressure yet
        crate.physics_tick()
        got = numpy_of(rec.read())
        assert got["states"].shape[0] == 2
        check_frame(got, 1, crate, window, crate.tick, f"n {n}, after a tick")
        U.same_bytes(got["positions"], got["states"][:, :, 0:2])
        U.same_bytes(got["velocities"], got["states"][:, :, 2:4])
    crate.close()


def test_ids_up_to_the_top(sc):
    xy, vxy, ids, window = K.top_state()
    crate = quiet_crate(sc)
    load(crate, xy, vxy, ids)
    rec = crate.record_trajectory(1, ids=window)
    got = numpy_of(rec.read())
    assert "pressure" not in got
    states, count, outside = check_frame(got, 0, crate, window, 0)
    assert (count, outside) == (len(ids), 5) and T.present(states)[[0, -1]].all() and T.present(states).sum() == 4
    crate.close()


def test_the_default_window_is_max_particles_not_the_capacity(sc):
    crate = quiet_crate(sc, capacity=64, max_particles=777)
    rec = crate.record_trajectory(1)
    assert (rec.id0, rec.rows) == (0, 777) and rec.read()["states"].shape == (1, 777, 4)
    crate.close()


# ---------------------------------------------------------------- 2. outsiders per wave
def test_outsiders_per_wave(sc):
    xy, vxy, ids = K.wave_state()
    crate = quiet_crate(sc)
    crate._set_state(xy, vxy)                                        # an upload: slot k holds id k
    for window in K.WAVE_WINDOWS:
        rec = crate.record_trajectory(1, ids=window)
        got = numpy_of(rec.read())
        _, count, outside = check_frame(got, 0, crate, window, 0, str(window))
        assert count == K.WAVE_COUNT and outside == sum(K.outsiders_per_wave(ids, window))
    crate.close()


# ---------------------------------------------------------------- 3. values that are not numbers
def test_values_that_are_not_numbers(sc):
    xy, vxy, live = K.odd_values()
    n = len(xy)
    crate = quiet_crate(sc)
    crate._set_state(xy, vxy)
    rec = crate.record_trajectory(1, ids=(0, n), pressure=True)
    got = numpy_of(rec.read())
    states, count, outside = check_frame(got, 0, crate, (0, n), 0)
    assert (count, outside) == (int(live.sum()), 0) and T.present(got["states"][0]).tolist() == live.tolist()
    # ... and against the spec from the arrays as they were stored
    want = T.frame(xy[:, 0], xy[:, 1], vxy[:, 0], vxy[:, 1], np.zeros(n), np.arange(n), n, 0, False, 0, n)
    U.same_bytes(got["states"][0], want[0])
    U.same_bytes(got["pressure"][0], want[1])
    absent = got["states"][0][~live]
    assert (np.ascontiguousarray(absent).view(np.uint64) == T.FILL_BITS).all()
    assert (np.ascontiguousarray(got["pressure"][0][~live]).view(np.uint64) == T.FILL_BITS).all()
    import torch
    assert rec.present(rec.read()["states"]).cpu().numpy().tolist() == [live.tolist()]
    assert rec.complete_rows(rec.read()["states"]).cpu().numpy().tolist() == np.flatnonzero(live).tolist()
    assert isinstance(rec.read()["states"], torch.Tensor) and rec.read()["states"].is_cuda
    crate.close()


# ---------------------------------------------------------------- 4. a run
def make_run_crate(sc, case, capacity):
    wc = sc.WorldConfig(rigid_bodies=copy.deepcopy(case.bodies), particle_sources=copy.deepcopy(case.sources),
                        coefficients=copy.deepcopy(case.coef))
    return sc.Crate(wc, noise="counter", noise_seed=G.SEED, capacity=capacity)     # (seeds np.random, crate.py:22)


def run_tick(crate, case):
    flows = case.flows_at(crate.tick)
    if flows is not None:
        for s, f in zip(crate.particle_sources, flows):
            s.flow = f
    crate.physics_tick()


def final_state(crate):
    return tuple(crate.engine.download()) + tuple(t.cpu().numpy() for t in crate.state_tensors(ids=True))


def recorded_run(sc, case, capacity, every, ticks, downloads, frames=None):
    """The case for `ticks` ticks on a crate that records; with `downloads` a spec log is fed from `Engine.download()`
    after every tick that is due.  -> (crate, the recording, the spec log or None)."""
    crate = make_run_crate(sc, case, capacity)
    lo, hi = K.RUN_WINDOW
    frames = ticks // every + 1 if frames is None else frames
    rec = crate.record_trajectory(frames, ids=K.RUN_WINDOW, every=every, pressure=True)
    log = T.Log(frames, lo, hi - lo) if downloads else None
    if downloads:
        log.take(0, crate.engine.download())
    for _ in range(ticks):
        run_tick(crate, case)
        if downloads and T.due(crate.tick, every):
            log.take(crate.tick, crate.engine.download())
    return crate, rec, log


@pytest.fixture()
def no_reads(monkeypatch):
    """While armed: no download, no export, no synchronisation of the library's stream or of torch.  (The crate's own
    8-byte count for sources drawn on the host, `Engine.count`, is part of such a tick with or without a recording.)"""
    import torch
    from sand_crate_amd.engine import Engine
    armed = [False]

    def guard(real, name):
        def call(*args, **kw):
            assert not armed[0], f"{name} was called while the twin recorded"
            return real(*args, **kw)
        return call

    for owner, name in ((Engine, "download"), (Engine, "synchronize"), (Engine, "export_state"), (torch.cuda, "synchronize"),
                        (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.cuda.Stream, "synchronize")):
        monkeypatch.setattr(owner, name, guard(getattr(owner, name), name))
    return armed


@pytest.mark.parametrize("every", K.EVERYS)
def test_a_run_with_gaps_in_the_ids(sc, every, no_reads):
    case = K.run_case()
    # the crate that downloads after every tick: its log is the spec's
    crate, rec, log = recorded_run(sc, case, case.ample, every, K.RUN_TICKS, downloads=True)
    got = numpy_of(rec.read())
    assert got["ticks"].tolist() == list(range(0, K.RUN_TICKS + 1, every)) and got["dropped"] == 0
    check_log(got, log, f"every {every}")
    assert got["counts"][0] == 0 and got["outside"][-1] > 0 and got["counts"][-1] > got["outside"][-1]
    inside = T.present(got["states"][-1])
    assert 0 < inside.sum() < len(inside) and not inside[: inside.nonzero()[0][-1]].all()   # gaps
    assert np.any(got["pressure"][-1][inside] != 0.0)
    want_final = final_state(crate)
    crate.close()
    # a twin that reads nothing until `read()`
    twin, twin_rec, _ = recorded_run(sc, case, case.ample, every, 0, downloads=False, frames=K.RUN_TICKS // every + 1)
    no_reads[0] = True
    try:
        for _ in range(K.RUN_TICKS):
            run_tick(twin, case)
    finally:
        no_reads[0] = False
    twin_got = numpy_of(twin_rec.read())
    for name in ("states", "pressure", "ticks", "counts", "outside"):
        U.same_bytes(twin_got[name], got[name], f"twin, every {every}: {name}")
    assert twin_got["dropped"] == 0
    twin_final = final_state(twin)
    twin.close()
    # ... and a third that never recorded: recording changes nothing
    plain = make_run_crate(sc, case, case.ample)
    for _ in range(K.RUN_TICKS):
        run_tick(plain, case)
    for a, b, c in zip(final_state(plain), twin_final, want_final):
        U.same_bytes(a, b)
        U.same_bytes(a, c)
    plain.close()


def test_recording_through_run(sc):
    """`Crate.run`: the ticks promise their successors' inputs; a recorded tick is not fused, and the frames are those of
    ticking one by one."""
    xy, vxy = K.tk.cloud(5, 300)
    logs = []
    for path in ("run", "physics_tick"):
        crate = quiet_crate(sc)
        crate._set_state(xy, vxy)
        rec = crate.record_trajectory(8, ids=(0, 300), every=2)
        if path == "run":
            crate.run(9)
        else:
            for _ in range(9):
                crate.physics_tick()
        got = numpy_of(rec.read())
        assert got["ticks"].tolist() == [0, 2, 4, 6, 8]
        logs.append((got, crate.engine.download()))
        crate.close()
    for name in ("states", "ticks", "counts", "outside"):
        U.same_bytes(logs[0][0][name], logs[1][0][name], name)
    for a, b in zip(logs[0][1], logs[1][1]):
        U.same_bytes(a, b)


# ---------------------------------------------------------------- 5. the log's bounds
def test_a_full_log_drops_and_counts_and_restarts(sc):
    xy, vxy = K.tk.cloud(6, 300, lo=0.45, hi=0.55)                   # (dense: the pressures are not all zero)
    window = (10, 290)
    crate = quiet_crate(sc)
    crate._set_state(xy, vxy)
    rec = crate.record_trajectory(3, ids=window, pressure=True, initial=False)
    assert len(rec.read()["ticks"]) == 0                             # initial=False: no frame 0
    log = T.Log(3, window[0], window[1] - window[0])
    for _ in range(5):
        crate.physics_tick()
        log.take(crate.tick, crate.engine.download())
    got = numpy_of(rec.read())
    assert got["dropped"] == 2 and got["ticks"].tolist() == [1, 2, 3]
    check_log(got, log, "full")                                      # frames 0..2 untouched by the dropped ones
    again = numpy_of(rec.read())                                     # reading does not restart
    assert again["dropped"] == 2
    for name in ("states", "pressure", "ticks", "counts", "outside"):
        U.same_bytes(again[name], got[name], name)
    rec.capture()                                                    # on demand into a full log: dropped as well
    assert rec.read()["dropped"] == 3 and len(rec.read()["ticks"]) == 3
    rec.restart()
    log.restart()
    assert len(rec.read()["ticks"]) == 0 and rec.read()["dropped"] == 0
    for _ in range(2):
        crate.physics_tick()
        log.take(crate.tick, crate.engine.download())
    got = numpy_of(rec.read())
    assert got["ticks"].tolist() == [6, 7]
    check_log(got, log, "restarted")
    # a state just loaded shows zero pressure in a captured frame
    state = crate.state_tensors(ids=True)
    crate.load_state_tensors(state[0], state[1], state[3])
    rec.capture()
    got = numpy_of(rec.read())
    assert got["ticks"].tolist() == [6, 7, 7]
    states, _, _ = check_frame(got, 2, crate, window, 7)
    assert T.present(states).sum() > 200 and not got["pressure"][2][T.present(states)].any()
    assert got["pressure"][1][T.present(got["states"][1])].any()
    # stop: what was recorded stays readable; the crate records no more
    crate.stop_trajectory()
    assert not rec.recording
    crate.physics_tick()
    assert numpy_of(rec.read())["ticks"].tolist() == [6, 7, 7]
    with pytest.raises(RuntimeError):
        rec.capture()
    crate.close()


def test_a_second_recording_replaces_the_first(sc):
    xy, vxy = K.tk.cloud(8, 100)
    crate = quiet_crate(sc)
    crate._set_state(xy, vxy)
    first = crate.record_trajectory(4, ids=(0, 100))
    crate.physics_tick()
    second = crate.record_trajectory(4, ids=(50, 120), initial=False)
    assert not first.recording and second.recording
    crate.physics_tick()
    assert numpy_of(first.read())["ticks"].tolist() == [0, 1]
    got = numpy_of(second.read())
    assert got["ticks"].tolist() == [2]
    check_frame(got, 0, crate, (50, 120), 2)
    crate.close()


def test_an_abandoned_tick_leaves_no_frame(sc):
    from sand_crate_amd import _native as N
    from sand_crate_amd.load_config import WorldConfig
    p, v = rc.quiet()
    crate = sc.Crate(WorldConfig([copy.deepcopy(rc.BOX)], [], copy.deepcopy(rc.COEF)), noise="counter", noise_seed=77,
                     capacity=rc.capacity(len(p)))
    crate._set_state(p, v)
    window = (100, 5000)
    rec = crate.record_trajectory(16, ids=window, pressure=True, initial=False)
    log = T.Log(16, window[0], window[1] - window[0])

    def good(k):
        for _ in range(k):
            crate.physics_tick()
            log.take(crate.tick, crate.engine.download())

    good(rc.GOOD_BEFORE)
    crate.engine.set_scan_patience(-1)  # every workgroup of the scan but the first gives up without having looked
    for _ in range(rc.ABANDONED):
        crate.physics_tick()
    crate.engine.set_scan_patience(1 << 22)
    with pytest.raises(N.NativeError) as e:
        crate.synchronize()
    assert e.value.code == N.ERR_HIP and "skipped" in str(e.value)
    good(rc.GOOD_AFTER)
    got = numpy_of(rec.read())
    assert got["ticks"].tolist() == [1, 2, 5, 6, 7] and got["dropped"] == 0
    check_log(got, log, "abandoned")
    crate.close()


# ---------------------------------------------------------------- 6. growth
def test_growth_keeps_the_recording(sc):
    """From capacity 16 the crate outgrows its context twice while it records: frames, ticks, the phase of `every` and
    the cursor carry over, and the log is the one of a twin with ample room."""
    case = K.run_case()
    logs = []
    for capacity in case.capacities:
        crate = make_run_crate(sc, case, capacity)
        rec = crate.record_trajectory(case.ticks // 3 + 1, ids=K.RUN_WINDOW, every=3, pressure=True)
        engines = [crate.engine]
        for _ in range(case.ticks):
            run_tick(crate, case)
            if crate.engine is not engines[-1]:
                engines.append(crate.engine)
        logs.append((numpy_of(rec.read()), len(engines), final_state(crate)))
        assert rec.recording
        crate.close()
    (grown, contexts, final), (twin, twin_contexts, twin_final) = logs
    assert (contexts, twin_contexts) == (3, 1)
    assert grown["ticks"].tolist() == list(range(0, case.ticks + 1, 3)) and grown["dropped"] == twin["dropped"] == 0
    assert grown["counts"][-1] > 200
    for name in ("states", "pressure", "ticks", "counts", "outside"):
        U.same_bytes(grown[name], twin[name], name)
    for a, b in zip(final, twin_final):
        U.same_bytes(a, b)


# ---------------------------------------------------------------- 7. refusals
def log_tensors(sc, frames, rows, device=0, sentinel=-7):
    import torch
    dev = torch.device("cuda", device)
    return dict(states=torch.full((frames, rows, 4), float(sentinel), dtype=torch.float64, device=dev), pressure=None,
                ticks=torch.full((frames,), sentinel, dtype=torch.int64, device=dev),
                counts=torch.full((frames,), sentinel, dtype=torch.int64, device=dev),
                outside=torch.full((frames,), sentinel, dtype=torch.int64, device=dev),
                words=torch.full((4,), sentinel, dtype=torch.int64, device=dev))


def enable(eng, t, **kw):
    eng.traj_enable(t["states"], t["pressure"], t["ticks"], t["counts"], t["outside"], t["words"], **kw)


def log_untouched(t, sentinel=-7):
    import torch
    torch.cuda.synchronize()
    return U.untouched(*(v for v in t.values() if v is not None), sentinel=sentinel)


def test_refused_inside_a_tick_and_the_recording_goes_on(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(sc.load_config("config/wave_machine.yaml").world_config, noise="host-sync")
    crate.physics_tick()
    eng = crate.engine
    rec = crate.record_trajectory(4, ids=(0, 64), initial=False)
    other = log_tensors(sc, 2, 8)
    torch.cuda.synchronize()
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        assert U.code_of(enable, eng, other, id0=0) == N.ERR_STATE
        assert U.code_of(eng.traj_capture) == N.ERR_STATE
        assert U.code_of(eng.traj_disable) == N.ERR_STATE
        stats = eng.step_stats()
        eng.set_noise_host(np.random.rand(stats.neighbor_slots, 2))
    finally:
        eng.step_finish()
    crate._state_changed()
    got = numpy_of(rec.read())                                       # the refused calls left the recording on, into its log
    assert got["ticks"].tolist() == [2] and log_untouched(other)
    check_frame(got, 0, crate, (0, 64), 2)
    crate.close()


def test_refused_after_a_promised_tick_and_in_slab_mode(sc):
    import torch
    from sand_crate_amd import _native as N
    crate = sc.Crate(sc.load_config("config/wave_machine.yaml").world_config, noise="counter")
    crate.physics_tick()
    eng = crate.engine
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    now = crate._pack_tick_inputs()
    for body in crate.rigid_bodies:
        body.apply_velocity(crate.dt)
    nxt = crate._pack_tick_inputs()
    log = log_tensors(sc, 2, 8)
    torch.cuda.synchronize()
    eng.tick(now, nxt)
    assert U.code_of(enable, eng, log, id0=0) == N.ERR_STATE
    assert U.code_of(eng.traj_disable) == N.ERR_STATE
    assert U.code_of(eng.traj_capture) == N.ERR_STATE                  # (it is not on)
    assert log_untouched(log)
    eng.tick(nxt)
    enable(eng, log, id0=0)                                          # the promise is kept: now it can
    eng.tick(nxt)
    eng.synchronize()
    assert log["words"].cpu().tolist()[:3] == [1, 0, 0] and log["ticks"].cpu().tolist()[0] == 4
    eng.traj_disable()
    eng.traj_disable()                                               # (off twice is fine)
    # the arguments the library checks itself
    for bad in (dict(id0=-1), dict(id0=0, every=0)):
        with pytest.raises(ValueError):
            enable(eng, log, **bad)
    lib, ctx, p = eng._lib, eng._ctx, lambda t: N._P(t.data_ptr())
    t = log
    ok = (p(t["states"]), None, p(t["ticks"]), p(t["counts"]), p(t["outside"]), p(t["words"]))
    for frames, id0, rows, every in ((0, 0, 8, 1), (2, -1, 8, 1), (2, 0, 0, 1), (2, 2 ** 31 - 8, 8, 1), (2, 0, 8, 0)):
        assert lib.sc_traj_enable_device(ctx, *ok, frames, id0, rows, every, 1) == N.ERR_ARG, (frames, id0, rows, every)
    for k in (0, 2, 3, 4, 5):
        args = list(ok)
        args[k] = None
        assert lib.sc_traj_enable_device(ctx, *args, 2, 0, 8, 1, 1) == N.ERR_ARG, k
    assert lib.sc_traj_enable_device(ctx, N._P(t["states"].data_ptr() + 8), *ok[1:], 1, 0, 8, 1, 1) == N.ERR_ARG
    assert U.code_of(eng.traj_capture) == N.ERR_STATE                  # none of them switched it on
    crate.close()
    # slab mode
    eng = sc.Engine(capacity=64)
    xy, vxy = K.tk.cloud(1, 20)
    eng.upload(xy, vxy)
    log = log_tensors(sc, 2, 8)
    torch.cuda.synchronize()
    enable(eng, log, id0=0)
    eng.set_slab(0, 10, 3, False, False)
    for call, args, kw in ((enable, (eng, log), dict(id0=0)), (eng.traj_capture, (), {}), (eng.traj_disable, (), {})):
        assert U.code_of(call, *args, **kw) == N.ERR_STATE
        assert eng.count() == 20                                     # the context is fine
    eng.synchronize()
    assert log["words"].cpu().tolist() == [0, 0, 0, 0] and log_untouched({k: v for k, v in log.items() if k != "words"})
    eng.close()


# ---------------------------------------------------------------- the driver
def test_driver_writes_trajectory_npz(sc, tmp_path):
    from pathlib import Path
    from sand_crate_amd.main import main
    root = Path(__file__).resolve().parent.parent
    main(root / "config" / "wave_machine.yaml", tmp_path, variants=1, ticks=40, trajectory=10, record_every=10)
    variant = tmp_path / "variant_00"
    with np.load(variant / "trajectory.npz") as z, np.load(variant / "state.npz") as state:
        assert sorted(z.files) == ["counts", "dropped", "id0", "outside", "states", "ticks"]
        assert z["ticks"].tolist() == [0, 10, 20, 30, 40] and int(z["dropped"]) == 0 and int(z["id0"]) == 0
        assert z["states"].shape == (5, 4000, 4) and z["counts"][0] == 0 and not z["outside"].any()
        for k in range(4):                                           # state.npz holds the same ticks' positions, by rank
            live = T.present(z["states"][k + 1])
            assert int(state["ticks"][k]) == z["ticks"][k + 1] and live.sum() == z["counts"][k + 1]
            U.same_bytes(z["states"][k + 1][live][:, 0:2], state[f"particles_{k}"])
