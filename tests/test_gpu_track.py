"""GPU tests of the tracker (sc_track_*, `Engine.track_*`, `Crate.capture_frame` / `track` / `tracked`, `track.Player`,
`main --track`, `replay`): a captured frame equals tests/track_spec.py applied to the downloaded state -- in canonical
form, records by id --, the log holds byte for byte what capturing after every tick returns, logging changes no result,
a full log drops whole frames and counts them, the log survives a grown engine, a loaded frame is exactly what
`track.parse` reads and renders exactly as the render, GIF, JPEG and text specs say, and bad frames are refused.

Pressures cannot be uploaded -- the device computes them -- so the colour rule is checked on the device by ticked
states, by particles appended behind them, and by a round trip of all 256 colour bytes through sc_track_load; the edge
pressures of track_cases.py (NaN, the infinities, the neighbours of k / 255) are the spec's business in
test_track_cpu.py.  Coordinates that are not finite cannot be downloaded (sc_download_state skips them): those cases are
compared with the spec applied to the uploaded arrays, which is what a download would return."""
import struct
from pathlib import Path

import numpy as np
import pytest

import gif_spec as G
import gpu_support as U
import jpeg_spec as J
import render_spec as R
import text_spec as T
import track_cases as K
import track_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def world(sc, n, bodies=None, sources=False):
    """wave_machine's coefficients with discs sized for n particles; `bodies` replaces its walls."""
    wc = U.spread_world(sc, n, least=64)                                   # (a handful of particles keep sensible discs)
    if sources:
        wc.particle_sources = U.scene(sc).particle_sources                # (a fresh load: nobody else's)
    if bodies is not None:
        wc.rigid_bodies = bodies
    return wc


def crate_of(sc, xy, vxy=None, bodies=None, noise="counter", **kw):
    n = len(xy)
    crate = sc.Crate(world(sc, n, bodies), noise=noise, noise_seed=1, capacity=kw.pop("capacity", n + 64), **kw)
    crate.particles = xy
    crate.particle_velocities = np.zeros_like(xy) if vxy is None else vxy
    return crate


def segments_of(crate):
    return crate.segments if crate.rigid_bodies else np.zeros((0, 2, 2))


def spec_pack(crate, valid_slots=None):
    """track_spec.pack of what the engine downloads and the walls as they stand."""
    xy, _, pressure, ids = crate.engine.download()
    return S.pack(crate.tick, xy, pressure, ids, segments_of(crate), pressure_valid=crate.tick > 0, valid_slots=valid_slots)


def check_capture(crate, want=None):
    got = crate.capture_frame()
    want = spec_pack(crate) if want is None else want
    assert len(got) == len(want) == crate.engine.track_bound(S.header(got)["n"], S.header(got)["n_segments"])
    assert S.canonical(got) == S.canonical(want)
    assert crate.capture_frame() == got                                     # the same state twice: the same bytes
    return got


# ---- a captured frame is the spec's

@pytest.mark.parametrize("n", K.COUNTS)
def test_every_count_before_and_after_a_tick(sc, n):
    xy, vxy = K.cloud(n + 1, n)
    crate = crate_of(sc, xy, vxy)
    frame = check_capture(crate)                                           # before the first tick: no valid pressure
    p = S.parse(frame)
    assert p["tick"] == 0 and p["flags"] == 0 and p["n"] == n and (p["c"] == 255).all() and len(p["segments"]) == 8
    assert p["ids"].tolist() == list(range(n))                             # (an upload stores in id order)
    crate.physics_tick()
    frame = check_capture(crate)
    p = S.parse(frame)
    assert p["tick"] == 1 and p["flags"] == 1 and p["n"] == n == crate.particle_count
    assert np.array_equal(p["segments"], crate.segments)                   # the motored wall where the tick put it
    if n >= 255:
        assert len(set(p["c"].tolist())) > 1                               # (pressures differ: the colour plane is alive)
        assert sorted(p["ids"].tolist()) == list(range(n)) and p["ids"].tolist() != list(range(n))   # cell-sorted order


def test_coordinate_cases(sc):
    coords = K.coordinates()
    other = np.resize(K.finite_coordinates()[::-1], len(coords))
    for xy in (np.stack([coords, other], axis=1), np.stack([other, coords], axis=1)):
        crate = crate_of(sc, xy)
        want = S.pack(0, xy, np.zeros(len(xy)), np.arange(len(xy)), crate.segments, pressure_valid=False)
        p = S.parse(check_capture(crate, want))
        assert p["n"] == len(xy)                                            # (slots that are not finite are stored, and coded)
        assert (p["qx"] == 65535).sum() == (~np.isfinite(xy[:, 0])).sum() and (p["qy"] == 65535).sum() == (~np.isfinite(xy[:, 1])).sum()
    finite = K.finite_coordinates()
    xy = np.stack([finite, finite[::-1]], axis=1)
    crate = crate_of(sc, xy)
    check_capture(crate)                                                   # all finite: against the download itself
    assert np.array_equal(crate.engine.download()[0], xy)


@pytest.mark.parametrize("n_segments", K.SEGMENT_COUNTS)
def test_segment_counts(sc, n_segments):
    xy, vxy = K.cloud(5, 65)
    crate = crate_of(sc, xy, vxy, bodies=K.wall_bodies(n_segments))
    p = S.parse(check_capture(crate))
    assert p["segments"].shape == (n_segments, 2, 2) and np.array_equal(p["segments"], segments_of(crate))
    crate.physics_tick()
    p = S.parse(check_capture(crate))
    assert p["segments"].shape == (n_segments, 2, 2) and p["tick"] == 1


def test_sparse_ids(sc):
    n = 257
    xy, vxy = K.cloud(9, n)
    ids = K.sparse_ids(4, n)
    crate = crate_of(sc, xy, vxy)
    crate.engine.upload_with_ids(xy, vxy, ids)
    crate._state_changed()
    p = S.parse(check_capture(crate))
    assert p["ids"].tolist() == ids.tolist() and p["ids"].max() == 1_000_000 and (p["ids"] > 65_536).sum() > 200
    crate.physics_tick()
    p = S.parse(check_capture(crate))
    assert sorted(p["ids"].tolist()) == sorted(ids.tolist())


def test_appended_behind_ticked_ones(sc):
    xy, vxy = K.cloud(12, 300)
    crate = crate_of(sc, xy, vxy, capacity=1024)
    crate.physics_tick()
    more, more_v = K.cloud(13, 70)
    crate.engine.append(more, more_v)
    crate._state_changed()
    _, _, pressure, ids = crate.engine.download()
    assert (pressure[ids < 300] > 0).any() and (pressure[ids >= 300] == 0).all()
    p = S.parse(check_capture(crate, spec_pack(crate, valid_slots=ids < 300)))
    assert p["n"] == 370 and p["flags"] == 1 and (p["c"][p["ids"] >= 300] == 255).all() and (p["c"][p["ids"] < 300] < 255).any()


def test_after_ticks_that_removed_particles(sc):
    xy, vxy = K.cloud(14, 400)
    xy[::7, 0] = 1.3                                                        # outside the crate: the first tick removes them
    crate = crate_of(sc, xy, vxy)
    assert S.parse(crate.capture_frame())["n"] == 400
    for _ in range(3):
        crate.physics_tick()
    p = S.parse(check_capture(crate))
    gone = len(range(0, 400, 7))
    assert p["n"] == crate.particle_count <= 400 - gone and not set(p["ids"].tolist()) & set(range(0, 400, 7))
    assert p["n"] >= 400 - gone - 8                                         # (the ticks themselves may push a few more out)


def test_all_colour_bytes_round_trip_through_load(sc):
    from sand_crate_amd import track
    n = 256
    xy = np.stack([np.linspace(0.1, 0.9, n), np.linspace(0.9, 0.1, n)], axis=1)
    frame = bytearray(S.pack(5, xy, S.pressure_of(np.arange(n)), np.arange(n), K.walls(1)))
    eng = sc.Engine(capacity=n)
    eng.track_load(bytes(frame))
    _, _, pressure, _ = eng.download()
    assert np.array_equal(pressure, S.pressure_of(np.arange(n)))
    again = S.parse(eng.track_capture())
    assert again["c"].tolist() == list(range(n)) and again["flags"] == 1 and again["n"] == n
    assert np.array_equal(again["qx"], S.parse(bytes(frame))["qx"]) and np.array_equal(again["qy"], S.parse(bytes(frame))["qy"])
    assert track.parse(bytes(frame))["colour"].tolist() == list(range(n))
    eng.close()


# ---- the log

def wave_crate(sc, noise="counter"):
    """A small scene with a motored wall and an active source."""
    wc = world(sc, 600, sources=True)
    wc.particle_sources[0]["flow"] = 3000
    crate = sc.Crate(wc, noise=noise, noise_seed=3, capacity=2048)
    xy, vxy = K.cloud(21, 300, 0.1, 0.9)
    crate.particles = xy
    crate.particle_velocities = vxy
    return crate


def same_state(a, b):
    for x, y in zip(a.engine.download(), b.engine.download()):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()


def ticked(sc, noise, ticks=12, track=None, capture=False):
    """A wave_crate run for `ticks` ticks, alone: with noise "counter" the source draws from the host's global stream,
    which `Crate()` seeds, so two crates that are to see the same particles must not take turns."""
    crate = wave_crate(sc, noise)
    if track is not None:
        crate.track(**track)
    captured = []
    for _ in range(ticks):
        crate.physics_tick()
        if capture:
            captured.append(crate.capture_frame())
    return crate, captured


@pytest.mark.parametrize("noise", ["host", "counter"])
def test_log_equals_capturing_after_every_tick_and_changes_nothing(sc, noise):
    assert wave_crate(sc, noise).tracked() == ([], 0)
    logged, captured = ticked(sc, noise, track=dict(capacity_bytes=1 << 20), capture=True)
    frames, dropped = logged.tracked()
    assert dropped == 0 and len(frames) == 12 and frames == captured       # byte for byte
    assert [S.header(f)["tick"] for f in frames] == list(range(1, 13))
    counts = [S.header(f)["n"] for f in frames]
    assert counts[-1] > counts[0] >= 300                                    # (the source is active)
    assert len({S.parse(f)["segments"].tobytes() for f in frames}) == 12    # (the wall moves)
    assert S.canonical(frames[-1]) == S.canonical(spec_pack(logged))
    plain, _ = ticked(sc, noise)
    same_state(logged, plain)                                              # the log changes no result
    assert logged.tracked() == ([], 0)                                     # read and rewound
    logged.physics_tick()
    frames, _ = logged.tracked()
    assert [S.header(f)["tick"] for f in frames] == [13]
    logged.track(False)
    logged.physics_tick()
    assert logged.tracked() == ([], 0)


def test_every_third_tick(sc):
    crate, _ = ticked(sc, "counter", track=dict(every=3, capacity_bytes=1 << 20))
    frames, dropped = crate.tracked()
    assert dropped == 0 and [S.header(f)["tick"] for f in frames] == [3, 6, 9, 12]
    _, captured = ticked(sc, "counter", capture=True)
    assert frames == [captured[t - 1] for t in (3, 6, 9, 12)]


def test_log_through_run(sc):
    def make():
        xy, vxy = K.cloud(22, 400)
        return crate_of(sc, xy, vxy)
    logged, single, plain = make(), make(), make()
    logged.track(capacity_bytes=1 << 20)
    logged.run(12)
    plain.run(12)
    captured = []
    for _ in range(12):
        single.physics_tick()
        captured.append(single.capture_frame())
    frames, dropped = logged.tracked()
    assert dropped == 0 and frames == captured
    same_state(logged, plain)                                              # run() with the log on: the same state, bit for bit
    same_state(logged, single)


def boxed(sc, n=400):
    """Walls all round and no source: the particle count cannot change."""
    xy, vxy = K.cloud(23, n, 0.1, 0.9, speed=0.02)
    return crate_of(sc, xy, vxy, bodies=K.box_bodies())


def test_a_full_log_drops_whole_frames_and_counts(sc):
    n, s = 400, 4
    crate = boxed(sc, n)
    size = S.frame_bytes(n, s)
    crate.track(capacity_bytes=2 * size + 1)
    for _ in range(5):
        crate.physics_tick()
    assert crate.particle_count == n, "the world was to keep its particles: the test's sizes no longer hold"
    frames, dropped = crate.tracked()
    assert [S.header(f)["tick"] for f in frames] == [1, 2] and dropped == 3 and all(len(f) == size for f in frames)
    for f in frames:
        assert S.header(f)["n"] == n and sorted(S.parse(f)["ids"].tolist()) == list(range(n))   # whole frames
    crate.physics_tick()
    crate.physics_tick()
    crate.physics_tick()
    assert crate.particle_count == n
    frames, dropped = crate.tracked()                                       # after the read it logs again
    assert [S.header(f)["tick"] for f in frames] == [6, 7] and dropped == 1
    assert frames[-1] != frames[0] and S.canonical(frames[1]) != S.canonical(frames[0])
    blob, count, dropped = crate.engine.track_read()
    assert (blob, count, dropped) == (b"", 0, 0)


def test_grow_keeps_the_log(sc):
    n = 50
    crate = sc.Crate(world(sc, 4 * n + 2000), noise="counter", noise_seed=1, capacity=n)
    xy, vxy = K.cloud(2, n)
    crate.particles = xy
    crate.particle_velocities = vxy
    crate.track(capacity_bytes=1 << 20)
    for _ in range(3):
        crate.physics_tick()
    old = crate.engine
    more, _ = K.cloud(3, 4 * n + 2000)
    crate.particles = more                                                  # more than the capacity: a new context
    assert crate.engine is not old
    for _ in range(2):
        crate.physics_tick()
    frames, dropped = crate.tracked()
    assert dropped == 0 and [S.header(f)["tick"] for f in frames] == [1, 2, 3, 4, 5]  # (the new context counts on)
    assert [S.header(f)["n"] for f in frames[:3]] == [n] * 3 and S.header(frames[3])["n"] == len(more)
    assert frames[-1] == crate.engine.track_capture()


# ---- loading a frame

@pytest.fixture(scope="module")
def recorded(sc):
    """One frame of a ticked scene, its parsed form, and the particle radius that goes with it."""
    from sand_crate_amd import track
    crate = sc.Crate(U.scene(sc), noise="counter", noise_seed=2)
    for _ in range(60):
        crate.physics_tick()
    frame = crate.capture_frame()
    parsed = track.parse(frame)
    assert parsed["n"] > 300 and len(set(parsed["colour"].tolist())) > 10
    return frame, parsed, crate.particle_radius


def test_load_then_download_is_parse(sc, recorded):
    frame, parsed, _ = recorded
    eng = sc.Engine(capacity=parsed["n"] + 10)
    eng.track_load(frame)
    xy, vxy, pressure, ids = eng.download()
    order = np.argsort(parsed["ids"], kind="stable")
    assert eng.count() == parsed["n"] and ids.tolist() == parsed["ids"][order].tolist()
    assert xy.tobytes() == parsed["particles"][order].tobytes()             # bit-equal: lo + q * step, not contracted
    assert not vxy.any() and vxy.shape == xy.shape
    assert pressure.tobytes() == parsed["pressure"][order].tobytes()
    assert np.array_equal(S.parse(frame)["xy"], parsed["particles"])        # (the product's parse is the spec's)
    back = eng.track_capture()                                              # and what was loaded packs to the same planes
    assert S.header(back)["n"] == parsed["n"] and S.header(back)["n_segments"] == 0   # (this engine has seen no walls)
    assert S.canonical(back)[64:] == S.canonical(frame)[64 + 32 * len(parsed["segments"]):]
    eng.track_load(frame, plain=True)
    assert (eng.download()[2] == S.pressure_of([100])[0]).all()
    eng.close()


def spec_render(parsed, radius, width, height, zoom=1.0, center=None, plain=False):
    pressure = np.full(parsed["n"], S.pressure_of([100])[0]) if plain else parsed["pressure"]
    return R.render(parsed["particles"], pressure, parsed["ids"], parsed["segments"], width, height, radius,
                    zoom=zoom, center=center)


@pytest.mark.parametrize("width,height", [(64, 48), (48, 64)])
@pytest.mark.parametrize("zoom,center", [(1.0, None), (2.5, "bulk")])
def test_player_renders_what_the_specs_say(sc, recorded, width, height, zoom, center):
    from sand_crate_amd import track
    from sand_crate_amd.hud_font import default_placement
    frame, parsed, radius = recorded
    if center == "bulk":   # a fractional centre next to the median particle's pixel: the zoomed view shows the crowd
        mx, my = np.median(parsed["particles"], axis=0)
        center = (float(np.trunc(mx * (width - 1))) + 0.25, float(np.trunc(my * (height - 1))) - 0.5)
    player = track.Player(particle_radius=radius)
    img = player.render(frame, width, height, zoom=zoom, center=center)
    want = spec_render(parsed, radius, width, height, zoom, center)
    assert img.shape == (height, width, 3) and img.tobytes() == want.tobytes()
    empty = R.render(np.zeros((0, 2)), np.zeros(0), np.zeros(0, dtype=np.int64), parsed["segments"], width, height, radius,
                     zoom=zoom, center=center)
    assert want.tobytes() != empty.tobytes()                                # (the view shows particles, not the walls alone)
    plain = player.render(frame, width, height, zoom=zoom, center=center, plain=True)
    assert plain.tobytes() == spec_render(parsed, radius, width, height, zoom, center, plain=True).tobytes()
    discs = (plain[..., 2] == 255) & (plain[..., 0] != 255) & plain.any(axis=2)
    assert discs.any() and (plain[discs] == (100, 100, 255)).all()          # every disc in the playback colour
    assert player.render_gif(frame, width, height, zoom=zoom, center=center) == G.image_data(G.indices(want))
    assert player.render_jpeg(frame, width, height, zoom=zoom, center=center) == J.encode(want, 95)
    text = f"Tick: {parsed['tick']}\nParticles: {parsed['n']}"
    with_hud = player.render(frame, width, height, zoom=zoom, center=center, hud=True)
    assert with_hud.tobytes() == T.draw(want, text.encode(), *default_placement(width)).tobytes() != want.tobytes()
    mine = player.render(frame, width, height, zoom=zoom, center=center, hud="x1")
    assert mine.tobytes() == T.draw(want, b"x1", *default_placement(width)).tobytes()
    assert player.render(frame, width, height, zoom=zoom, center=center).tobytes() == want.tobytes()   # the HUD is off again
    assert player.render(frame, width, height, zoom=zoom, center=center, particle_radius=2 * radius).tobytes() == \
        R.render(parsed["particles"], parsed["pressure"], parsed["ids"], parsed["segments"], width, height, 2 * radius,
                 zoom=zoom, center=center).tobytes()
    player.close()
    with pytest.raises(track.TrackError):
        track.Player().render(frame, width, height)                         # no radius anywhere


def test_bad_frames_are_refused_and_change_nothing(sc, recorded):
    from sand_crate_amd import _native as N
    frame, parsed, _ = recorded
    n, s = parsed["n"], len(parsed["segments"])
    eng = sc.Engine(capacity=n)
    xy, vxy = K.cloud(31, 33)
    eng.upload(xy, vxy)
    before = eng.download()

    def with_header(**kw):
        h = dict(magic=b"SCTK", version=1, tick=parsed["tick"], n=n, nseg=s, flags=1, lo=S.LO, span=S.SPAN)
        h.update(kw)
        head = struct.pack("<4sIqqiidd", h["magic"], h["version"], h["tick"], h["n"], h["nseg"], h["flags"], h["lo"], h["span"])
        return head + frame[48:]

    bigger = S.pack(1, np.zeros((n + 1, 2)), np.zeros(n + 1), np.arange(n + 1), parsed["segments"])
    bad = {"magic": (with_header(magic=b"SCTX"), N.ERR_ARG), "version 2": (with_header(version=2), N.ERR_ARG),
           "one short": (frame[:-1], N.ERR_ARG), "one long": (frame + b"\0", N.ERR_ARG), "n = -1": (with_header(n=-1), N.ERR_ARG),
           "17 segments": (with_header(nseg=17), N.ERR_ARG), "beyond the capacity": (bigger, N.ERR_CAPACITY),
           "a header alone is too short": (frame[:40], N.ERR_ARG), "empty": (b"", N.ERR_ARG)}
    for name, (data, code) in bad.items():
        with pytest.raises(N.NativeError) as err:
            eng.track_load(data)
        assert err.value.code == code, name
        assert eng.count() == 33, name
        for a, b in zip(before, eng.download()):
            assert a.tobytes() == b.tobytes(), name
    eng.track_load(frame)                                                  # the good one still loads
    assert eng.count() == n
    # the other calls' arguments and states
    for call, args in ((eng.track_enable, (0, 1024)), (eng.track_enable, (1, 0))):
        with pytest.raises(N.NativeError) as err:
            call(*args)
        assert err.value.code == N.ERR_ARG
    with pytest.raises(N.NativeError) as err:
        eng.track_read()
    assert err.value.code == N.ERR_STATE                                    # not enabled
    eng.track_disable()                                                     # (off twice is fine)
    eng.set_slab(0, 10, 3, False, False)
    for call, args in ((eng.track_capture, ()), (eng.track_enable, (1, 1024)), (eng.track_disable, ()), (eng.track_read, ()),
                       (eng.track_load, (frame,))):
        with pytest.raises(N.NativeError) as err:
            call(*args)
        assert err.value.code == N.ERR_STATE                                # slabs are not served, as by the probe
    eng.close()


# ---- the driver and the replay

def test_driver_track_then_replay_gif(sc, tmp_path):
    from sand_crate_amd import replay, track
    from sand_crate_amd.main import main
    summary = main(ROOT / "config" / "wave_machine.yaml", tmp_path, variants=1, ticks=40, track=10)
    variant = tmp_path / "variant_00"
    assert sorted(summary[0]) == ["coefficients", "particles", "seconds", "ticks", "variant"]
    assert (variant / "state.npz").exists() and (variant / "config.yaml").exists()   # every other output as it was
    with track.TrackReader(variant) as reader:
        frames = list(reader)
        assert reader.ticks() == [10, 20, 30, 40] and not reader.truncated and reader.particle_radius() == 0.005
    with np.load(variant / "state.npz") as z:                               # the recording agrees with state.npz
        for k, f in enumerate(frames):
            p = track.parse(f)
            order = np.argsort(p["ids"])
            assert int(z["ticks"][k]) == p["tick"] and np.array_equal(z[f"segments_{k}"], p["segments"])
            assert np.abs(p["particles"][order] - z[f"particles_{k}"]).max() <= S.HALF_STEP + S.ROUNDING
            assert np.array_equal(p["colour"][order], S.colour(z[f"pressure_{k}"]))
    done = replay.main([str(variant), "--gif", "--width", "96", "--height", "80", "--zoom", "1.5", "--center", "40", "44.5",
                        "--hud"])
    assert done["frames"] == 4 and done["ticks"] == [10, 20, 30, 40] and done["outputs"] == {"gif": variant / "video.gif"}
    decoded, _, delays, loop = G.decode((variant / "video.gif").read_bytes())
    player = track.Player(particle_radius=0.005)
    view = dict(zoom=1.5, center=(40.0, 44.5), hud=True)
    want = [player.render_gif(f, 96, 80, **view) for f in frames]
    assert len(decoded) == 4 and decoded[0].shape == (80, 96) and delays == [1] * 4 and loop == 0
    for k, f in enumerate(frames):
        assert np.array_equal(decoded[k], G.indices(player.render(f, 96, 80, **view)))
    assert (variant / "video.gif").read_bytes() == G.header(96, 80) + b"".join(G.frame(96, 80, d) for d in want) + b";"
    picked = replay.replay(variant / "track.sctk", frames=True, every=2, width=32, height=32, out=tmp_path / "o")
    with np.load(tmp_path / "o" / "frames.npz") as z:
        assert z["ticks"].tolist() == [10, 30] == picked["ticks"] and z["frames"].shape == (2, 32, 32, 3)
        assert z["frames"][1].tobytes() == player.render(frames[2], 32, 32).tobytes()
    player.close()
