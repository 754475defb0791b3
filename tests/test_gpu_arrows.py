"""GPU tests of the debug arrows (sc_set_arrows, `Engine.set_arrows`, the `arrows=` argument of `Crate.render`,
`render_jpeg` and `render_gif`, `main --arrows`): a frame with a list of arrows equals tests/arrow_spec.py laid over
tests/render_spec.py's frame (and under tests/text_spec.py's text) bit for bit; the velocity mode, whose `pow` runs on the
device, agrees wherever arrow_spec's banded masks decide; the encoders see the arrows; frames without arrows are what
they were; drawing changes nothing in the simulation."""
import copy
from pathlib import Path

import numpy as np
import pytest

import arrow_cases as K
import arrow_spec as A
import gif_spec as G
import gpu_support as U
import jpeg_spec as J
import render_spec as R
import text_spec as T
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CASES = K.cases()
VELOCITY = K.velocity_cases()
WALLS = dict(segment_width=20)  # thick walls: the frame's edge is white ten pixels deep


@pytest.fixture(scope="module")
def crate(sc):
    """400 particles all over the wave_machine world after one tick (so they have pressures), discs of a few pixels at
    the frame sizes used here."""
    n = 400
    rs = np.random.RandomState(77)
    crate = sc.Crate(U.spread_world(sc, n), noise="counter", noise_seed=1, capacity=n + 1024)
    crate.particles = rs.rand(n, 2) * 0.96 + 0.02
    crate.particle_velocities = (rs.rand(n, 2) - 0.5) * 0.1
    crate.physics_tick()
    return crate


@pytest.fixture(scope="module")
def state(crate):
    xy, _, pressure, ids = crate.engine.download()
    return xy, pressure, ids, crate.segments.copy(), crate.particle_radius


_bases = {}


def base_of(state, width, height, zoom=1.0, center=None):
    """render_spec's frame of the module's crate, computed once per view."""
    key = (width, height, zoom, center)
    if key not in _bases:
        xy, pressure, ids, seg, radius = state
        frame = R.render(xy, pressure, ids, seg, width, height, radius, zoom=zoom, center=center, **WALLS)
        frame.setflags(write=False)
        _bases[key] = frame
    return _bases[key]


@pytest.fixture(scope="module")
def first_frames(crate, state):
    """Device frames taken before any arrows were set in this module's context."""
    return {name: crate.render(c.width, c.height, **c.view, **WALLS) for name, c in CASES.items() if name in ("axes", "layers")}


def green(frame):
    return (frame[..., 0] == 0) & (frame[..., 1] == 255) & (frame[..., 2] == 0)


def banded(got, base, ends, width, height, zoom, center):
    """The velocity mode's comparison: every sure_in pixel green, every sure_out pixel the frame without arrows; at
    most 1 % of the sure_in pixels undecided (a property of the spec and the state, asserted all the same)."""
    sure_in, sure_out = A.arrow_masks(ends, width, height, zoom, center)
    undecided = int((~sure_in & ~sure_out).sum())
    assert sure_in.sum() > 100 and undecided <= 0.01 * sure_in.sum(), (undecided, int(sure_in.sum()))
    assert K.trunc_room(ends, width, height) > 1e-9  # (a few ulp of an end, in cells, are 1e-13)
    miss = sure_in & ~green(got)
    assert not miss.any(), f"{miss.sum()} covered pixels are not green, the first at {np.argwhere(miss)[0].tolist()}"
    extra = sure_out & (got != base).any(axis=-1)
    assert not extra.any(), f"{extra.sum()} pixels outside every arrow changed, the first at {np.argwhere(extra)[0].tolist()}"
    rest = ~sure_in & ~sure_out
    assert (green(got[rest]) | (got[rest] == base[rest]).all(axis=-1)).all()  # undecided: one or the other, nothing else


# ---- list mode: bit for bit

def test_frames_before_any_arrows(first_frames, state):
    for name, frame in first_frames.items():
        c = CASES[name]
        U.same_frame(frame, base_of(state, c.width, c.height, c.zoom, c.center))


def test_the_layers_scene_puts_discs_and_a_wall_under_the_arrows(state):
    c = CASES["layers"]
    base = base_of(state, c.width, c.height)
    arrows = A.mask(c.ends, c.width, c.height)
    under = base[arrows]
    assert (under == 255).all(axis=-1).sum() > 20                      # the wall
    assert ((under[:, 2] == 255) & (under[:, 0] < 255)).sum() > 20     # discs under pressure
    assert (under == 0).all(axis=-1).sum() > 20                        # background
    ink = T.ink(c.hud, 6, 6, 1, c.width, c.height)
    assert (ink & arrows).any() and (base[:10, :10] == 255).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(crate, state, first_frames, name):
    c = CASES[name]
    base = base_of(state, c.width, c.height, c.zoom, c.center)
    hud = None if c.hud is None else c.hud.decode()
    got = crate.render(c.width, c.height, **c.view, **WALLS, arrows=c.pairs, hud=hud)
    want = A.draw(base, c.ends, c.zoom, c.center)
    if c.hud is not None:
        want = T.draw(want, c.hud, T.MARGIN, T.MARGIN, T.default_scale(c.width))
    U.same_frame(got, want)
    assert green(got).any()
    data = crate.render_gif(c.width, c.height, **c.view, **WALLS, arrows=c.pairs, hud=hud)
    U.same_stream(data, G.image_data(A.indices(want)))
    U.same_frame(crate.render(c.width, c.height, **c.view, **WALLS), base)  # arrows=None after an arrow frame: none


def test_engine_list_is_start_and_end(crate, state):
    """`Engine.set_arrows` takes (start, end) as they are: no compression below `Crate`."""
    from sand_crate_amd import _native as N
    c = CASES["random"]
    ends = c.ends
    crate.render(c.width, c.height, **WALLS)  # (the crate knows of no arrows)
    crate.engine.set_arrows(N.ARROWS_LIST, ends)
    try:
        got = crate.engine.render(crate.engine.view(c.width, c.height, crate.particle_radius, **WALLS), crate.segments)
    finally:
        crate.engine.set_arrows(N.ARROWS_OFF)
    U.same_frame(got, A.draw(base_of(state, c.width, c.height), ends))


def test_debug_arrows_true(sc):
    crate = sc.Crate(U.scene(sc, "wave_machine"))
    for _ in range(5):
        crate.physics_tick()
    assert crate.debug_arrows == []
    w, h = 200, 150
    base = crate.render(w, h)
    U.same_frame(crate.render(w, h, arrows=True), base)                  # an empty list
    rs = np.random.RandomState(9)
    pairs = [(rs.rand(2), (rs.rand(2) - 0.5) * 0.4) for _ in range(25)]
    pairs.append((np.array([np.nan, 0.5]), np.array([0.1, 0.1])))      # playback.py:97 skips these
    pairs.append((np.array([0.5, 0.5]), np.array([0.0, 0.0])))         # no direction: nothing
    crate.debug_arrows = list(pairs)
    got = crate.render(w, h, arrows=True)
    ends = []
    for start, direction in pairs[:25]:                                # playback.py:99-104, entry by entry
        with np.errstate(all="ignore"):
            dx, dy = direction
            d = direction / np.power(np.sqrt(dx * dx + dy * dy) + 0.001, 0.3)
        ends.append([start, start + d])
    want = A.draw(base, np.array(ends))
    U.same_frame(got, want)
    assert green(got).sum() > 200
    U.same_frame(crate.render(w, h, arrows=np.array([[s, d] for s, d in pairs])), want)  # the same list as an array
    U.same_frame(crate.render(w, h, arrows=[[list(s), list(d)] for s, d in pairs]), want)
    crate.physics_tick()                                               # crate.py:94: the tick empties the list
    assert crate.debug_arrows == []
    after = crate.render(w, h, arrows=True)
    assert not green(after).any()
    U.same_frame(after, crate.render(w, h))


# ---- velocity mode

@pytest.fixture(scope="module")
def uploaded(sc):
    """The velocity cases' state set through the `Crate` setters, no tick: ids are 0 .. n - 1."""
    v = next(iter(VELOCITY.values()))
    n = len(v.xy)
    wc = U.spread_world(sc, n)
    crate = sc.Crate(wc, noise="counter", noise_seed=1, capacity=n + 64)
    crate.particles = v.xy
    crate.particle_velocities = v.vxy
    return crate


@pytest.mark.parametrize("name", sorted(VELOCITY))
def test_velocity_of_an_uploaded_state(uploaded, name):
    v = VELOCITY[name]
    base = uploaded.render(v.width, v.height, **v.view)
    got = uploaded.render(v.width, v.height, **v.view, arrows="velocity", arrow_every=v.every, arrow_scale=v.scale)
    banded(got, base, v.ends, v.width, v.height, v.zoom, v.center)
    U.same_frame(uploaded.render(v.width, v.height, **v.view), base)


def test_velocity_after_ticks(sc):
    """512 particles at most, 20 ticks with the scene's source running: slots are cell-sorted, ids are not slot numbers."""
    wc = copy.deepcopy(U.scene(sc, "wave_machine"))
    wc.coefficients.update(max_particles=512)
    crate = sc.Crate(wc, noise="counter", noise_seed=3)
    rs = np.random.RandomState(31)
    crate.particles = rs.rand(260, 2) * 0.8 + 0.1
    crate.particle_velocities = (rs.rand(260, 2) - 0.5) * 2.0
    for _ in range(20):
        crate.physics_tick()
    xy, vxy, _, ids = crate.engine.download()
    assert 300 < len(ids) <= 512 and np.array_equal(xy, crate.particles) and np.array_equal(vxy, crate.particle_velocities)
    view = dict(zoom=1.37, center=(83.3, 57.6))
    w, h = 160, 120
    base = crate.render(w, h, **view)
    for every, scale in ((1, None), (3, 0.05), (7, 0.3)):
        got = crate.render(w, h, **view, arrows="velocity", arrow_every=every, arrow_scale=scale)
        ends = A.velocity_ends(xy, vxy, ids, crate.dt if scale is None else scale, every)
        assert len(ends) == (ids % every == 0).sum()
        banded(got, base, ends, w, h, view["zoom"], view["center"])
    U.same_frame(crate.render(w, h, **view), base)


# ---- where the frame lives, and the encoders

def test_unaligned_device_frame(crate, state):
    """61 x 37 into a tensor that starts one byte past a 4-byte boundary (sc_render_device)."""
    import torch
    c = CASES["odd_zoom_2.5"]
    w, h = c.width, c.height
    buf = torch.zeros(3 * w * h + 8, dtype=torch.uint8, device="cuda")
    out = buf[1:1 + 3 * w * h].view(h, w, 3)
    assert out.data_ptr() % 4 == 1 and out.is_contiguous()
    torch.cuda.synchronize()
    base = base_of(state, w, h, c.zoom, c.center)
    assert crate.render(w, h, out=out, arrows=c.pairs, **c.view, **WALLS) is out
    crate.synchronize()
    U.same_frame(out.cpu().numpy(), A.draw(base, c.ends, c.zoom, c.center))
    got = buf.cpu().numpy()
    assert got[0] == 0 and not got[1 + 3 * w * h:].any()  # nothing outside the frame
    assert crate.render(w, h, out=out, **c.view, **WALLS) is out  # and without: the plain frame again
    crate.synchronize()
    U.same_frame(out.cpu().numpy(), base)


def test_render_jpeg_with_arrows(crate, state):
    c = CASES["random_zoomed"]
    w, h = c.width, c.height
    frame = crate.render(w, h, **c.view, **WALLS, arrows=c.pairs)
    U.same_frame(frame, A.draw(base_of(state, w, h, c.zoom, c.center), c.ends, c.zoom, c.center))
    for q in (95, 50):
        U.same_stream(crate.render_jpeg(w, h, quality=q, **c.view, **WALLS, arrows=c.pairs), J.encode(frame, q))
    U.same_stream(crate.render_jpeg(w, h, **c.view, **WALLS), J.encode(base_of(state, w, h, c.zoom, c.center), 95))


def test_render_gif_with_arrows(crate, state, tmp_path):
    from sand_crate_amd.gif import GifWriter
    c = CASES["layers"]
    w, h = c.width, c.height
    base = base_of(state, w, h)
    frame = A.draw(base, c.ends)
    want = A.indices(frame)
    assert (want == 1).any() and (want == 255).any() and want[(want > 1) & (want < 255)].min() >= 2
    data = crate.render_gif(w, h, **WALLS, arrows=c.pairs)
    U.same_stream(data, G.image_data(want))
    frames, _, _, _ = G.decode(G.header(w, h) + G.frame(w, h, data) + b"\x3B")
    assert np.array_equal(frames[0] == 1, A.mask(c.ends, w, h) & (want == 1))
    # velocity arrows reach the encoder too: index 1 appears, and only there does the frame differ in kind
    vel = G.decode(G.header(w, h) + G.frame(w, h, crate.render_gif(w, h, **WALLS, arrows="velocity", arrow_scale=2.0)) + b"\x3B")[0][0]
    assert (vel == 1).any() and np.array_equal(vel[vel != 1], A.indices(base)[vel != 1])
    # without arrows: today's bytes, max(c, 1)
    U.same_stream(crate.render_gif(w, h, **WALLS), G.image_data(G.indices(base)))
    path = tmp_path / "arrows.gif"
    with GifWriter(path, w, h, arrows=True) as gif:
        gif.write(data)
    decoded, pal, _, _ = G.decode(path.read_bytes())
    assert np.array_equal(pal, A.palette()) and np.array_equal(decoded[0], want)
    lossy = frame.copy()
    low = (frame[..., 2] == 255) & (frame[..., 0] < 2)
    lossy[low] = (2, 2, 255)                              # the stated loss: colour bytes 0 and 1 become (2, 2, 255)
    assert np.array_equal(pal[decoded[0]], lossy)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        U.same_frame(np.array(im.convert("RGB")), lossy)


# ---- the simulation is left alone

def test_drawing_is_read_only(sc):
    def trajectory(draw):
        crate = sc.Crate(U.scene(sc, "wave_machine"))
        for k in range(10):
            crate.physics_tick()
            if draw:
                before = crate.engine.download(), crate.engine.rng_get_state()
                crate.debug_arrows = [(np.array([0.1, 0.9]), np.array([0.2, -0.1]))]
                crate.render(160, 120, arrows=True)
                crate.render_gif(100, 130, zoom=3.0, center=(20.0, 100.0), arrows=CASES["random"].pairs)
                crate.render_jpeg(96, 64, arrows="velocity", arrow_every=2)
                crate.render(160, 120, arrows="velocity", arrow_scale=0.1, hud=True)
                after = crate.engine.download(), crate.engine.rng_get_state()
                for x, y in zip(before[0], after[0]):
                    assert np.array_equal(x, y)
                assert np.array_equal(before[1][0], after[1][0]) and before[1][1] == after[1][1]
        assert crate.tick == 10
        return (*crate.engine.download(), crate.engine.rng_get_state())

    a, b = trajectory(False), trajectory(True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


# ---- errors, contexts

def test_argument_errors(crate, state):
    import ctypes as C
    from sand_crate_amd import _native as N
    eng = crate.engine
    lib, ctx = eng._lib, eng._ctx
    c = CASES["axes"]
    base = base_of(state, c.width, c.height)
    with_arrows = A.draw(base, c.ends)
    ends = np.ascontiguousarray(c.ends)
    ptr = C.cast(ends.ctypes.data, C.POINTER(N.Arrow))

    def call(mode=N.ARROWS_LIST, arrows=ptr, n=len(ends), scale=1.0, every=1, ctx=ctx):
        return lib.sc_set_arrows(ctx, mode, arrows, n, scale, every)

    def frame():
        return eng.render(eng.view(c.width, c.height, crate.particle_radius, **WALLS), crate.segments)

    crate.render(c.width, c.height, **WALLS)  # (the crate knows of no arrows)
    U.same_frame(frame(), base)
    bads = (dict(mode=3), dict(mode=-1), dict(n=-1), dict(n=N.MAX_ARROWS + 1), dict(arrows=None), dict(every=0),
            dict(every=-5), dict(scale=float("nan")), dict(scale=float("inf")), dict(mode=N.ARROWS_VELOCITY, every=0),
            dict(mode=N.ARROWS_VELOCITY, scale=float("-inf")), dict(ctx=None))
    for bad in bads:
        assert call(**bad) == N.ERR_ARG, bad
        assert lib.sc_last_error()
    U.same_frame(frame(), base)                                  # none of them set anything
    try:
        assert call() == 0
        U.same_frame(frame(), with_arrows)
        for bad in bads:
            assert call(**bad) == N.ERR_ARG, bad
        U.same_frame(frame(), with_arrows)                       # a refused call leaves the arrows that were there
        with pytest.raises(N.NativeError) as err:
            eng.set_arrows(N.ARROWS_VELOCITY, None, 1.0, 0)
        assert err.value.code == N.ERR_ARG
        U.same_frame(frame(), with_arrows)
        assert call(arrows=None, n=0) == 0                     # an empty list is no arrows; the list may then be null
        U.same_frame(frame(), base)
        assert call() == 0 and call(mode=N.ARROWS_OFF, arrows=None, n=0) == 0
        U.same_frame(frame(), base)
    finally:
        eng.set_arrows(N.ARROWS_OFF)


def test_no_arrows_inside_a_tick(sc):
    from sand_crate_amd import _native as N
    crate = sc.Crate(U.scene(sc, "wave_machine"), noise="host-sync")
    crate.physics_tick()
    eng = crate.engine
    crate._send_tick_inputs()
    eng.step_begin()
    try:
        with pytest.raises(N.NativeError) as err:
            eng.set_arrows(N.ARROWS_VELOCITY)
        assert err.value.code == N.ERR_STATE
        stats = eng.step_stats()
        eng.set_noise_host(np.random.rand(stats.neighbor_slots, 2))
    finally:
        eng.step_finish()
    assert not green(crate.render(64, 48)).any()


def test_a_new_context_has_no_arrows(sc, crate):
    from sand_crate_amd import _native as N
    crate.render(64, 48)
    crate.engine.set_arrows(N.ARROWS_LIST, CASES["axes"].ends)
    try:
        other = sc.Engine(capacity=16)
        view = other.view(64, 48, 0.01)
        assert not other.render(view, np.zeros((0, 2, 2))).any()
        other.close()
    finally:
        crate.engine.set_arrows(N.ARROWS_OFF)


def test_arrows_survive_a_grown_engine(sc):
    n = 50
    crate = sc.Crate(U.spread_world(sc, n), noise="counter", noise_seed=1, capacity=n)
    rs = np.random.RandomState(2)
    crate.particles = rs.rand(n, 2) * 0.9 + 0.05
    pairs = CASES["axes"].pairs
    before = crate.render(64, 48, arrows=pairs)
    assert green(before).sum() == 4 * 21
    old = crate.engine
    more = rs.rand(4 * n + 2000, 2) * 0.9 + 0.05
    crate.particles = more                                    # more than the capacity: `_grow` makes a new context
    assert crate.engine is not old
    after = crate.render(64, 48, arrows=pairs)
    assert np.array_equal(green(after), green(before))        # re-sent to the new context
    got = crate.render(64, 48, arrows="velocity")
    assert not green(got).any()                                # (at rest)


# ---- the driver

def test_headless_driver_with_arrows(tmp_path):
    from sand_crate_amd.main import main
    cfg = U.small_screen_config(tmp_path)
    first = {}
    for arrows in (0, 4):
        out = tmp_path / f"arrows{arrows}"
        main(cfg, out, variants=1, ticks=20, record_every=10, gif=True, arrows=arrows)
        frames, pal, _, _ = G.decode((out / "variant_00" / "video.gif").read_bytes())
        assert len(frames) == 2 and np.array_equal(pal, A.palette() if arrows else G.palette())
        first[arrows] = frames[0]
    assert (first[4] == 1).any() and (first[4] > 1).any()     # palette index 1: the arrows
    plain = first[0]
    rest = first[4] != 1
    assert np.array_equal(np.maximum(plain[rest], np.where(plain[rest] > 0, 2, 0)), first[4][rest])  # max(c, 2) elsewhere
