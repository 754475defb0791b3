"""The frame renderer at the edges of its raster rule (tests/render_cases.py), against tests/render_spec.py.

Every case is rendered three ways -- the host frame of sc_render, the device frame of sc_render_device written one byte
off a 4-byte boundary, and the palette-index image of sc_render_gif, decoded -- and each must equal the specification
applied to what sc_download_state returns at that moment, bit for bit (the index image: tests/gif_spec.py's indices of
that frame).  What a case claims about its frame is proven on the specification in tests/test_render_cases_cpu.py; the
frames of the uploaded cases are also held to the specification of the case as it was built.  `pressures` and
`appended` are ticked on the device, whose tick differs from the oracle's in the ninth digit, so they assert their
premises again on the downloaded state.  No HUD and no arrows are set."""
import numpy as np
import pytest

import gif_spec as G
import render_cases as K
import render_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

COEF = ("dt", "particle_radius", "wall_collision_decay", "pressure_amplifier", "ignored_pressure",
        "collider_noise_level", "viscosity", "surface_smoothing", "target_pressure")


@pytest.fixture(scope="module")
def engine(sc):
    eng = sc.Engine(capacity=8192)
    yield eng
    eng.close()


def same(img, want, what):
    assert img.shape == want.shape and img.dtype == np.uint8, what
    if not np.array_equal(img, want):
        bad = np.argwhere((img != want).any(axis=2) if img.ndim == 3 else img != want)
        raise AssertionError(f"{what}: {len(bad)} pixels differ, first {bad[:5].tolist()}: {img[tuple(bad[0])]} vs "
                             f"{want[tuple(bad[0])]}")


def check(eng, c):
    """The three outputs of case `c`'s frame against the specification of the device's state; -> that frame."""
    import torch
    xy, _, pressure, ids = eng.download()
    with np.errstate(over="ignore"):  # (a wall's len2 may overflow: wall_shapes_1e300)
        want = S.render(xy, pressure, ids, c.segments, c.width, c.height, c.particle_radius, **c.view)
    view = eng.view(c.width, c.height, c.particle_radius, **c.view)
    same(eng.render(view, c.segments), want, f"{c.name}, sc_render")
    buf = torch.zeros(3 * c.width * c.height + 1, dtype=torch.uint8, device="cuda")
    out = buf[1:].view(c.height, c.width, 3)
    torch.cuda.synchronize()  # (the library's stream does not wait for torch's)
    assert eng.render(view, c.segments, out=out) is out
    eng.synchronize()
    same(out.cpu().numpy(), want, f"{c.name}, sc_render_device")
    assert int(buf[0]) == 0
    data = eng.render_gif(view, c.segments)
    frames, _, _, _ = G.decode(G.header(c.width, c.height) + G.frame(c.width, c.height, data) + b"\x3B")
    same(frames[0], G.indices(want), f"{c.name}, the index image of sc_render_gif")
    return want


@pytest.mark.parametrize("name", K.UPLOADED)
def test_uploaded(engine, name):
    for c in K.group(name):
        engine.upload(c.xy, np.zeros_like(c.xy))
        assert np.array_equal(check(engine, c), c.spec()), c.name


@pytest.mark.parametrize("backwards", (False, True), ids=("in_order", "backwards"))
def test_frame_sizes_on_one_context(sc, backwards):
    cases = K.group("frame_sizes")
    eng = sc.Engine(capacity=1024)
    eng.upload(cases[0].xy, np.zeros_like(cases[0].xy))
    for c in (cases[::-1] if backwards else cases):
        want = check(eng, c)
        assert np.array_equal(want, c.spec()) and bool(c.claims.get("black")) == (not want.any()), c.name
    eng.close()


def ticked_engine(sc):
    """A context that holds the blob of `pressures` after one tick of the device.  Before that the context ticks a
    larger world twice -- the blob and 300 crowded particles that sort behind it -- so that the pressure buffers hold
    something other than zero behind the blob's slots: a renderer that colours every stored slot shows it."""
    from oracle.scene import OracleCrate
    from oracle.world import World
    from sand_crate_amd import _native as N
    coef = dict(K.PRESSURE_COEF)
    orc = OracleCrate(World(K.PRESSURE_BODIES, [], coef))
    seg = orc.segments
    bodies = [(b.position, b.center_velocity, b.omega, b.n_segments) for b in orc.body_states()]
    eng = sc.Engine(capacity=8192)
    eng.set_noise_mode(N.NOISE_NONE, 0)

    def tick():
        eng.set_params(gravity=coef["gravity"], **{k: coef[k] for k in COEF})
        eng.set_segments(seg, sc.pad_segments(seg, coef["particle_radius"]), bodies)
        eng.step_begin()
        eng.step_finish()

    p, v = K.pressure_blob()
    rs = np.random.RandomState(5)
    crowd = np.column_stack((0.3 + rs.rand(300) * 0.3, 0.93 + rs.rand(300) * 0.04))
    eng.upload(np.vstack((p, crowd)), np.vstack((v, np.zeros((300, 2)))))
    tick()
    tick()
    eng.upload(p, v)
    tick()
    return eng


def test_pressures(sc):
    c, = K.group("pressures")
    eng = ticked_engine(sc)
    xy, _, pressure, ids = eng.download()
    assert K.pressure_premises(xy, pressure, ids, c) >= 50
    np.testing.assert_allclose(pressure, c.pressure, rtol=1e-9, atol=1e-12)  # (the oracle's tick, to the parity bar)
    check(eng, c)
    eng.close()


def test_appended(sc):
    c, = K.group("appended")
    eng = ticked_engine(sc)
    before = eng.download()
    eng.append(*K.appended_particles())
    xy, _, pressure, ids = eng.download()
    assert np.array_equal(xy[:K.PRESSURE_N], before[0]) and np.array_equal(pressure[:K.PRESSURE_N], before[2])
    old, new = K.appended_premises(xy, pressure, ids, c)
    want = check(eng, c)
    assert (want[new] == 255).all() and (want[old][:, 0] < 255).sum() >= 50
    eng.close()
