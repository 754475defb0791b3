"""GPU tests of the frame renderer (sc_render / sc_render_device, `Crate.render`): every frame equals tests/render_spec.py
applied to what sc_download_state returns at the same moment, bit for bit, and rendering changes nothing."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

import gpu_support as U
import render_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


def check(crate, width, height, **kw):
    img = crate.render(width, height, **kw)
    want = U.spec_frame(crate, width, height, **kw)
    assert img.shape == want.shape and img.dtype == np.uint8
    if not np.array_equal(img, want):
        bad = np.argwhere((img != want).any(axis=2))
        raise AssertionError(f"{len(bad)} pixels differ, first {bad[:5].tolist()}: {img[tuple(bad[0])]} vs "
                             f"{want[tuple(bad[0])]}")
    return img


def test_wave_machine_with_its_source_at_1000(sc):
    crate = sc.Crate(U.scene(sc, "wave_machine"))
    for _ in range(60):
        crate.physics_tick()
    assert S.disc_radius(1000, crate.particle_radius, 1.0) == 5  # the one-wave-per-disc path
    img = check(crate, 1000, 1000)
    n = crate.particle_count
    assert n > 0 and ((img[..., 2] == 255) & (img[..., 0] < 255)).any()  # particles under pressure are drawn
    assert (img == 255).all(axis=2).any()  # and the walls


def test_stirring_cup_with_moving_walls(sc):
    crate = sc.Crate(U.scene(sc, "stirring_cup"))
    for _ in range(100):
        crate.physics_tick()
    check(crate, 1000, 1000)
    check(crate, 640, 480, segment_width=5)
    check(crate, 333, 777, segment_width=0)  # a frame whose pixel count is not a multiple of four; hairline walls


def test_million_particles_at_1000_and_2048(sc):
    crate = U.m2_crate(sc, 1048576)
    crate.physics_tick()
    crate.physics_tick()
    assert S.disc_radius(1000, crate.particle_radius, 1.0) == 0
    img = check(crate, 1000, 1000)
    assert (img[..., 2] == 255).mean() > 0.5
    assert S.disc_radius(2048, crate.particle_radius, 1.0) == 1
    check(crate, 2048, 2048)


def test_zoomed_view_cut_by_the_frame_edges(sc):
    crate = sc.Crate(U.scene(sc, "wave_machine"))
    for _ in range(40):
        crate.physics_tick()
    for center in ((120.0, 880.0), (905.5, 60.25)):
        img = check(crate, 1000, 1000, zoom=4.0, center=center)
        assert img.any()
    check(crate, 700, 500, zoom=2.5, center=(50.0, 450.0), segment_width=3)


def test_pile_up_highest_id_wins(sc):
    """Thousands of particles per pixel: the frame keeps the last-drawn (highest id) one of each."""
    crate = U.m2_crate(sc, 262144)
    crate.physics_tick()
    eng = crate.engine
    xy, _, pressure, ids = eng.download()
    for side in (8, 3, 1):
        check(crate, side, side)
        img = eng.render(eng.view(side, side, crate.particle_radius), np.zeros((0, 2, 2)))  # no walls on top
        want = S.render(xy, pressure, ids, np.zeros((0, 2, 2)), side, side, crate.particle_radius)
        assert np.array_equal(img, want)
    assert img[0, 0].tolist() == [S.colour(pressure[-1:])[0]] * 2 + [255]  # one pixel: the highest id of all


def test_after_upload_every_particle_is_white(sc):
    crate = U.m2_crate(sc, 65536)
    img = check(crate, 1000, 1000)
    drawn = img.any(axis=2) & ~(img == 255).all(axis=2)
    assert not drawn.any()  # nothing but white discs (and white walls) on black
    assert (img == 255).all(axis=2).sum() > 10000


def test_rendering_is_read_only_for_physics_tick(sc):
    def trajectory(render):
        crate = sc.Crate(U.scene(sc, "wave_machine"))
        for _ in range(20):
            crate.physics_tick()
            if render:
                crate.render(500, 500)
                crate.render(300, 300, zoom=3.0, center=(40.0, 260.0))
        xy, v, pr, ids = crate.engine.download()
        return xy, v, pr, ids, crate.engine.rng_get_state()

    a, b = trajectory(False), trajectory(True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


def test_rendering_is_read_only_for_run(sc):
    def trajectory(render):
        crate = U.m2_crate(sc, 16384)
        for _ in range(4):
            crate.run(5)
            if render:
                crate.render(256, 256)
        return crate.engine.download()

    for x, y in zip(trajectory(False), trajectory(True)):
        assert np.array_equal(x, y)


def test_device_path_equals_host_path(sc):
    import torch
    crate = sc.Crate(U.scene(sc, "stirring_cup"))
    for _ in range(30):
        crate.physics_tick()
    host = crate.render(1000, 1000)
    out = torch.zeros((1000, 1000, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the library's stream does not wait for torch's)
    assert crate.render(1000, 1000, out=out) is out
    crate.synchronize()
    assert np.array_equal(out.cpu().numpy(), host)
    # a frame that starts off a 4-byte boundary, of a size that is not a multiple of four pixels
    buf = torch.zeros(333 * 777 * 3 + 1, dtype=torch.uint8, device="cuda")
    odd = buf[1:].view(777, 333, 3)
    torch.cuda.synchronize()
    crate.render(333, 777, out=odd)
    crate.synchronize()
    assert np.array_equal(odd.cpu().numpy(), crate.render(333, 777)) and int(buf[0]) == 0


def test_error_codes(sc):
    from sand_crate_amd import _native as N
    crate = U.m2_crate(sc, 4096)
    crate.physics_tick()
    eng = crate.engine
    lib, ctx = eng._lib, eng._ctx
    img = np.zeros((64, 64, 3), dtype=np.uint8)
    seg = np.zeros((17, 2, 2))

    def call(view, n_seg=0, buf=img):
        return lib.sc_render(ctx, ctypes.byref(view), N.dptr(seg), n_seg, None if buf is None else N._P(buf.ctypes.data))

    good = eng.view(64, 64, crate.particle_radius)
    assert call(good) == 0 and call(good, 16) == 0
    assert call(eng.view(0, 64, crate.particle_radius)) == N.ERR_ARG
    assert call(eng.view(64, 16385, crate.particle_radius)) == N.ERR_ARG
    assert call(eng.view(64, 64, crate.particle_radius, zoom=0.0)) == N.ERR_ARG
    assert call(eng.view(64, 64, crate.particle_radius, zoom=-1.0)) == N.ERR_ARG
    assert call(eng.view(64, 64, crate.particle_radius, zoom=float("nan"))) == N.ERR_ARG
    assert call(eng.view(64, 64, -0.1)) == N.ERR_ARG
    assert call(eng.view(64, 64, crate.particle_radius, segment_width=-1)) == N.ERR_ARG
    assert call(good, buf=None) == N.ERR_ARG
    assert lib.sc_render_device(ctx, ctypes.byref(good), None, 0, None) == N.ERR_ARG
    assert call(good, 17) == N.ERR_ARG
    assert call(good, -1) == N.ERR_ARG
    crate._send_tick_inputs()
    eng.step_begin()
    assert call(good) == N.ERR_STATE
    assert lib.sc_render_device(ctx, ctypes.byref(good), None, 0, None) == N.ERR_STATE
    eng.step_finish()
    assert call(good) == 0
    with pytest.raises(N.NativeError) as err:
        crate.render(0, 10)
    assert err.value.code == N.ERR_ARG


def test_headless_driver_writes_frames(sc, tmp_path):
    from sand_crate_amd.main import main
    main(ROOT / "config" / "wave_machine.yaml", tmp_path, variants=1, ticks=20, record_every=10, frames=True)
    out = tmp_path / "variant_00"
    r = U.scene(sc, "wave_machine").coefficients["particle_radius"]
    with np.load(out / "frames.npz") as z, np.load(out / "state.npz") as st:
        frames, ticks = z["frames"], z["ticks"]
        assert frames.shape == (2, 1000, 1000, 3) and ticks.tolist() == [10, 20] == st["ticks"].tolist()
        for k in range(2):
            xy = st[f"particles_{k}"]
            want = S.render(xy, st[f"pressure_{k}"], np.arange(len(xy)), st[f"segments_{k}"], 1000, 1000, r)
            assert np.array_equal(frames[k], want)
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert (out / "video.gif").exists()
