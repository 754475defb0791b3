"""GPU tests of the GIF encoder (sc_gif_encode_device, sc_render_gif, `Crate.render_gif`, `main --gif`): the image data of
every frame equals tests/gif_spec.py byte for byte, of the palette indices of the frame tests/render_spec.py draws from
what sc_download_state returns at the same moment, and encoding changes nothing."""
import copy
import ctypes
from pathlib import Path

import numpy as np
import pytest

import gif_cases as K
import gif_spec as G
import gpu_support as U
import render_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CASES = K.cases()


@pytest.fixture(scope="module")
def engine(sc):
    eng = sc.Engine(capacity=1024)
    yield eng
    eng.close()


def spec_data(crate, width, height, **kw):
    return G.image_data(G.indices(U.spec_frame(crate, width, height, **kw)))


@pytest.fixture(scope="module")
def wave(sc):
    """The wave_machine scene after 40 ticks, and the specification's indices of its frame at three sizes."""
    crate = sc.Crate(U.scene(sc, "wave_machine"))
    for _ in range(40):
        crate.physics_tick()
    idx = {size: G.indices(U.spec_frame(crate, *size)) for size in ((200, 150), (300, 200), (1000, 1000))}
    for a in idx.values():
        a.setflags(write=False)
    return crate, idx


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(engine, name):
    import torch
    idx = CASES[name]
    want = G.image_data(idx)
    U.same_stream(engine.encode_gif(np.array(idx)), want)
    t = torch.from_numpy(np.array(idx)).cuda()
    U.same_stream(engine.encode_gif(t), want)


def test_rendered_index_images(engine, wave):
    import torch
    _, idx = wave
    for size in ((300, 200), (1000, 1000)):
        a = idx[size]
        assert a.shape == (size[1], size[0]) and len(np.unique(a)) > 2
        want = G.image_data(a)
        U.same_stream(engine.encode_gif(np.array(a)), want)
        U.same_stream(engine.encode_gif(torch.from_numpy(np.array(a)).cuda()), want)
    # back to a small frame: the workspace and the host buffer stay at the largest size asked for
    U.same_stream(engine.encode_gif(np.array(CASES["size_1x1"])), G.image_data(CASES["size_1x1"]))
    with pytest.raises(ValueError):
        engine.encode_gif(np.zeros((4, 4, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        engine.encode_gif(torch.zeros((4, 4), dtype=torch.int32, device="cuda"))


def test_wave_machine_render_gif(wave):
    crate, idx = wave
    U.same_stream(crate.render_gif(200, 150), G.image_data(idx[(200, 150)]))
    U.same_stream(crate.render_gif(1000, 1000), G.image_data(idx[(1000, 1000)]))
    # zoomed and off centre, a frame whose pixel count is not a multiple of four
    kw = dict(zoom=2.5, center=(50.0, 120.0), segment_width=3)
    U.same_stream(crate.render_gif(211, 151, **kw), spec_data(crate, 211, 151, **kw))
    # and what comes out is a GIF of that frame
    frames, pal, _, _ = G.decode(G.header(200, 150) + G.frame(200, 150, crate.render_gif(200, 150)) + b"\x3B")
    want = crate.render(200, 150)
    lossy = (want[..., 0] == 0) & (want[..., 2] == 255)
    assert np.array_equal(pal[frames[0]][~lossy], want[~lossy]) and (pal[frames[0]][lossy] == [1, 1, 255]).all()


def test_stirring_cup_render_gif(sc):
    crate = sc.Crate(U.scene(sc, "stirring_cup"))
    for _ in range(30):
        crate.physics_tick()
    U.same_stream(crate.render_gif(200, 150), spec_data(crate, 200, 150))


def test_empty_crate(sc):
    wc = copy.deepcopy(U.scene(sc, "wave_machine"))
    wc.particle_sources = []
    crate = sc.Crate(wc)
    crate.physics_tick()
    assert crate.particle_count == 0
    U.same_stream(crate.render_gif(200, 150), spec_data(crate, 200, 150))
    wc.rigid_bodies = []
    bare = sc.Crate(wc)
    data = bare.render_gif(64, 48)
    U.same_stream(data, G.image_data(np.zeros((48, 64), dtype=np.uint8)))


def test_pressures_of_one_and_above(sc):
    """A pile: pressures of 1 and above are colour byte 0, which the palette stores as index 1 -- the format's one loss.
    (The tick's pressure is max(0, .), so the device never holds a negative one; the colour rule for negative and
    non-finite pressures is the specification's, checked in tests/test_gif_cpu.py.)"""
    n = 4096
    rs = np.random.RandomState(8)
    xy = rs.rand(n, 2) * 0.96 + 0.02
    xy[: n // 2] = 0.35 + 0.3 * rs.rand(n // 2, 2)  # half of them ten times as dense
    crate = U.m2_crate(sc, n, xy)
    crate.physics_tick()
    pressure = crate.engine.download()[2]
    assert (pressure >= 1.0).any() and (pressure < 1.0 / 255).any()
    frame = U.spec_frame(crate, 200, 150)
    idx = G.indices(frame)
    assert ((frame[..., 0] == 0) & (frame[..., 2] == 255)).any() and (idx == 1).any()
    U.same_stream(crate.render_gif(200, 150), G.image_data(idx))


def test_encoding_is_read_only(sc):
    def trajectory(encode):
        crate = sc.Crate(U.scene(sc, "wave_machine"))
        for _ in range(20):
            crate.physics_tick()
            if encode:
                before = crate.engine.download(), crate.engine.rng_get_state()
                crate.render_gif(320, 240)
                crate.render_gif(100, 130, zoom=3.0, center=(20.0, 100.0))
                crate.engine.encode_gif(np.array(CASES["mixed"]))
                after = crate.engine.download(), crate.engine.rng_get_state()
                for x, y in zip(before[0], after[0]):
                    assert np.array_equal(x, y)
                assert np.array_equal(before[1][0], after[1][0]) and before[1][1] == after[1][1]
        assert crate.tick == 20
        return (*crate.engine.download(), crate.engine.rng_get_state())

    a, b = trajectory(False), trajectory(True)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    assert np.array_equal(a[4][0], b[4][0]) and a[4][1] == b[4][1]


def test_capacity_and_argument_errors(sc, engine):
    from sand_crate_amd import _native as N
    import torch
    lib, ctx = engine._lib, engine._ctx
    idx = np.array(CASES["noise_40x64"])
    h, w = idx.shape
    want = G.image_data(idx)
    dev = torch.from_numpy(idx).cuda()
    torch.cuda.synchronize()
    n = ctypes.c_int64(-1)
    buf = np.zeros(len(want) + 16, dtype=np.uint8)

    def call(cap, w=w, h=h, ptr=dev.data_ptr(), out=buf, n_out=ctypes.byref(n)):
        return lib.sc_gif_encode_device(ctx, N._P(ptr), w, h, None if out is None else N._P(out.ctypes.data), cap, n_out)

    assert call(len(want) - 1) == N.ERR_CAPACITY and n.value == len(want)
    assert not buf.any()  # nothing written
    assert call(0, out=None) == N.ERR_CAPACITY and n.value == len(want)  # a size query
    assert call(len(want)) == 0 and n.value == len(want) and buf[:len(want)].tobytes() == want
    assert not buf[len(want):].any()
    bound = ctypes.c_int64(0)
    assert lib.sc_gif_bound(w, h, ctypes.byref(bound)) == 0 and bound.value >= len(want)
    assert bound.value <= 2 * h * w  # ... and is of the order of the frame
    assert lib.sc_gif_bound(0, h, ctypes.byref(bound)) == N.ERR_ARG
    assert lib.sc_gif_bound(w, 16385, ctypes.byref(bound)) == N.ERR_ARG
    assert lib.sc_gif_bound(w, h, None) == N.ERR_ARG
    for bad in (dict(w=0), dict(h=16385), dict(h=-1), dict(ptr=0), dict(out=None), dict(cap=-1)):
        n.value = -1
        assert call(bad.pop("cap", len(buf)), **bad) == N.ERR_ARG and n.value == 0  # *n_out is always set
    assert call(len(buf), n_out=None) == N.ERR_ARG
    assert lib.sc_gif_encode_device(None, N._P(dev.data_ptr()), w, h, N._P(buf.ctypes.data), len(buf), ctypes.byref(n)) == \
        N.ERR_ARG

    crate = U.m2_crate(sc, 4096)
    crate.physics_tick()
    eng = crate.engine
    view = eng.view(64, 64, crate.particle_radius)
    out = np.zeros(1 << 16, dtype=np.uint8)
    seg = np.ascontiguousarray(crate.segments, dtype=np.float64)

    def render(cap, view=view, nseg=len(seg)):
        return eng._lib.sc_render_gif(eng._ctx, ctypes.byref(view), N.dptr(seg), nseg, N._P(out.ctypes.data), cap,
                                      ctypes.byref(n))

    assert render(10) == N.ERR_CAPACITY and n.value == len(crate.render_gif(64, 64)) and not out.any()
    assert render(len(out), view=eng.view(0, 64, crate.particle_radius)) == N.ERR_ARG
    assert render(len(out), view=eng.view(64, 64, crate.particle_radius, zoom=0.0)) == N.ERR_ARG
    assert render(len(out), nseg=N.MAX_SEGMENTS + 1) == N.ERR_ARG
    crate._send_tick_inputs()
    eng.step_begin()
    assert render(len(out)) == N.ERR_STATE
    assert eng._lib.sc_gif_encode_device(eng._ctx, N._P(dev.data_ptr()), w, h, N._P(buf.ctypes.data), len(buf),
                                         ctypes.byref(n)) == N.ERR_STATE
    eng.step_finish()
    assert render(len(out)) == 0 and out[:n.value].tobytes() == crate.render_gif(64, 64)


def check_video_gif(sc, out: Path, ticks, width=160, height=120):
    frames, pal, delays, loop = G.decode((out / "video.gif").read_bytes())
    assert len(frames) == len(ticks) and delays == [1] * len(ticks) and loop == 0
    assert np.array_equal(pal, G.palette())
    r = U.scene(sc, "wave_machine").coefficients["particle_radius"]
    want = []
    with np.load(out / "state.npz") as st:
        assert st["ticks"].tolist() == ticks
        for k in range(len(ticks)):
            xy = st[f"particles_{k}"]
            want.append(G.indices(S.render(xy, st[f"pressure_{k}"], np.arange(len(xy)), st[f"segments_{k}"], width, height, r)))
            assert np.array_equal(frames[k], want[k])
    assert (out / "video.gif").read_bytes() == G.file(want)
    return want


def test_headless_driver_streams_video_gif(sc, tmp_path):
    from sand_crate_amd.main import main
    cfg = U.small_screen_config(tmp_path)
    ticks = [10, 20, 30, 40]
    main(cfg, tmp_path / "gif", variants=1, ticks=40, record_every=10, gif=True)
    out = tmp_path / "gif" / "variant_00"
    want = check_video_gif(sc, out, ticks)
    assert any(f.any() for f in want)
    assert not (out / "frames.npz").exists() and not (out / "video.avi").exists()  # each keeps its own switch

    # with --frames as well: frames.npz as ever, and the device's video.gif is the one kept
    main(cfg, tmp_path / "both", variants=1, ticks=40, record_every=10, gif=True, frames=True, video=True)
    out = tmp_path / "both" / "variant_00"
    want = check_video_gif(sc, out, ticks)
    with np.load(out / "frames.npz") as z:
        assert z["frames"].shape == (4, 120, 160, 3) and z["ticks"].tolist() == ticks
        for k in range(4):
            assert np.array_equal(G.indices(z["frames"][k]), want[k])
    assert (out / "video.avi").stat().st_size > 0

    # --frames alone: PIL's video.gif, as before (no global palette of ours)
    main(cfg, tmp_path / "frames", variants=1, ticks=20, record_every=10, frames=True)
    out = tmp_path / "frames" / "variant_00"
    assert (out / "frames.npz").exists() and not (out / "video.avi").exists()
    try:
        import PIL  # noqa: F401
    except ImportError:
        assert not (out / "video.gif").exists()
    else:
        data = (out / "video.gif").read_bytes()
        assert data[:6] in (b"GIF89a", b"GIF87a") and data[13:13 + 768] != G.palette().tobytes()
