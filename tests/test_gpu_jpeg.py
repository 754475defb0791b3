"""GPU tests of the JPEG encoder (sc_jpeg_encode_device, sc_render_jpeg, `Crate.render_jpeg`, `main --video`): every file
equals tests/jpeg_spec.py byte for byte, of the frame tests/render_spec.py draws from what sc_download_state returns at
the same moment, and encoding changes nothing."""
import ctypes
import io
import struct
from pathlib import Path

import numpy as np
import pytest

import gpu_support as U
import jpeg_spec as J
import render_spec as S
from gpu_support import sc  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def engine(sc):
    eng = sc.Engine(capacity=1024)
    yield eng
    eng.close()


def test_random_images_at_odd_sizes(engine):
    rs = np.random.RandomState(1)
    for h, w in ((1, 1), (7, 9), (8, 8), (9, 7), (17, 1), (1, 130), (64, 64), (333, 777), (1001, 999)):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        U.same_stream(engine.encode_jpeg(img, 75), J.encode(img, 75))


def test_noise_at_quality_100(engine):
    """Long codes, many stuffed 0xFF bytes, files larger than the raw frame (the host buffer grows)."""
    rs = np.random.RandomState(2)
    for h, w in ((1000, 1000), (123, 2051)):
        img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
        data = engine.encode_jpeg(img, 100)
        assert len(data) > 3 * h * w
        U.same_stream(data, J.encode(img, 100))


def test_flat_and_extreme_images(engine):
    for value in ((0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 0, 255), (12, 200, 99)):
        img = np.empty((40, 56, 3), dtype=np.uint8)
        img[:] = value
        for q in (1, 100):
            U.same_stream(engine.encode_jpeg(img, q), J.encode(img, q))
    # the largest DC steps: black and white blocks in turn, at quality 100
    img = np.zeros((16, 64, 3), dtype=np.uint8)
    img[:, 8::16] = 255
    img[:, 9:16] = 255
    U.same_stream(engine.encode_jpeg(img, 100), J.encode(img, 100))


def test_quality_sweep(engine):
    rs = np.random.RandomState(3)
    y, x = np.mgrid[0:200, 0:300]
    smooth = np.stack([x * 255 // 299, y * 255 // 199, (x * y) % 256], axis=2).astype(np.uint8)
    noisy = np.clip(smooth + rs.randint(-20, 21, smooth.shape), 0, 255).astype(np.uint8)
    for q in (1, 2, 10, 25, 49, 50, 51, 75, 90, 95, 99, 100):
        for img in (smooth, noisy):
            U.same_stream(engine.encode_jpeg(img, q), J.encode(img, q))


def test_cuda_tensor_input(engine):
    import torch
    img = np.random.RandomState(4).randint(0, 256, (300, 200, 3)).astype(np.uint8)
    t = torch.from_numpy(img).cuda()
    U.same_stream(engine.encode_jpeg(t, 90), J.encode(img, 90))
    with pytest.raises(ValueError):
        engine.encode_jpeg(t[:, :, :2].contiguous(), 90)


def test_wave_machine_render_jpeg(sc):
    crate = sc.Crate(U.scene(sc, "wave_machine"))
    for _ in range(60):
        crate.physics_tick()
    for q in (95, 50):
        U.same_stream(crate.render_jpeg(1000, 1000, quality=q), J.encode(U.spec_frame(crate, 1000, 1000), q))
    U.same_stream(crate.render_jpeg(640, 481, zoom=2.0, center=(100.0, 300.0)),
                  J.encode(U.spec_frame(crate, 640, 481, zoom=2.0, center=(100.0, 300.0)), 95))


def test_million_particles_at_1000_and_4096(sc):
    crate = U.m2_crate(sc, 1048576)
    crate.physics_tick()
    crate.physics_tick()
    for side in (1000, 4096):
        U.same_stream(crate.render_jpeg(side, side), J.encode(U.spec_frame(crate, side, side), 95))


def test_device_frame_from_render(sc):
    """sc_jpeg_encode_device on a frame sc_render_device wrote: what Crate.render_jpeg gives."""
    import torch
    crate = sc.Crate(U.scene(sc, "stirring_cup"))
    for _ in range(30):
        crate.physics_tick()
    out = torch.zeros((480, 640, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    crate.render(640, 480, out=out)
    crate.synchronize()
    U.same_stream(crate.engine.encode_jpeg(out, 95), crate.render_jpeg(640, 480))


def test_encoding_is_read_only(sc):
    def trajectory(encode):
        crate = sc.Crate(U.scene(sc, "wave_machine"), noise="counter", noise_seed=5)
        for _ in range(20):
            crate.physics_tick()
            if encode:
                before = crate.engine.download()
                crate.render_jpeg(500, 500)
                crate.render_jpeg(300, 200, quality=10, zoom=3.0)
                for x, y in zip(before, crate.engine.download()):
                    assert np.array_equal(x, y)
        assert crate.tick == 20
        return crate.engine.download()

    for x, y in zip(trajectory(False), trajectory(True)):
        assert np.array_equal(x, y)


def test_capacity_and_argument_errors(sc, engine):
    from sand_crate_amd import _native as N
    import torch
    lib, ctx = engine._lib, engine._ctx
    img = np.random.RandomState(6).randint(0, 256, (50, 70, 3)).astype(np.uint8)
    want = J.encode(img, 80)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    n = ctypes.c_int64(-1)
    buf = np.zeros(len(want) + 16, dtype=np.uint8)

    def call(cap, q=80, w=70, h=50, ptr=dev.data_ptr(), out=buf):
        return lib.sc_jpeg_encode_device(ctx, N._P(ptr), w, h, q, None if out is None else N._P(out.ctypes.data), cap,
                                         ctypes.byref(n))

    assert call(len(want) - 1) == N.ERR_CAPACITY and n.value == len(want)
    assert not buf.any()  # nothing written
    assert call(0, out=None) == N.ERR_CAPACITY and n.value == len(want)  # a size query
    assert call(len(want)) == 0 and n.value == len(want) and buf[:len(want)].tobytes() == want
    bound = ctypes.c_int64(0)
    assert lib.sc_jpeg_bound(70, 50, ctypes.byref(bound)) == 0 and bound.value >= len(want)
    assert lib.sc_jpeg_bound(0, 50, ctypes.byref(bound)) == N.ERR_ARG
    for q in (0, 101):
        assert call(len(buf), q=q) == N.ERR_ARG
    assert call(len(buf), w=0) == N.ERR_ARG
    assert call(len(buf), h=16385) == N.ERR_ARG
    assert call(len(buf), ptr=0) == N.ERR_ARG
    assert call(len(buf), out=None) == N.ERR_ARG
    assert lib.sc_jpeg_encode_device(ctx, N._P(dev.data_ptr()), 70, 50, 80, N._P(buf.ctypes.data), len(buf), None) == \
        N.ERR_ARG

    crate = U.m2_crate(sc, 4096)
    crate.physics_tick()
    eng = crate.engine
    view = eng.view(64, 64, crate.particle_radius)
    out = np.zeros(1 << 16, dtype=np.uint8)
    seg = np.ascontiguousarray(crate.segments, dtype=np.float64)
    rc = eng._lib.sc_render_jpeg(eng._ctx, ctypes.byref(view), N.dptr(seg), len(seg), 95, N._P(out.ctypes.data), 10,
                                 ctypes.byref(n))
    assert rc == N.ERR_CAPACITY and n.value == len(crate.render_jpeg(64, 64))
    crate._send_tick_inputs()
    eng.step_begin()
    assert eng._lib.sc_render_jpeg(eng._ctx, ctypes.byref(view), N.dptr(seg), 0, 95, N._P(out.ctypes.data), len(out),
                                   ctypes.byref(n)) == N.ERR_STATE
    eng.step_finish()
    with pytest.raises(N.NativeError) as err:
        crate.render_jpeg(64, 64, quality=0)
    assert err.value.code == N.ERR_ARG


def avi_frames(path: Path):
    """The 00dc chunks of an AVI file, in index order."""
    data = path.read_bytes()
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI "
    movi = data.index(b"movi") - 8
    idx = data.rindex(b"idx1")
    n = struct.unpack("<I", data[idx + 4:idx + 8])[0] // 16
    out = []
    for k in range(n):
        ckid, _, off, size = struct.unpack("<4sIII", data[idx + 8 + 16 * k:idx + 24 + 16 * k])
        at = movi + 8 + off
        assert ckid == b"00dc" == data[at:at + 4]
        out.append(data[at + 8:at + 8 + size])
    return out


def test_headless_driver_writes_video(sc, tmp_path):
    from sand_crate_amd.main import main
    main(ROOT / "config" / "wave_machine.yaml", tmp_path, variants=1, ticks=200, record_every=10, video=True)
    out = tmp_path / "variant_00"
    frames = avi_frames(out / "video.avi")
    assert len(frames) == 20
    r = U.scene(sc, "wave_machine").coefficients["particle_radius"]
    with np.load(out / "state.npz") as st:
        assert st["ticks"].tolist() == list(range(10, 201, 10))
        for k, f in enumerate(frames):
            xy = st[f"particles_{k}"]
            img = S.render(xy, st[f"pressure_{k}"], np.arange(len(xy)), st[f"segments_{k}"], 1000, 1000, r)
            U.same_stream(f, J.encode(img, 95))
    try:
        from PIL import Image
    except ImportError:
        return
    assert np.asarray(Image.open(io.BytesIO(frames[-1])).convert("RGB")).shape == (1000, 1000, 3)
    assert not (out / "frames.npz").exists()  # --frames keeps its own switch
