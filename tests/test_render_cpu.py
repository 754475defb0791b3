"""Frames without a GPU: the raster rule of tests/render_spec.py checked against hand-counted cases, the two render entry
points in the header, the export table and the ctypes layout, and the driver's frame writer."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import render_spec as S

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "sandcrate_hip.h"
NO_WALLS = np.zeros((0, 2, 2))


def one(x, y, W=100, H=100, radius=0.05, p=0.0, **kw):
    return S.render(np.array([[x, y]]), np.array([p]), np.array([0]), NO_WALLS, W, H, radius, **kw)


def covered(img):
    return int(img.any(axis=2).sum())


def test_disc_pixel_counts():
    # trunc(100 * 0.05) = 5: Gauss's circle count N(5) = 81; trunc(100 * 0.009) = 0: the centre pixel only
    assert S.disc_radius(100, 0.05, 1.0) == 5
    assert covered(one(0.5, 0.5)) == 81
    assert S.disc_radius(100, 0.009, 1.0) == 0
    assert covered(one(0.5, 0.5, radius=0.009)) == 1
    # zoom scales the truncated radius, then floors: trunc(5) * 1.5 = 7.5 -> 7, N(7) = 149
    assert covered(one(0.5, 0.5, zoom=1.5)) == 149


def test_view_at_zoom_one_is_the_truncated_world_coordinate():
    W, H = 640, 480
    rs = np.random.RandomState(3)
    xy = rs.rand(500, 2)
    keys = S.particle_keys(xy, np.zeros(500), np.arange(500), W, H, 0.0)
    want = np.zeros((H, W), dtype=np.uint64)
    for k, (x, y) in enumerate(xy):
        want[int(y * (H - 1)), int(x * (W - 1))] = max(want[int(y * (H - 1)), int(x * (W - 1))], ((k + 1) << 8) | 255)
    assert np.array_equal(keys, want)
    assert np.array_equal(S.screen([0.25, 0.75], W, W / 2, 1.0), [int(0.25 * (W - 1)), int(0.75 * (W - 1))])


def test_highest_id_wins_on_the_overlap():
    xy = np.array([[0.45, 0.5], [0.55, 0.5]])
    img = S.render(xy, np.array([0.0, 1.0]), np.array([7, 3]), NO_WALLS, 100, 100, 0.08)
    a, b = one(0.45, 0.5, radius=0.08).any(axis=2), one(0.55, 0.5, radius=0.08).any(axis=2)
    both = a & b
    assert both.sum() > 0
    assert (img[both] == [255, 255, 255]).all()  # id 7 (pressure 0, white) over id 3 (pressure 1, blue)
    assert (img[b & ~a] == [0, 0, 255]).all()
    # swap the ids: now the blue one is drawn last
    img = S.render(xy, np.array([0.0, 1.0]), np.array([3, 7]), NO_WALLS, 100, 100, 0.08)
    assert (img[both] == [0, 0, 255]).all()


def test_colours():
    c = S.colour(np.array([0.0, 0.5, 1.0, 3.0, np.nan, -0.5, np.inf, -np.inf]))
    assert c.tolist() == [255, 128, 0, 0, 0, 255, 0, 255]
    img = one(0.5, 0.5, p=0.5, radius=0.009)
    assert img[49, 49].tolist() == [128, 128, 255]


def test_horizontal_wall_of_width_two_covers_three_rows():
    W = H = 101
    seg = np.array([[[0.2, 0.5], [0.8, 0.5]]])
    img = S.render(np.zeros((0, 2)), np.zeros(0), np.zeros(0, dtype=np.int64), seg, W, H, 0.0, segment_width=2)
    rows = np.nonzero(img.any(axis=(1, 2)))[0]
    assert rows.tolist() == [49, 50, 51]
    assert (img[img.any(axis=2)] == 255).all()
    # a wall overrides the particles under it
    img = S.render(np.array([[0.5, 0.5]]), np.array([1.0]), np.array([0]), seg, W, H, 0.05)
    assert img[50, 50].tolist() == [255, 255, 255] and img[47, 50].tolist() == [0, 0, 255]


def test_clipping_at_the_four_edges():
    full = covered(one(0.5, 0.5))
    for x, y in ((0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0)):
        n = covered(one(x, y))
        assert 0 < n < full  # part of the disc is outside the frame: those pixels are dropped, the rest drawn
    # a disc centred on column 0 keeps its columns 0..5, of 11, 9, 9, 9, 7 and 1 pixels
    assert covered(one(0.0, 0.5)) == 46
    assert covered(one(1.0, 1.0)) == 26  # at the corner (99, 99) a quarter with its two radii: 6 + 5 + 5 + 5 + 4 + 1
    # discs that miss the frame entirely, and positions that are not finite, draw nothing
    for x, y in ((-0.2, 0.5), (1.2, 0.5), (0.5, -0.2), (0.5, 1.2), (np.nan, 0.5), (0.5, np.inf)):
        assert covered(one(x, y)) == 0


def test_header_declares_and_library_exports_the_render_path():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for name in ("sc_render", "sc_render_device"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
    from sand_crate_amd import build
    lib = ctypes.CDLL(str(build.build()))
    assert hasattr(lib, "sc_render") and hasattr(lib, "sc_render_device")


def test_view_struct_layout():
    from sand_crate_amd import _native as N
    text = HEADER.read_text()
    body = re.search(r"typedef struct sc_view \{(.*?)\} sc_view;", text, re.S).group(1)
    assert re.findall(r"\b(int32_t|double)\b", body) == ["int32_t", "double", "double", "double", "int32_t", "int32_t"]
    assert ctypes.sizeof(N.View) == 2 * 4 + 4 * 8 + 2 * 4
    assert N.View.zoom.offset == 8 and N.View.particle_radius.offset == 32 and N.View.segment_width.offset == 40
    assert "sc_render" in N.SIGNATURES and "sc_render_device" in N.SIGNATURES


def test_frame_writer_round_trips(tmp_path):
    from sand_crate_amd.main import write_frames
    rs = np.random.RandomState(5)
    frames = [np.zeros((24, 32, 3), dtype=np.uint8) for _ in range(3)]
    for k, f in enumerate(frames):
        f[rs.rand(24, 32) < 0.3] = [(255, 255, 255), (0, 0, 255), (128, 128, 255)][k]
    write_frames(tmp_path, frames, [10, 20, 30])
    with np.load(tmp_path / "frames.npz") as z:
        assert z["frames"].shape == (3, 24, 32, 3) and z["frames"].dtype == np.uint8
        assert np.array_equal(z["frames"], np.stack(frames))
        assert z["ticks"].tolist() == [10, 20, 30]
    try:
        from PIL import Image
    except ImportError:
        assert not (tmp_path / "video.gif").exists()
        return
    with Image.open(tmp_path / "video.gif") as gif:
        assert gif.size == (32, 24) and gif.n_frames == 3
        for k in range(3):
            gif.seek(k)
            assert np.array_equal(np.asarray(gif.convert("RGB")), frames[k])  # three colours: no palette loss


def test_no_frames_without_the_flag(tmp_path):
    """HeadlessPlayback.save_recording without --frames writes what it wrote before."""
    from sand_crate_amd.load_config import load_config
    from sand_crate_amd.main import HeadlessPlayback
    pb = HeadlessPlayback.__new__(HeadlessPlayback)
    pb.config = load_config(ROOT / "config" / "wave_machine.yaml")
    pb.frames = [{"tick": 10, "particles": np.zeros((2, 2)), "pressure": np.zeros(2), "segments": np.zeros((1, 2, 2))}]
    pb.render_frames = False
    pb.images = []
    pb.save_recording(tmp_path)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["config.yaml", "state.npz"]
