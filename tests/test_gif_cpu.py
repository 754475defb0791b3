"""CPU checks of the GIF bitstream's specification (tests/gif_spec.py), of the inputs built to exercise it
(tests/gif_cases.py: each has the property it is named for) and of the file writer (sand_crate_amd/gif.py).
No GPU: the device encoder is held to gif_spec byte for byte by tests/test_gpu_gif.py."""
import io

import numpy as np
import pytest

import gif_cases as K
import gif_spec as G
import render_spec as S

CASES = K.cases()


def data_codes_per_chunk(idx):
    """The number of data codes between each clear code and the next (or the end code), and the clears' widths."""
    counts, widths = [], []
    for code, width in G.lzw_codes(idx):
        if code == G.CLEAR:
            counts.append(0)
            widths.append(width)
        elif code != G.END:
            counts[-1] += 1
    return counts, widths


def test_palette():
    pal = G.palette()
    assert pal.shape == (256, 3) and pal.dtype == np.uint8
    assert pal[0].tolist() == [0, 0, 0] and pal[1].tolist() == [1, 1, 255] and pal[255].tolist() == [255, 255, 255]
    assert all(pal[k].tolist() == [k, k, 255] for k in range(1, 256))
    from sand_crate_amd import gif
    assert gif.palette() == pal.tobytes()


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_round_trips(name):
    idx = CASES[name]
    data = G.file([idx, idx[::-1, ::-1]])
    frames, pal, delays, loop = G.decode(data)
    assert len(frames) == 2 and np.array_equal(frames[0], idx) and np.array_equal(frames[1], idx[::-1, ::-1])
    assert np.array_equal(pal, G.palette()) and delays == [1, 1] and loop == 0
    try:
        from PIL import Image
    except ImportError:
        return
    im = Image.open(io.BytesIO(data))
    assert im.n_frames == 2 and im.info["duration"] == 10 and im.info["loop"] == 0
    for k, want in enumerate((idx, idx[::-1, ::-1])):
        im.seek(k)
        assert np.array_equal(np.asarray(im.convert("RGB")), G.palette()[want])


def test_sizes_in_pixels():
    assert sorted(CASES[f"size_{h}x{w}"].size for h, w in K.SIZES) == [1, 1023, 1023, 1024, 1025, 2049]
    for (h, w), chunks in zip(K.SIZES, (1, 1, 1, 2, 3, 1)):
        assert len(data_codes_per_chunk(CASES[f"size_{h}x{w}"])[0]) == chunks
    # one pixel: clear, the pixel, end, 9 bits each
    assert G.lzw_codes(CASES["size_1x1"]) == [(256, 9), (int(CASES["size_1x1"][0, 0]), 9), (257, 9)]
    assert len(G.image_data(CASES["size_1x1"])) == 1 + 1 + 4 + 1


def test_flat_chunks_have_the_longest_matches():
    # a run of n equal pixels goes out as strings of 1, 2, 3, .. pixels: 1024 = 1 + .. + 44 + 34
    assert data_codes_per_chunk(CASES["flat_zero_1x1024"])[0] == [45]
    counts, widths = data_codes_per_chunk(CASES["flat_3x683"])
    assert counts == [45, 45, 1] and widths == [9, 9, 9]  # 2049 pixels: two full chunks and one pixel


def test_noise_reaches_eleven_bits_and_no_more():
    for name in ("noise_40x64", "size_1x1024", "mixed"):
        widths = {w for _, w in G.lzw_codes(CASES[name])}
        assert widths == {9, 10, 11}
    assert max(code for code, _ in G.lzw_codes(CASES["noise_40x64"])) <= 1281


def test_mixed_chunks_emit_clear_codes_at_every_width():
    counts, widths = data_codes_per_chunk(CASES["mixed"])
    assert len(counts) == 7 and set(widths) == {9, 10, 11}
    assert widths[:4] == [9, 9, 10, 11]  # the first; after flat; after the ramp; after noise
    assert counts[0] < 255 <= counts[1] < 767 <= counts[2]


@pytest.mark.parametrize("count", K.BUMP_COUNTS)
def test_exact_code_counts(count):
    after = 9 if count < 255 else (10 if count < 767 else 11)
    codes = G.lzw_codes(CASES[f"last_{count}"])
    assert data_codes_per_chunk(CASES[f"last_{count}"])[0] == [count]
    assert codes[-1] == (G.END, after) and codes[-2][1] == (9 if count <= 255 else (10 if count <= 767 else 11))
    idx = CASES[f"full_{count}"]
    assert idx.size == K.CHUNK + 7
    counts, widths = data_codes_per_chunk(idx)
    assert counts[0] == count and widths == [9, after]


def test_packed_lengths_at_the_sub_block_edges():
    for size in K.PACKED_LENGTHS:
        idx = CASES[f"packed_{size}"]
        assert K.packed_length(idx) == size
        data = G.image_data(idx)
        assert data[0] == 8 and data[-1] == 0 and len(data) == 2 + size + -(-size // 255)
        lengths, at = [], 1
        while data[at]:
            lengths.append(data[at])
            at += 1 + data[at]
        assert at == len(data) - 1  # the terminator; no empty block before it
        assert lengths == [255] * (size // 255) + ([size % 255] if size % 255 else [])


def test_indices_of_rendered_frames():
    """Background, discs of c = 0, 1, 255 and others, walls."""
    xy = np.array([[0.2, 0.2], [0.5, 0.2], [0.8, 0.2], [0.2, 0.7], [0.5, 0.7], [0.8, 0.7]])
    pressure = np.array([1.5, 254.5 / 255, 0.0, 0.5, -3.0, np.nan])
    assert S.colour(pressure).tolist() == [0, 1, 255, 128, 255, 0]
    seg = np.array([[[0.05, 0.95], [0.95, 0.95]], [[0.05, 0.05], [0.05, 0.95]]])
    img = S.render(xy, pressure, np.arange(6), seg, 120, 90, 0.04)
    idx = G.indices(img)
    assert idx.shape == (90, 120) and idx.dtype == np.uint8
    keys = S.particle_keys(xy, pressure, np.arange(6), 120, 90, 0.04)
    wall = S.wall_mask(seg, 120, 90)
    c = (keys & np.uint64(0xFF)).astype(np.uint8)
    want = np.where(wall, 255, np.where(keys == 0, 0, np.maximum(c, 1))).astype(np.uint8)
    assert np.array_equal(idx, want)
    assert {0, 1, 128, 255} <= set(np.unique(idx).tolist())
    assert (idx[(keys != 0) & ~wall & (c == 0)] == 1).all() and ((keys != 0) & ~wall & (c == 0)).any()
    # the palette gives the frame back, but for (0, 0, 255) -> (1, 1, 255)
    back = G.palette()[idx]
    lossy = (img[..., 0] == 0) & (img[..., 2] == 255)
    assert lossy.any() and np.array_equal(back[~lossy], img[~lossy]) and (back[lossy] == [1, 1, 255]).all()
    frames, _, _, _ = G.decode(G.file([idx]))
    assert np.array_equal(frames[0], idx)


@pytest.mark.parametrize("count", (0, 1, 3))
def test_gif_writer_equals_the_spec(tmp_path, count):
    from sand_crate_amd.gif import GifWriter
    frames = [CASES["size_31x33"], CASES["size_31x33"].T.copy().reshape(31, 33), CASES["size_31x33"][::-1]][:count]
    for kw in ({}, {"delay_cs": 7, "loop": 3}):
        with GifWriter(tmp_path / "a.gif", 33, 31, **kw) as w:
            for f in frames:
                w.write(G.image_data(f))
            assert w.frames == count
        assert (tmp_path / "a.gif").read_bytes() == G.file(frames, size=(33, 31), **kw)
    got, _, delays, loop = G.decode((tmp_path / "a.gif").read_bytes())
    assert len(got) == count and delays == [7] * count and loop == 3
    with pytest.raises(ValueError):
        w.write(G.image_data(frames[0]) if frames else b"\x08\x00")  # closed
    with pytest.raises(ValueError):
        GifWriter(tmp_path / "b.gif", 0, 5)
    with GifWriter(tmp_path / "c.gif", 2, 2) as w, pytest.raises(ValueError):
        w.write(b"\xff\xd8 not image data")


def test_write_frames_can_skip_its_gif(tmp_path):
    from sand_crate_amd.main import write_frames
    frames = [np.zeros((4, 5, 3), dtype=np.uint8)] * 2
    write_frames(tmp_path, frames, [10, 20], gif=False)
    assert (tmp_path / "frames.npz").exists() and not (tmp_path / "video.gif").exists()
    write_frames(tmp_path, frames, [10, 20])
    try:
        import PIL  # noqa: F401
    except ImportError:
        return
    assert (tmp_path / "video.gif").exists()
