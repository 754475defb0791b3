"""CPU tests of the JPEG bitstream rule (tests/jpeg_spec.py) and of the Motion-JPEG AVI writer (sand_crate_amd/avi.py).
No GPU: the device encoder is held to jpeg_spec byte for byte by tests/test_gpu_jpeg.py."""
import io
import struct

import numpy as np
import pytest

import jpeg_spec as J
import render_spec as S

PIL = pytest.importorskip("PIL")
from PIL import Image  # noqa: E402

BOX = np.array([[[0.02, 0.02], [0.98, 0.02]], [[0.98, 0.02], [0.98, 0.98]], [[0.98, 0.98], [0.02, 0.98]],
                [[0.02, 0.98], [0.02, 0.02]]])


def decode(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def psnr(a, b) -> float:
    err = ((np.asarray(a, dtype=np.float64) - b) ** 2).mean()
    return float("inf") if err == 0 else 10 * np.log10(255.0 ** 2 / err)


def particle_frame(n: int, radius: float) -> np.ndarray:
    """render_spec's frame of n particles spread over the crate, pressures 0..1.2, inside four walls."""
    rs = np.random.RandomState(7)
    xy = rs.rand(n, 2) * 0.96 + 0.02
    return S.render(xy, rs.rand(n) * 1.2, np.arange(n), BOX, 1000, 1000, radius)


def segments(data: bytes):
    """(marker, body) of every segment up to SOS, then the entropy-coded data up to EOI."""
    assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    out, i = [], 2
    while True:
        marker, length = struct.unpack(">HH", data[i:i + 4])
        out.append((marker, data[i + 4:i + 2 + length]))
        i += 2 + length
        if marker == 0xFFDA:
            return out, data[i:-2]


@pytest.mark.parametrize("h,w", [(1, 1), (7, 9), (8, 8), (1000, 1000), (1001, 999)])
def test_the_spec_decodes(h, w):
    rs = np.random.RandomState(h * 7 + w)
    img = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    for q in (1, 50, 95, 100):
        out = decode(J.encode(img, q))
        assert out.shape == (h, w, 3)
        if q == 100:
            assert psnr(out, img) > 45


def test_smooth_image_decodes_close():
    y, x = np.mgrid[0:77, 0:131]
    img = np.stack([x * 255 // 130, y * 255 // 76, (x + y) * 255 // 206], axis=2).astype(np.uint8)
    assert psnr(decode(J.encode(img, 95)), img) > 40


def test_quality_floor_on_rendered_frames():
    """Quality 95 (the driver's default) on render_spec frames; the floors sit just below the spec's own numbers
    (40.12 dB at 4,000 particles of radius 5 px, 37.55 dB at 1,048,576 of radius 0)."""
    small = particle_frame(4000, 0.005)
    assert psnr(decode(J.encode(small, 95)), small) >= 40.0
    big = particle_frame(1048576, float(np.sqrt(12 / (np.pi * 1048576))) / 2)
    assert psnr(decode(J.encode(big, 95)), big) >= 37.4


def test_tables_are_the_standard_ones():
    """PIL (libjpeg) at the same quality, unoptimised: the same quantisation and Huffman tables."""
    img = np.random.RandomState(3).randint(0, 256, (16, 16, 3)).astype(np.uint8)
    for q in (1, 10, 50, 75, 95, 100):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=0)
        theirs, _ = segments(buf.getvalue())
        ours, _ = segments(J.encode(img, q))
        pick = lambda segs, m: b"".join(b for k, b in segs if k == m)  # noqa: E731
        assert pick(ours, 0xFFDB) == pick(theirs, 0xFFDB)
        # (libjpeg writes each DHT table as its own segment, the spec all four in one)
        assert pick(ours, 0xFFC4) == pick(theirs, 0xFFC4)


def test_marker_order_and_header_fields():
    segs, _ = segments(J.encode(np.zeros((37, 61, 3), dtype=np.uint8), 80))
    assert [m for m, _ in segs] == [0xFFE0, 0xFFDB, 0xFFC0, 0xFFC4, 0xFFDD, 0xFFDA]
    body = dict(segs)
    assert body[0xFFE0][:5] == b"JFIF\x00"
    assert struct.unpack(">BHHB", body[0xFFC0][:6]) == (8, 37, 61, 3)
    assert body[0xFFC0][6:] == bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])  # 4:4:4
    assert struct.unpack(">H", body[0xFFDD])[0] == 8  # one MCU row per restart interval
    assert len(J.header(61, 37, 80)) == 613


def test_integer_dct_is_near_the_float_dct():
    rs = np.random.RandomState(5)
    frames = [rs.randint(0, 256, (64, 64, 3)).astype(np.uint8), particle_frame(4000, 0.005)[:400, :400],
              np.full((16, 24, 3), 255, dtype=np.uint8), np.zeros((16, 24, 3), dtype=np.uint8)]
    for img in frames:
        s = J.blocks(img)
        U = J.dct(s)
        assert np.abs(U).max() < 2 ** 25
        assert np.abs(U / 2.0 ** 15 - J.float_dct(s)).max() < 0.5
        for q in (1, 50, 95, 100):
            Q = J.quant_tables(q)[[0, 1, 1]][None, None]
            exact = np.sign(J.float_dct(s)) * np.floor(np.abs(J.float_dct(s)) / Q + 0.5)
            assert np.abs(J.quantise(U, q) - exact).max() <= 1


def test_restart_markers_cycle_and_ff_is_stuffed():
    """Noise at quality 100: long codes, many 0xFF bytes.  134 rows: RST0..7 in turn, 133 of them."""
    img = np.random.RandomState(9).randint(0, 256, (1069, 45, 3)).astype(np.uint8)
    data = J.encode(img, 100)
    _, ecs = segments(data)
    b = np.frombuffer(ecs, dtype=np.uint8)
    ff = np.nonzero(b[:-1] == 0xFF)[0]
    nxt = b[ff + 1]
    assert b[-1] != 0xFF
    assert set(nxt.tolist()) <= {0x00} | set(range(0xD0, 0xD8))  # every 0xFF: stuffed, or a restart marker
    rst = nxt[nxt != 0] - 0xD0
    assert len(rst) == (1069 + 7) // 8 - 1
    assert rst.tolist() == [k % 8 for k in range(len(rst))]
    assert (nxt == 0).sum() > 1000
    assert psnr(decode(data), img) > 45  # (PIL reads it through every restart)


def test_restart_intervals_are_independent():
    """The DC predictor restarts every row: re-encoding one MCU row alone gives the same bytes."""
    img = np.random.RandomState(2).randint(0, 256, (24, 40, 3)).astype(np.uint8)
    rows = J.entropy_rows(J.coefficients(img, 75))
    for r in range(3):
        alone = J.entropy_rows(J.coefficients(img[8 * r:8 * r + 8], 75))
        assert alone[0].tobytes() == rows[r].tobytes()


def test_avi_structure(tmp_path):
    from sand_crate_amd.avi import AviWriter
    rs = np.random.RandomState(4)
    frames = [J.encode(rs.randint(0, 256, (48, 64, 3)).astype(np.uint8), q) for q in (10, 50, 90, 95, 100)]
    # lengths of both parities for certain (odd chunks get a pad byte; a decoder ignores what follows EOI)
    frames += [frames[0] + b"\x00" * (1 + len(frames[0]) % 2), frames[0] + b"\x00" * (2 - len(frames[0]) % 2)]
    path = tmp_path / "video.avi"
    with AviWriter(path, 64, 48) as avi:
        for f in frames:
            avi.write(f)
    data = path.read_bytes()

    def chunks(buf, start, end):
        i = start
        while i < end:
            fourcc, size = buf[i:i + 4], struct.unpack("<I", buf[i + 4:i + 8])[0]
            yield fourcc, i, size
            i += 8 + size + (size & 1)
        assert i == end

    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    top = list(chunks(data, 12, len(data)))
    assert [(c, data[i + 8:i + 12]) for c, i, _ in top[:2]] == [(b"LIST", b"hdrl"), (b"LIST", b"movi")]
    assert top[2][0] == b"idx1" and len(top) == 3
    _, h, hsize = top[0]
    hdrl = list(chunks(data, h + 12, h + 8 + hsize))
    assert hdrl[0][0] == b"avih" and hdrl[0][2] == 56
    avih = struct.unpack("<14I", data[hdrl[0][1] + 8:hdrl[0][1] + 64])
    assert avih[0] == 20000 and avih[4] == len(frames) and avih[6] == 1 and avih[8:10] == (64, 48)
    assert avih[3] & 0x10  # AVIF_HASINDEX
    _, s, ssize = hdrl[1]
    assert data[s + 8:s + 12] == b"strl"
    strl = list(chunks(data, s + 12, s + 8 + ssize))
    assert [c for c, _, _ in strl] == [b"strh", b"strf"]
    strh = data[strl[0][1] + 8:strl[0][1] + 8 + strl[0][2]]
    assert strh[:8] == b"vidsMJPG"
    scale, rate, _, length = struct.unpack("<4I", strh[20:36])
    assert rate / scale == 50 and length == len(frames)
    strf = data[strl[1][1] + 8:strl[1][1] + 48]
    assert struct.unpack("<Iii", strf[:12]) == (40, 64, 48) and strf[16:20] == b"MJPG"
    _, m, msize = top[1]
    movi = list(chunks(data, m + 12, m + 8 + msize))
    assert [c for c, _, _ in movi] == [b"00dc"] * len(frames)
    _, x, xsize = top[2]
    idx = [struct.unpack("<4sIII", data[x + 8 + 16 * k:x + 24 + 16 * k]) for k in range(xsize // 16)]
    assert len(idx) == len(frames)
    for (ckid, flags, off, size), (c, at, n), f in zip(idx, movi, frames):
        assert ckid == b"00dc" and flags & 0x10 and size == n == len(f)
        assert m + 8 + off == at  # offsets from the 'movi' fourcc
        assert data[at:at + 4] == b"00dc"
        body = data[at + 8:at + 8 + n]
        assert body == f
        assert decode(body).shape == (48, 64, 3)


def test_avi_refuses_to_pass_4_gib(tmp_path):
    from sand_crate_amd import avi as A
    w = A.AviWriter(tmp_path / "big.avi", 8, 8)
    w.write(b"\xff\xd8\xff\xd9")
    end = w._end
    w._end = A.RIFF_LIMIT - 64  # (as if nearly 4 GiB of frames had been written)
    with pytest.raises(ValueError, match="4 GiB"):
        w.write(b"\x00" * 100)
    w._end = end
    w.close()
    assert w.frames == 1 and (tmp_path / "big.avi").stat().st_size == end + 8 + 16
