"""CPU checks of the debug arrows: the pixel rule of tests/arrow_spec.py on arrows drawn by hand, the cases of
tests/arrow_cases.py (each has the property it is named for), the GIF palette with the arrows' entry, and the Python
plumbing that needs no GPU (`Crate`'s `arrows=` argument against a recording engine, the driver's --arrows, the ABI table).
The device pass is held to arrow_spec bit for bit by tests/test_gpu_arrows.py."""
import inspect

import numpy as np
import pytest

import arrow_cases as K
import arrow_spec as A
import gif_spec as G
import text_spec as T

CASES = K.cases()
VELOCITY = K.velocity_cases()


def picture(mask, x0, y0, w, h):
    return ["".join("#" if v else "." for v in row[x0:x0 + w]) for row in mask[y0:y0 + h]]


def boxes(case):
    return [A.box(a, case.width, case.height, case.zoom, case.center) for a in case.ends]


def lengths(case):
    out = []
    for a in case.ends:
        S = A.on_screen(a, case.width, case.height, case.zoom, case.center)
        out.append(None if S is None else float(np.hypot(S[2] - S[0], S[3] - S[1])))
    return out


# ---- the rule, by hand

def test_a_horizontal_arrow_of_six_pixels():
    """From S = (10, 10) to E = (16, 10): three rows of five body pixels, columns 10..14, and a head of 5, 3 and 1 pixels
    on columns 14, 15, 16."""
    arrow = [[K.world(10, 64), K.world(10, 48)], [K.world(16, 64), K.world(10, 48)]]
    assert A.on_screen(arrow, 64, 48) == (10.0, 10.0, 16.0, 10.0)
    got = A.covered(arrow, 64, 48)
    assert picture(got, 9, 7, 9, 7) == [".........",
                                        ".....#...",
                                        ".######..",
                                        ".#######.",
                                        ".######..",
                                        ".....#...",
                                        "........."]
    assert got.sum() == 3 * 5 + 5 + 3 + 1 - 3  # (column 14 is the body's last and the head's first)
    body = np.zeros((48, 64), dtype=bool)
    body[9:12, 10:15] = True
    head = np.zeros((48, 64), dtype=bool)
    head[8:13, 14] = head[9:12, 15] = head[10, 16] = True
    assert np.array_equal(got, body | head)


def test_the_four_axis_directions_are_rotations():
    c = CASES["axes"]
    assert K.to_cells(c.pairs, c.width, c.height).tolist() == [list(map(float, a)) for a in K.AXES]
    east, west, south, north = (A.covered(a, c.width, c.height) for a in c.ends)
    patch = east[7:14, 7:20]                                   # around S = (10, 10), E = (16, 10): 3 left, 3 right
    assert patch.sum() == east.sum() == 21
    assert np.array_equal(west[7:14, 31:44], patch[:, ::-1])   # S = (40, 10), E = (34, 10)
    assert np.array_equal(south[27:40, 7:14], patch.T)         # S = (10, 30), E = (10, 36)
    assert np.array_equal(north[27:40, 37:44], patch.T[::-1])  # S = (40, 36), E = (40, 30)
    assert west.sum() == south.sum() == north.sum() == 21


def test_short_arrows_have_no_body():
    """L = 1 along +x from S = (10, 10): the head alone -- t in [-1, 1], |w| <= 1 - t: column 10 (t = 0) is 3 high,
    column 11 the tip; column 9 (t = -1) would be 5 high but t >= L2 - 2 L = -1 holds there too."""
    arrow = [[K.world(10, 64), K.world(10, 48)], [K.world(11, 64), K.world(10, 48)]]
    got = A.covered(arrow, 64, 48)
    assert picture(got, 8, 7, 5, 7) == [".....", ".#...", ".##..", ".###.", ".##..", ".#...", "....."]
    # the body would add nothing a head of L < 2 does not have, but at L = 3 it is there: rows -1..1 from column 0 to 1
    longer = A.covered([[K.world(10, 64), K.world(10, 48)], [K.world(13, 64), K.world(10, 48)]], 64, 48)
    assert picture(longer, 9, 7, 6, 7) == ["......", "..#...", ".###..", ".####.", ".###..", "..#...", "......"]


def test_nothing_is_drawn():
    w, h = 64, 48
    p = [K.world(10, w), K.world(10, h)]
    assert not A.covered([p, p], w, h).any()                                   # L2 == 0
    assert not A.covered([p, [p[0] + 0.2 / (w - 1), p[1]]], w, h).any()         # ... also when only the screen points agree
    for bad in (np.nan, np.inf, -np.inf):
        for k in range(4):
            arrow = np.array([p, [K.world(20, w), K.world(10, h)]]).reshape(4)
            arrow[k] = bad
            assert A.on_screen(arrow, w, h) is None and not A.covered(arrow, w, h).any()
    assert A.on_screen([p, [1e308, 0.5]], w, h) is None                         # the screen number overflows
    outside = [[K.world(80, w), K.world(10, h)], [K.world(100, w), K.world(20, h)]]
    assert A.on_screen(outside, w, h) is not None and not A.covered(outside, w, h).any()
    assert A.box(outside, w, h) is None
    assert not A.mask(np.zeros((0, 2, 2)), w, h).any()


def test_compress_is_the_viewers_scaling():
    d = np.array([[0.3, -0.4], [0.0, 0.0], [1e-9, 0.0], [-5.0, 12.0]])
    got = A.compress(d)
    for k, (dx, dy) in enumerate(d):
        direction = np.array([dx, dy])
        want = direction / np.power(np.sqrt(dx * dx + dy * dy) + 0.001, 0.3)   # playback.py:99 with |d| spelt out
        assert np.array_equal(got[k], want)
    assert np.allclose(got[0], np.array([0.3, -0.4]) / 0.501 ** 0.3, rtol=1e-15)
    assert np.array_equal(got[1], [0.0, 0.0])
    pairs = np.array([[[0.5, 0.5], [0.3, -0.4]], [[np.nan, 0.5], [0.1, 0.1]], [[0.2, 0.2], [0.0, np.nan]]])
    ends = A.ends(pairs)
    assert ends.shape == (1, 2, 2) and np.array_equal(ends[0, 1], np.array([0.5, 0.5]) + got[0])
    from sand_crate_amd.crate import arrow_ends
    assert np.array_equal(arrow_ends(pairs), ends)          # the product's host-side copy of the same arithmetic
    for name, c in CASES.items():
        assert np.array_equal(arrow_ends(c.pairs), c.ends, equal_nan=True), name
    assert np.array_equal(arrow_ends([(np.array([0.5, 0.5]), np.array([0.3, -0.4]))]), ends)  # the reference's list form
    assert arrow_ends([]).shape == (0, 2, 2)


def test_uncompress_inverts_compress():
    for want in ([0.1, 0.0], [-0.03, 0.07], [2.0, -3.0], [1e-4, 1e-4]):
        assert np.allclose(A.compress(K.uncompress(want))[0], want, rtol=1e-12, atol=0)


# ---- the cases

def test_axis_cases_hit_the_equalities_on_pixels():
    """Integer S and a: t, w, L2 and L are whole numbers, so `t <= L2 - 2 L`, `w w <= L2` ... hold with equality on pixels."""
    c = CASES["axes"]
    for a in c.ends:
        S = A.on_screen(a, c.width, c.height)
        assert all(float(v).is_integer() for v in S)
        L2, L, t, w = A._terms(S, c.width, c.height)
        assert (L2, L) == (36.0, 6.0)
        cov = A.covered(a, c.width, c.height)
        assert (cov & (t == L2 - 2 * L)).sum() == 5          # the head's base, on the body's last column
        assert (cov & (t == 0)).sum() == 3 and (cov & (t == L2)).sum() == 1
        assert (cov & (np.abs(w) == L2 - t) & (t > L2 - 2 * L)).sum() == 3  # the head's slanted edges and its tip
        assert (cov & (w * w == L2)).sum() >= 10             # the body's long edges


def test_odd_frames_start_between_pixels():
    for name in ("odd_zoom_2.5", "odd_zoom_0.4"):
        c = CASES[name]
        assert c.width % 2 == 1 and c.height % 2 == 1 and c.center != (c.width / 2, c.height / 2)
        S = [A.on_screen(a, c.width, c.height, c.zoom, c.center) for a in c.ends]
        assert any(not float(s[0]).is_integer() for s in S) and any(not float(s[1]).is_integer() for s in S)
        assert A.mask(c.ends, c.width, c.height, c.zoom, c.center).sum() > 50
        assert sum(b is None for b in boxes(c)) <= 1         # (one has L2 == 0)
    assert CASES["odd_zoom_2.5"].zoom == 2.5 and CASES["odd_zoom_0.4"].zoom == 0.4


def test_diagonal_and_random_cases():
    c = CASES["diagonal"]
    S = [A.on_screen(a, c.width, c.height) for a in c.ends]
    assert all(abs(s[2] - s[0]) == abs(s[3] - s[1]) > 0 for s in S)
    for name in ("random", "random_zoomed"):
        c = CASES[name]
        ls = [v for v in lengths(c) if v]
        assert len(c.pairs) == 60 and min(ls) < 6 and max(ls) > 25
        area = [b[2] * b[3] for b in boxes(c) if b]
        assert min(area) <= A.WAVE_BOX < max(area)           # both of the kernel's paths
    assert CASES["random_zoomed"].zoom not in (1.0, 2.0) and CASES["random_zoomed"].width % 2 == 1


def test_lengths_around_two():
    below, exact, above = (CASES[n] for n in ("L_below_2", "L_exactly_2", "L_above_2"))
    for c, check in ((below, lambda v: 2 - 1e-6 < v < 2), (exact, lambda v: v == 2.0), (above, lambda v: 2 < v < 2 + 1e-6)):
        ls = lengths(c)
        assert all(check(v) for v in ls[:4]), ls             # one cell along each axis direction
        assert ls[4] > 2.8 and ls[5] == 0.0                  # a diagonal cell, and L2 == 0
        assert boxes(c)[5] is None and all(b is not None for b in boxes(c)[:5])
    count = {n: int(A.covered(CASES[n].ends[0], 64, 48, CASES[n].zoom, CASES[n].center).sum())
             for n in ("L_below_2", "L_exactly_2", "L_above_2")}
    for c in (below, exact, above):
        S = A.on_screen(c.ends[0], 64, 48, c.zoom, c.center)
        L2 = A._terms(S, 64, 48)[0]
        assert (L2 >= 4.0) == (c is not below)               # the body's switch
    assert count["L_exactly_2"] > count["L_below_2"]          # at exactly 2 the equalities are hit on pixels


def test_nonfinite_case():
    c = CASES["nonfinite"]
    assert np.isnan(c.pairs).any(axis=(1, 2)).sum() == 2 and np.isinf(c.pairs).any(axis=(1, 2)).sum() == 4
    assert len(c.ends) == 5                                  # the NaN entries are dropped on the host
    drawn = [b is not None for b in boxes(c)]
    assert drawn == [False, True, False, False, False]       # only the one good arrow
    assert not np.isfinite(c.ends[3:]).all(axis=(1, 2)).any()  # an infinite direction makes an end that is not finite
    assert A.mask(c.ends, 64, 48).sum() == A.covered(c.ends[1], 64, 48).sum() > 20


def test_edges_case():
    c = CASES["edges"]
    w, h = c.width, c.height
    ends = c.ends
    assert len(ends) == 18
    for a in ends[:6]:                                       # half outside: drawn, and cut by the frame
        x0, y0, bw, bh = A.box(a, w, h)
        assert A.covered(a, w, h).any() and (x0 == 0 or y0 == 0 or x0 + bw == w or y0 + bh == h)
    touched = set()
    for a in ends[:6]:
        cov = A.covered(a, w, h)
        touched |= {s for s, hit in (("l", cov[:, 0].any()), ("r", cov[:, -1].any()), ("t", cov[0].any()),
                                     ("b", cov[-1].any())) if hit}
    assert touched == {"l", "r", "t", "b"}
    for a in ends[6:12]:                                     # wholly outside
        assert A.on_screen(a, w, h) is not None and A.box(a, w, h) is None and not A.covered(a, w, h).any()
    assert np.abs(c.pairs[12:16]).max() == 1e300
    for a in ends[12:16]:                                    # 1e300: L2 overflows or is 0, nothing is drawn
        assert not A.covered(a, w, h).any()
    for a in ends[16:]:                                      # far, finite: the body crosses the frame to its edge
        S = A.on_screen(a, w, h)
        assert max(abs(v) for v in S) > 1e4 and A.box(a, w, h)[2] * A.box(a, w, h)[3] > A.WAVE_BOX
        assert A.covered(a, w, h).sum() > 30


def test_boxes_on_each_side_of_the_wave_threshold():
    assert A.WAVE_BOX == 256
    area = lambda c: [b[2] * b[3] for b in boxes(c)]
    assert area(CASES["box_at_threshold"]) == [256, 252]
    assert area(CASES["box_over_threshold"]) == [272, 259]
    assert area(CASES["box_both"]) == [256, 272, 252, 7 * 37]
    c = CASES["whole_frame"]
    assert boxes(c) == [(0, 0, 128, 96)] and A.covered(c.ends[0], 128, 96)[[0, 95], [0, 127]].all()
    import re
    from pathlib import Path
    text = (Path(__file__).resolve().parent.parent / "sand_crate_amd" / "csrc" / "sc_arrows.h").read_text()
    assert int(re.search(r"kArrowWaveBox = (\d+);", text).group(1)) == A.WAVE_BOX
    assert int(re.search(r"kArrowMargin = (\d+);", text).group(1)) == A.MARGIN


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_covered_pixel_is_in_its_box(name):
    c = CASES[name]
    assert c.width <= 256 and c.height <= 192 and len(c.pairs) <= 4096
    for a in c.ends[:200]:
        cov = A.covered(a, c.width, c.height, c.zoom, c.center)
        b = A.box(a, c.width, c.height, c.zoom, c.center)
        if b is None:
            assert not cov.any()
            continue
        inside = np.zeros_like(cov)
        inside[b[1]:b[1] + b[3], b[0]:b[0] + b[2]] = True
        assert not (cov & ~inside).any()


def test_pile_case():
    c = CASES["pile"]
    assert len(c.pairs) == 4096
    cells = K.to_cells(c.pairs, 64, 48)
    assert (cells[:, :2] == [32, 24]).all() and len(np.unique(cells[:, 2:], axis=0)) == 15 * 15
    assert 150 < A.mask(c.ends, 64, 48).sum() < 23 * 23


def test_layers_case_crosses_the_text():
    c = CASES["layers"]
    ink = T.ink(c.hud, T.MARGIN, T.MARGIN, 1, c.width, c.height)
    arrows = A.mask(c.ends, c.width, c.height)
    assert (ink & arrows).sum() > 20 and (arrows & ~ink).sum() > 500
    box = (slice(6, 6 + 36), slice(6, 6 + 8 * 27))
    assert (arrows[box] & ~ink[box]).any()                   # arrow pixels show between the glyphs
    assert arrows[:10].any() and arrows[:, :10].any()        # ... and over the wall at the frame's edge (test_gpu_arrows)
    frame = np.zeros((c.height, c.width, 3), dtype=np.uint8)
    both = T.draw(A.draw(frame, c.ends), c.hud)
    assert (both[ink] == 255).all() and (both[arrows & ~ink] == A.GREEN).all() and not both[~arrows & ~ink].any()


def test_masks_band():
    c = CASES["random_zoomed"]
    exact = A.mask(c.ends, c.width, c.height, c.zoom, c.center)
    sure_in, sure_out = A.arrow_masks(c.ends, c.width, c.height, c.zoom, c.center)
    assert not (sure_in & ~exact).any() and not (sure_out & exact).any() and not (sure_in & sure_out).any()
    assert (~sure_in & ~sure_out).sum() <= 0.01 * sure_in.sum()
    # integer arrows sit on their equalities: the band must find them
    a = CASES["axes"]
    s_in, s_out = A.arrow_masks(a.ends, a.width, a.height)
    assert (~s_in & ~s_out).sum() >= 4 * 12 and not (s_in & s_out).any()
    wide_in, wide_out = A.arrow_masks(c.ends, c.width, c.height, c.zoom, c.center, slack=0.5)
    assert wide_in.sum() < sure_in.sum() and wide_out.sum() < sure_out.sum()


@pytest.mark.parametrize("name", sorted(VELOCITY))
def test_velocity_inputs_stay_clear_of_the_band(name):
    """A condition on the inputs, from the spec alone: at most 1 % of the covered pixels are within the slack of an
    edge, and no end is within 1e-6 of a cell boundary, where the view's trunc would turn last bits into a pixel."""
    v = VELOCITY[name]
    ends = v.ends
    assert len(v.xy) <= 2048 and v.width <= 256 and v.height <= 192
    assert len(ends) == len(range(0, len(v.xy), v.every))
    undecided, sure = K.undecided_share(ends, v.width, v.height, v.zoom, v.center)
    assert sure > 1000 and undecided <= 0.01 * sure, (undecided, sure)
    assert K.trunc_room(ends, v.width, v.height) > 1e-6
    area = [b[2] * b[3] for b in (A.box(a, v.width, v.height, v.zoom, v.center) for a in ends) if b]
    assert min(area) <= A.WAVE_BOX and (v.scale < 0.1 or max(area) > A.WAVE_BOX)
    drawn = sum(b is not None for b in (A.box(a, v.width, v.height, v.zoom, v.center) for a in ends))
    assert drawn < len(ends)                                  # particles at rest, outside, or not finite draw nothing


def test_velocity_ends_pick_ids():
    xy = np.arange(12, dtype=np.float64).reshape(6, 2) / 12
    vxy = np.ones((6, 2))
    ids = np.array([5, 0, 9, 3, 4, 6])
    ends = A.velocity_ends(xy, vxy, ids, 0.5, 3)
    assert np.array_equal(ends[:, 0], xy[[1, 2, 3, 5]])
    assert np.array_equal(ends[:, 1], xy[[1, 2, 3, 5]] + A.compress([[0.5, 0.5]]))


# ---- GIF

def test_palette_with_arrows():
    from sand_crate_amd import gif
    plain = bytes(3) + b"".join(bytes((k, k, 255)) for k in range(1, 256))
    assert gif.palette() == gif.palette(False) == gif.palette(arrows=False) == plain == G.palette().tobytes()
    with_arrows = gif.palette(arrows=True)
    assert len(with_arrows) == 768 and with_arrows[3:6] == bytes((0, 255, 0))
    assert with_arrows[:3] == plain[:3] and with_arrows[6:] == plain[6:]
    assert with_arrows == A.palette().tobytes()


def test_gif_writer_header_with_arrows(tmp_path):
    from sand_crate_amd.gif import GifWriter
    idx = np.zeros((5, 7), dtype=np.uint8)
    idx[1, 2:5] = 1
    idx[3, 1] = 2
    data = G.image_data(idx)
    files = {}
    for arrows in (False, True):
        path = tmp_path / f"{arrows}.gif"
        with GifWriter(path, 7, 5, **({"arrows": True} if arrows else {})) as w:
            w.write(data)
        files[arrows] = path.read_bytes()
    assert files[False] == G.file([idx])                      # without the flag: today's file, byte for byte
    assert len(files[True]) == len(files[False])
    differ = [k for k in range(len(files[True])) if files[True][k] != files[False][k]]
    assert differ == [13 + 3, 13 + 4, 13 + 5]                 # entry 1 of the global colour table
    frames, pal, _, _ = G.decode(files[True])
    assert np.array_equal(frames[0], idx) and np.array_equal(pal, A.palette())


def test_indices_with_arrows():
    frame = np.zeros((2, 4, 3), dtype=np.uint8)
    frame[0, 1] = (0, 0, 255)
    frame[0, 2] = (1, 1, 255)
    frame[0, 3] = (2, 2, 255)
    frame[1, 0] = (200, 200, 255)
    frame[1, 1] = (255, 255, 255)
    frame[1, 2] = A.GREEN
    assert A.indices(frame).tolist() == [[0, 2, 2, 2], [200, 255, 1, 0]]
    assert G.indices(frame[:, :2]).tolist() == [[0, 1], [200, 255]]  # (without arrows, as before)
    assert np.array_equal(A.palette()[A.indices(frame)][1], frame[1])


# ---- Python plumbing

class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_hud(self, text, x=6, y=6, scale=1):
        pass

    def set_arrows(self, mode, arrows=None, scale=1.0, every=1):
        self.calls.append((mode, None if arrows is None else np.array(arrows, dtype=np.float64).reshape(-1, 2, 2), scale,
                           every))

    def render(self, view, segments, out=None):
        return "frame"

    def render_jpeg(self, view, segments, quality=95):
        return b"jpeg"

    def render_gif(self, view, segments):
        return b"gif"


def recording_crate():
    from sand_crate_amd import Crate
    from sand_crate_amd.addons import Overlay
    crate = object.__new__(Crate)  # (no GPU context: only what the frame calls touch)
    crate._engine = RecordingEngine()
    crate._overlay = Overlay()
    crate._debug_prints = ""
    crate.debug_arrows = []
    crate.particle_radius = 0.01
    crate.dt = 0.002
    crate.rigid_bodies = []
    return crate


def test_crate_sends_the_arrows_only_when_they_change():
    from sand_crate_amd import _native as N
    crate = recording_crate()
    calls = crate._engine.calls
    assert crate.render(64, 48) == "frame" and crate.render_gif(64, 48, arrows=False) == b"gif" and not calls
    crate.render(64, 48, arrows=True)                         # an empty debug_arrows: nothing to draw is no arrows
    assert not calls
    pairs = CASES["nonfinite"].pairs
    crate.debug_arrows = [(s, d) for s, d in pairs]
    crate.render(64, 48, arrows=True)
    assert len(calls) == 1 and calls[0][0] == N.ARROWS_LIST
    assert np.array_equal(calls[0][1], A.ends(pairs), equal_nan=True)
    crate.render_jpeg(64, 48, arrows=True)
    crate.render_gif(64, 48, arrows=pairs)                    # the same list as an array
    crate.render(64, 48, arrows=pairs.tolist())
    assert len(calls) == 1
    crate.render(64, 48, arrows=pairs[3:4])
    assert len(calls) == 2 and np.array_equal(calls[1][1], A.ends(pairs[3:4]))
    crate.render(64, 48, arrows="velocity")
    assert calls[-1] == (N.ARROWS_VELOCITY, None, 0.002, 1) and len(calls) == 3   # the default scale is dt
    crate.render_gif(64, 48, arrows="velocity", arrow_scale=0.002, arrow_every=1)
    assert len(calls) == 3
    crate.render_jpeg(64, 48, arrows="velocity", arrow_every=8, arrow_scale=0.5)
    assert calls[-1] == (N.ARROWS_VELOCITY, None, 0.5, 8) and len(calls) == 4
    crate.render(64, 48)                                      # a call without them clears, once
    crate.render_gif(64, 48, arrows=None)
    assert calls[-1][0] == N.ARROWS_OFF and len(calls) == 5
    crate.render(64, 48, arrows=np.zeros((0, 2, 2)))
    assert len(calls) == 5
    for bad in (7, "speed", {"a": 1}, np.zeros((3, 3)), [[0.5, 0.5, 0.1]], object()):
        with pytest.raises(TypeError):
            crate.render(64, 48, arrows=bad)
    assert len(calls) == 5


def test_grow_forgets_what_was_sent():
    """The overlay across a growth (`leave` the old context, `enter` the new one): a HUD and arrows that were sent are
    both sent again, to the new engine, with the next frame -- once -- and the old engine hears nothing more."""
    from sand_crate_amd import _native as N

    class Both(RecordingEngine):
        def set_hud(self, text, x=6, y=6, scale=1):
            self.calls.append(("hud", text, x, y, scale))

    crate = recording_crate()
    crate._engine = old = Both()
    new = Both()
    crate.render(64, 48, hud="grown", arrows="velocity", arrow_every=4)
    sent = [("hud", b"grown", 6, 6, 1), (N.ARROWS_VELOCITY, None, 0.002, 4)]
    assert old.calls == sent
    crate._overlay.leave(old)
    crate._engine = new
    crate._overlay.enter(new)
    assert old.calls == sent and new.calls == []              # (nothing until a frame asks for it)
    crate.render_gif(64, 48, hud="grown", arrows="velocity", arrow_every=4)
    crate.render(64, 48, hud="grown", arrows="velocity", arrow_every=4)
    assert new.calls == sent and old.calls == sent
    crate._overlay.enter(new)                                  # a context that draws nothing is not told to draw nothing
    crate.render(64, 48)
    assert new.calls == sent


def test_engine_binding_lists_the_call():
    import ctypes
    from sand_crate_amd import _native
    from sand_crate_amd.engine import Engine
    assert "sc_set_arrows" in _native.SIGNATURES and callable(Engine.set_arrows)
    assert ctypes.sizeof(_native.Arrow) == 4 * 8
    assert (_native.ARROWS_OFF, _native.ARROWS_LIST, _native.ARROWS_VELOCITY) == (0, 1, 2)
    assert _native.MAX_ARROWS == A.MAX_ARROWS == 1048576
    sig = inspect.signature(Engine.set_arrows).parameters
    assert list(sig) == ["self", "mode", "arrows", "scale", "every"]
    assert (sig["arrows"].default, sig["scale"].default, sig["every"].default) == (None, 1.0, 1)


def test_library_exports_the_call():
    import ctypes
    from sand_crate_amd import build
    lib = ctypes.CDLL(str(build.build()))
    assert hasattr(lib, "sc_set_arrows")
    lib.sc_abi_version.restype = ctypes.c_int
    assert lib.sc_abi_version() == 5


def test_driver_accepts_arrows():
    from sand_crate_amd.main import HeadlessPlayback, argument_parser, main
    a = argument_parser().parse_args(["config/wave_machine.yaml", "out", "--gif", "--arrows", "--variants", "1"])
    assert a.arrows == 1 and a.gif is True and a.variants == 1
    a = argument_parser().parse_args(["config/wave_machine.yaml", "out", "--arrows", "8", "--gif"])
    assert a.arrows == 8
    assert argument_parser().parse_args(["config/wave_machine.yaml"]).arrows == 0
    assert inspect.signature(main).parameters["arrows"].default == 0
    assert inspect.signature(HeadlessPlayback.__init__).parameters["arrows"].default == 0
    for f in ("render", "render_jpeg", "render_gif"):
        from sand_crate_amd import Crate
        p = inspect.signature(getattr(Crate, f)).parameters
        assert (p["arrows"].default, p["arrow_every"].default, p["arrow_scale"].default) == (None, 1, None)
