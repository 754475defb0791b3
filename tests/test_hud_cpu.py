"""CPU checks of the HUD: the font table (sand_crate_amd/hud_font.py) and its committed C copy, the pixel rule of
tests/text_spec.py on the cases of tests/hud_cases.py, the default placement, and the Python plumbing that needs no GPU
(`Crate`'s `hud=` argument against a recording engine, the driver's --hud)."""
from pathlib import Path

import numpy as np
import pytest

import hud_cases as K
import text_spec as T
from sand_crate_amd import hud_font as F

ROOT = Path(__file__).resolve().parent.parent
CASES = K.cases()


def glyphs():
    return [F.FONT[16 * k:16 * k + 16] for k in range(95)]


# ---- the font

def test_table_size_and_cell():
    assert len(F.FONT) == 95 * 16 == 1520 and (F.CELL_W, F.CELL_H, F.FIRST, F.LAST) == (8, 16, 0x20, 0x7E)
    assert F.LINE_PITCH == T.PITCH == 18 and F.MARGIN == T.MARGIN == 6


def test_glyph_rules():
    g = glyphs()
    assert not any(g[0])  # space is empty
    for k in range(1, 95):
        assert any(g[k]), f"glyph {chr(0x20 + k)!r} has no ink"
    assert len(set(g)) == 95, "two glyphs are the same"
    for k, rows in enumerate(g):
        assert not any(r & 1 for r in rows), f"the rightmost column of {chr(0x20 + k)!r} is not empty"
        assert rows[0] == 0 and rows[15] == 0, f"row 0 or 15 of {chr(0x20 + k)!r} is not empty"


def test_glyph_lookup():
    assert F.glyph(ord("A")) == glyphs()[ord("A") - 0x20]
    for byte in (0x00, 0x09, 0x0A, 0x1F, 0x7F, 0x80, 0xFF):
        assert F.glyph(byte) == F.glyph(ord("?"))


def test_committed_header_is_the_generators_output():
    assert (ROOT / "sand_crate_amd" / "csrc" / "sc_font.h").read_text() == F.c_header()


def test_header_holds_the_table():
    import re
    text = (ROOT / "sand_crate_amd" / "csrc" / "sc_font.h").read_text()
    body = text[text.index("kFontTable"):]
    body = body[body.index("{") + 1:body.index("};")]
    assert bytes(int(v, 16) for v in re.findall(r"0x([0-9A-F]{2}),", body)) == F.FONT


def test_committed_specimen_is_the_generators_output():
    assert (ROOT / "docs" / "hud_font.txt").read_text() == F.specimen()


# ---- the pixel rule

def test_one_glyph_by_hand():
    """`T` at (1, 2) on a frame of 10 x 20, drawn here by hand from docs/hud_font.txt."""
    want = np.zeros((20, 10), dtype=bool)
    want[2 + 3, 1:8] = True        # the bar: glyph row 3, columns 0..6
    want[2 + 4:2 + 12, 1 + 3] = True  # the stem: rows 4..11, column 3
    assert np.array_equal(T.ink(b"T", 1, 2, 1, 10, 20), want)


def test_lines_split_like_str_split():
    for text in (b"", b"a", b"a\n", b"\n", b"\n\n", b"a\n\nb", b"a\nb\n"):
        assert [s.decode() for s in T.lines(text)] == text.decode().split("\n")


@pytest.mark.parametrize("name", sorted(CASES))
def test_box_of_every_case(name):
    c = CASES[name]
    assert T.box(c.text, c.x, c.y, c.scale, c.width, c.height) == c.box


@pytest.mark.parametrize("name", sorted(CASES))
def test_ink_stays_in_the_clipped_box(name):
    c = CASES[name]
    ink = T.ink(c.text, c.x, c.y, c.scale, c.width, c.height)
    assert ink.shape == (c.height, c.width)
    inside = np.zeros_like(ink)
    inside[c.y:c.y + c.box[1], c.x:c.x + c.box[0]] = True
    assert not (ink & ~inside).any()
    if name not in ("outside", "only_newline", "corner"):  # (corner: a `T`'s first row is empty)
        assert ink.any()
        # ... and the box is no larger than it has to be: the text's cells reach its last column and row
        assert c.box[0] == min(c.width - c.x, max(map(len, T.lines(c.text))) * 8 * c.scale)
    else:
        assert not ink.any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_short_lines_and_leading(name):
    c = CASES[name]
    ink = T.ink(c.text, c.x, c.y, c.scale, c.width, c.height)
    pitch = 18 * c.scale
    for l, line in enumerate(T.lines(c.text)):
        rows = ink[c.y + l * pitch:c.y + (l + 1) * pitch]
        assert not rows[:, c.x + len(line) * 8 * c.scale:].any(), f"line {l} draws past its end"
        assert not rows[16 * c.scale:].any(), f"line {l} draws into its leading"
        assert not rows[:c.scale].any() and not rows[15 * c.scale:].any()  # the glyphs' empty rows 0 and 15
    assert not ink[c.y + len(T.lines(c.text)) * pitch:].any() and not ink[:c.y].any() and not ink[:, :c.x].any()


def test_cut_glyphs_show_the_part_that_fits():
    c = CASES["cut"]
    ink = T.ink(c.text, c.x, c.y, c.scale, c.width, c.height)
    wide = T.ink(c.text, c.x, c.y, c.scale, 200, 200)
    assert np.array_equal(ink, wide[:c.height, :c.width])
    assert ink[:, 62:].any() and wide[:, 64:].any()          # the eighth glyph, cut after two columns
    assert ink[42:].any() and wide[48:, :].any()             # the third line, cut after six rows
    assert wide[6 + 54:6 + 72].any()                         # the fourth line lies below the frame


@pytest.mark.parametrize("name", sorted(CASES))
def test_scale_three_is_scale_one_repeated(name):
    c = CASES[name]
    if c.scale != 1:
        return
    one = T.ink(c.text, c.x, c.y, 1, c.width, c.height)
    three = T.ink(c.text, 3 * c.x, 3 * c.y, 3, 3 * c.width, 3 * c.height)
    assert np.array_equal(three, np.repeat(np.repeat(one, 3, axis=0), 3, axis=1))


def test_bytes_outside_the_font_are_question_marks():
    odd = bytes([0x00, 0x09, 0x1F, 0x7F, 0x80, 0xFF, 0x0D])
    assert np.array_equal(T.ink(odd, 2, 2, 1, 80, 24), T.ink(b"?" * len(odd), 2, 2, 1, 80, 24))
    c = CASES["all_glyphs"]
    ink = T.ink(c.text, c.x, c.y, 1, c.width, c.height)
    cells = [ink[6 + 18 * 6:6 + 18 * 7, 6 + 8 * k:6 + 8 * (k + 1)] for k in range(3)]  # the last line: 0x09, 0x7F, 0xFF
    assert all(np.array_equal(cell[:16], T.glyph_bits(ord("?"))) for cell in cells)


def test_draw_writes_white_and_leaves_the_rest():
    rs = np.random.RandomState(3)
    c = CASES["cut"]
    ink = T.ink(c.text, c.x, c.y, c.scale, c.width, c.height)
    rgb = rs.randint(0, 255, (c.height, c.width, 3)).astype(np.uint8)  # (no 255 anywhere)
    before = rgb.copy()
    out = T.draw(rgb, c.text, c.x, c.y, c.scale)
    assert np.array_equal(rgb, before)  # a copy
    assert (out[ink] == 255).all() and np.array_equal(out[~ink], rgb[~ink])
    idx = rs.randint(0, 255, (c.height, c.width)).astype(np.uint8)
    out = T.draw(idx, c.text, c.x, c.y, c.scale)
    assert (out[ink] == 255).all() and np.array_equal(out[~ink], idx[~ink])
    import gif_spec as G
    assert np.array_equal(G.indices(T.draw(np.zeros_like(rgb), c.text, c.x, c.y, c.scale)), np.where(ink, 255, 0))


# ---- placement

def test_default_scale_and_placement():
    want = {59: 1, 60: 1, 1000: 1, 1439: 1, 1440: 2, 16384: 17}
    for width, scale in want.items():
        assert T.default_scale(width) == scale and F.default_scale(width) == scale
        assert F.default_placement(width) == (6, 6, scale)


# ---- Python plumbing

class RecordingEngine:
    def __init__(self):
        self.calls = []

    def set_hud(self, text, x=6, y=6, scale=1):
        self.calls.append((text, x, y, scale))

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
    crate._debug_prints = "Tick: 3\nParticles: 5\n"
    crate.debug_arrows = []
    crate.particle_radius = 0.01
    crate.dt = 0.002
    crate.rigid_bodies = []
    return crate


def test_crate_sends_the_hud_only_when_it_changes():
    crate = recording_crate()
    calls = crate._engine.calls
    assert crate.render(64, 48) == "frame" and crate.render_gif(64, 48, hud=False) == b"gif" and not calls
    crate.render(64, 48, hud=True)
    assert calls == [(b"Tick: 3\nParticles: 5\n", 6, 6, 1)]
    crate.render_jpeg(64, 48, hud=True)
    crate.render_gif(64, 48, hud="Tick: 3\nParticles: 5\n")
    assert len(calls) == 1                                  # the same text, placement and scale
    crate.render_gif(1440, 48, hud=True)
    assert calls[-1] == (b"Tick: 3\nParticles: 5\n", 6, 6, 2) and len(calls) == 2  # the scale follows the width
    crate.render(64, 48, hud="café ☃")
    assert calls[-1] == (b"caf? ?", 6, 6, 1) and len(calls) == 3  # encode("ascii", "replace")
    crate.debug_prints = "Tick: 4\n"
    crate.render(64, 48, hud=True)
    assert calls[-1][0] == b"Tick: 4\n" and len(calls) == 4
    crate.render(64, 48)                                     # a call without one clears it, once
    crate.render_jpeg(64, 48, hud=None)
    assert calls[-1][0] is None and len(calls) == 5
    crate.render(64, 48, hud="")                             # nothing to draw is no HUD
    assert len(calls) == 5
    with pytest.raises(TypeError):
        crate.render(64, 48, hud=7)


def test_player_sends_the_hud_only_when_it_changes():
    """`track.Player` shares the crate's overlay code: the same call sequence, with the frame's own two lines for True,
    and again from the start in the engine a larger frame makes it open."""
    import track_spec
    from sand_crate_amd.addons import Overlay
    from sand_crate_amd.engine import Engine
    from sand_crate_amd.track import Player

    class PlayerEngine(RecordingEngine):
        capacity = 8

        def track_load(self, frame, plain=False):
            pass

        def close(self):
            pass

    made = []

    class Opened(PlayerEngine):                               # what `load` opens for a frame beyond the capacity
        view = staticmethod(Engine.view)

        def __init__(self, capacity, device=0):
            super().__init__()
            self.capacity = capacity
            made.append(self)

    def frame(tick, n):
        xy = np.full((n, 2), 0.5)
        return track_spec.pack(tick, xy, np.zeros(n), np.arange(n), np.zeros((0, 2, 2)))

    player = object.__new__(Player)  # (no GPU context: only what the frame calls touch)
    player._Engine, player._engine, player._overlay = Opened, PlayerEngine(), Overlay()
    player.device, player.particle_radius, player._fixed = 0, 0.01, False
    calls = player._engine.calls
    small = frame(3, 5)
    assert player.render(small, 64, 48) == "frame" and player.render_gif(small, 64, 48, hud=False) == b"gif" and not calls
    player.render(small, 64, 48, hud=True)
    assert calls == [(b"Tick: 3\nParticles: 5", 6, 6, 1)]
    player.render_jpeg(small, 64, 48, hud=True)
    player.render_gif(small, 64, 48, hud="Tick: 3\nParticles: 5")
    assert len(calls) == 1                                  # the same text, placement and scale
    player.render_gif(small, 1440, 48, hud=True)
    assert calls[-1] == (b"Tick: 3\nParticles: 5", 6, 6, 2) and len(calls) == 2  # the scale follows the width
    player.render(small, 64, 48, hud="café ☃")
    assert calls[-1] == (b"caf? ?", 6, 6, 1) and len(calls) == 3  # encode("ascii", "replace")
    player.render(frame(4, 5), 64, 48, hud=True)
    assert calls[-1][0] == b"Tick: 4\nParticles: 5" and len(calls) == 4
    player.render(small, 64, 48)                             # a call without one clears it, once
    player.render_jpeg(small, 64, 48, hud=None)
    assert calls[-1][0] is None and len(calls) == 5
    player.render(small, 64, 48, hud="")                     # nothing to draw is no HUD
    assert len(calls) == 5
    with pytest.raises(TypeError):
        player.render(small, 64, 48, hud=7)
    player.render(small, 64, 48, hud="kept")
    assert len(calls) == 6 and not made
    player.render(frame(5, 9), 64, 48, hud="kept")           # nine particles: a new engine, which has no HUD yet
    assert len(made) == 1 and player.engine is made[0] and made[0].calls == [(b"kept", 6, 6, 1)] and len(calls) == 6


def test_engine_binding_lists_the_call():
    from sand_crate_amd import _native
    from sand_crate_amd.engine import Engine
    assert "sc_set_hud" in _native.SIGNATURES and callable(Engine.set_hud)


def test_driver_accepts_hud():
    from sand_crate_amd.main import argument_parser
    a = argument_parser().parse_args(["config/wave_machine.yaml", "out", "--gif", "--hud", "--variants", "1"])
    assert a.hud is True and a.gif is True and a.variants == 1
    assert argument_parser().parse_args(["config/wave_machine.yaml"]).hud is False
    import inspect
    from sand_crate_amd.main import HeadlessPlayback, main
    assert inspect.signature(main).parameters["hud"].default is False
    assert inspect.signature(HeadlessPlayback.__init__).parameters["hud"].default is False
