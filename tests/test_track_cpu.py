"""The packed frame without a GPU: the spec's own round trips (tests/track_spec.py), `sand_crate_amd.track` against it
(`frame_bytes`, `parse`, the track.sctk writer and reader, truncation), that the cases of tests/track_cases.py tell the
spec's rules from the plausible wrong ones, and `sand_crate_amd.replay`'s argument parsing and output naming."""
import struct
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import track_cases as K
import track_spec as S


# ---- the spec's own promises

def test_every_code_survives_dequantise_quantise():
    q = np.arange(65536, dtype=np.uint16)
    x = S.dequantise(q)
    assert np.isposinf(x[65535]) and np.isfinite(x[:65535]).all()
    assert np.array_equal(S.quantise(x), q)
    assert x[0] == S.LO == -0.25 and S.quantise([-0.25, 1.25]).tolist() == [0, 65534]
    assert abs(x[65534] - 1.25) < 1e-15


def test_the_error_is_at_most_half_a_step():
    rs = np.random.RandomState(3)
    x = np.concatenate([rs.rand(200_000) * S.SPAN + S.LO, K.finite_coordinates()])
    x = x[(x >= S.LO) & (x <= S.LO + S.SPAN)]
    err = np.abs(S.dequantise(S.quantise(x)) - x)
    assert 1.1444e-5 < S.HALF_STEP < 1.1445e-5 and err.max() <= S.HALF_STEP + S.ROUNDING
    assert err.max() > 0.99 * S.STEP / 2                                  # (the half-step cases reach the bound)
    assert S.HALF_STEP * 999 < 0.0115                                     # 0.011 pixel at a width of 1000


def test_out_of_range_clamps_and_not_finite_is_its_own_code():
    lo, hi = S.LO, S.LO + S.SPAN
    assert S.quantise([lo - S.STEP, np.nextafter(lo, -np.inf), -1e300, hi + S.STEP, np.nextafter(hi, np.inf), 1e300]).tolist() \
        == [0, 0, 0, 65534, 65534, 65534]
    assert S.quantise([np.nan, np.inf, -np.inf]).tolist() == [65535] * 3
    assert S.quantise([0.0, -0.0]).tolist() == [10922, 10922] and S.quantise([1.0]).tolist() == [54612]


def test_colour_inversion_holds_for_every_byte():
    c = np.arange(256, dtype=np.uint8)
    assert np.array_equal(S.colour(S.pressure_of(c)), c)
    assert S.colour([np.nan, np.inf, -np.inf, 0.0, 1.0, 2.0, -1.0]).tolist() == [0, 0, 255, 255, 0, 0, 255]


def test_colour_is_the_renderers():
    import render_spec
    p = K.pressures()
    assert np.array_equal(S.colour(p), render_spec.colour(p))


# ---- frames

def frame_of(n, n_segments, seed=1, tick=7, valid=True):
    rs = np.random.RandomState(seed + n)
    xy = rs.rand(n, 2) * 1.7 - 0.35
    return S.pack(tick, xy, rs.rand(n) * 1.2 - 0.1, rs.permutation(n) + 5, K.walls(n_segments), valid), xy


@pytest.mark.parametrize("n", K.COUNTS)
def test_frame_bytes_and_parse(n):
    from sand_crate_amd import track
    for s in K.SEGMENT_COUNTS:
        frame, xy = frame_of(n, s)
        assert len(frame) == S.frame_bytes(n, s) == track.frame_bytes(n, s) == track.frame_length(frame[:64])
        assert len(frame) % 8 == 0 and all(o % 8 == 0 for o in S.planes(n, s))
        a, b = S.parse(frame), track.parse(frame)
        assert a["tick"] == b["tick"] == 7 and a["n"] == b["n"] == n and b["flags"] == 1 and b["pressure_valid"]
        assert np.array_equal(b["segments"], K.walls(s)) and b["segments"].shape == (s, 2, 2)
        assert np.array_equal(b["ids"], a["ids"]) and b["ids"].dtype == np.int64 and sorted(b["ids"]) == list(range(5, n + 5))
        assert np.array_equal(b["particles"], a["xy"]) and b["particles"].shape == (n, 2)
        assert np.array_equal(b["colour"], a["c"]) and np.array_equal(b["pressure"], S.pressure_of(a["c"]))
        assert not a["padding"].any()
        inside = ((xy >= S.LO) & (xy <= S.LO + S.SPAN)).all(axis=1)
        assert (np.abs(b["particles"][inside] - xy[inside]) <= S.HALF_STEP + S.ROUNDING).all()
        assert S.parse(S.canonical(frame))["ids"].tolist() == list(range(5, n + 5))
        assert S.canonical(S.canonical(frame)) == S.canonical(frame)


def test_pack_without_a_valid_pressure_and_with_some():
    frame, _ = frame_of(9, 1, valid=False)
    assert S.parse(frame)["flags"] == 0 and (S.parse(frame)["c"] == 255).all()
    xy = np.zeros((4, 2))
    some = S.pack(0, xy, [1.0, 1.0, 1.0, 1.0], range(4), K.walls(0), True, valid_slots=[True, True, False, False])
    assert S.parse(some)["c"].tolist() == [0, 0, 255, 255]


def test_parse_refuses_what_is_no_frame():
    from sand_crate_amd import track
    frame, _ = frame_of(5, 1)
    for bad in (b"XCTK" + frame[4:], frame[:4] + struct.pack("<I", 2) + frame[8:], frame[:-1], frame + b"\0", frame[:10],
                frame[:16] + struct.pack("<q", -1) + frame[24:], frame[:24] + struct.pack("<i", 17) + frame[28:]):
        with pytest.raises(track.TrackError):
            track.parse(bad)


# ---- the file

def test_file_round_trip_and_truncation(tmp_path):
    from sand_crate_amd import track
    frames = [frame_of(n, s, tick=t)[0] for t, (n, s) in enumerate(((0, 0), (5, 1), (257, 16), (9, 0)))]
    path = tmp_path / "variant_00" / track.FILE_NAME
    with track.TrackWriter(path, particle_radius=0.005, coefficients={"dt": 0.002}) as w:
        w.write_all(frames)
        assert w.frames == 4
        with pytest.raises(track.TrackError):
            w.write(frames[1][:-8])
    data = path.read_bytes()
    assert data[:16] == b"SCTKFILE" + struct.pack("<I", 1) + bytes(4) and data[16:] == b"".join(frames)
    assert track.split(data[16:]) == frames
    for where in (path, path.parent):                                       # the file, or the directory that holds it
        with track.TrackReader(where) as r:
            assert len(r) == 4 and not r.truncated and list(r) == frames and r[2] == frames[2] and r[-1] == frames[3]
            assert r.ticks() == [0, 1, 2, 3] and r.particle_radius() == 0.005
    # cut at every offset inside the last frame: the frames before it, and the flag
    start = len(data) - len(frames[3])
    cut = tmp_path / "cut.sctk"
    for at in range(start + 1, len(data)):
        cut.write_bytes(data[:at])
        with track.TrackReader(cut) as r:
            assert r.truncated and list(r) == frames[:3], at
    cut.write_bytes(data[:start])                                           # between two frames: nothing is missing
    with track.TrackReader(cut) as r:
        assert not r.truncated and len(r) == 3 and r.particle_radius() is None
    cut.write_bytes(b"SCTKFILF" + data[8:])
    with pytest.raises(track.TrackError):
        track.TrackReader(cut)
    with pytest.raises(track.TrackError):
        track.split(data[16:-1])


# ---- the cases tell the rules apart

def fused_quantise(v):
    """The spec's rule with the product and the sum contracted into one fused multiply-add: (v - lo) is rounded, then
    (v - lo) * scale + 0.5 is rounded once (Fraction -> float rounds to nearest, ties to even)."""
    scale = Fraction(S.CODES / S.SPAN)
    out = []
    for x in np.asarray(v, dtype=np.float64):
        t = float(Fraction(float(x) - S.LO) * scale + Fraction(1, 2))
        out.append(min(max(int(np.floor(t)), 0), S.CODES))
    return np.array(out, dtype=np.uint16)


def fused_dequantise(q):
    """lo + q * step as one fused multiply-add."""
    step = Fraction(S.STEP)
    return np.array([float(Fraction(S.LO) + int(k) * step) for k in q])


def wrong_quantisers():
    scale = S.CODES / S.SPAN

    def clamp(q):
        return np.clip(q, 0, S.CODES).astype(np.uint16)

    def f32(v):
        v32 = v.astype(np.float32)
        return clamp(np.floor((v32 - np.float32(S.LO)) * np.float32(scale) + np.float32(0.5)).astype(np.float64))

    return {
        "round half to even": lambda v: clamp(np.rint((v - S.LO) * scale)),
        "truncation": lambda v: clamp(np.trunc((v - S.LO) * scale)),
        "float32": f32,
        "divide by the step": lambda v: clamp(np.floor((v - S.LO) / S.STEP + 0.5)),
        "no clamp below": lambda v: np.minimum(np.floor((v - S.LO) * scale + 0.5), S.CODES).astype(np.int64).astype(np.uint16),
        "65535 codes": lambda v: clamp(np.floor((v - S.LO) * (65535 / S.SPAN) + 0.5)),
    }


def test_coordinate_cases_tell_wrong_quantisers_from_the_spec():
    v = K.finite_coordinates()
    v = v[np.abs(v) < 1e6]                                                  # (the wrong rules need not survive 1e300)
    want = S.quantise(v)
    for name, rule in wrong_quantisers().items():
        with np.errstate(all="ignore"):
            got = rule(v)
        assert (got != want).any(), f"no case tells '{name}' from the spec"


def test_where_a_fused_multiply_add_shows():
    """The half-step cases were meant to catch a contracted (x - lo) * scale + 0.5.  They cannot, and no coordinate can:
    the fused form rounds (x - lo) * scale + 0.5 once, BEFORE the floor, and the sum of the rounded product and 0.5 is
    exact wherever the two could part -- for a product p >= 0.5 the sum lies in p's binade or the next, where p + 0.5 is
    representable or rounds without crossing an integer; for p in [0.25, 0.5), the one place where the sum is rounded to
    a coarser grid than the product's, x - lo is a multiple of 2^-55 and the products lie 2^-39.6 apart, never within
    2^-54 of 0.5.  Measured: no difference at any of the 65,534 half steps with three neighbouring doubles on each side,
    nor among 200,000 random coordinates.  So this asserts what holds -- the two forms agree on every case -- and pins
    the contraction where it does show: lo + q * step of the way back, which a fused multiply-add changes for a third
    of the codes (the GPU test compares loaded positions bit for bit with this spec)."""
    half = K.half_step_coordinates()
    assert len(half) >= 5 * 300
    assert np.array_equal(fused_quantise(half), S.quantise(half))
    q = np.arange(S.CODES + 1)
    differ = fused_dequantise(q) != S.dequantise(q)
    assert differ.sum() > 20_000


def test_pressure_cases_tell_wrong_colour_rules_from_the_spec():
    p = K.pressures()
    want = S.colour(p)
    with np.errstate(all="ignore"):
        wrong = {
            # (255 - floor(p * 255) is no wrong rule: after the clip it is the spec's function -- the two part for negative
            # products only, where both give 255 or more.  The floor that does show is the floor of the difference.)
            "floor of the difference": np.clip(np.nan_to_num(np.floor(255.0 - p * 255.0), nan=0.0), 0, 255),
            # (clipping the pressure to [0, 1] first is the spec's function too; what shows is not clipping at all, the byte
            # taken from the low bits, and clipping to a byte before the subtraction instead of after it)
            "no clip: the low byte": np.nan_to_num(255.0 - np.trunc(p * 255.0), nan=0.0, posinf=0.0, neginf=0.0) % 256.0,
            "clip the product to a byte, then subtract from 256": np.clip(
                np.nan_to_num(256.0 - np.clip(np.trunc(p * 255.0), 0, 255), nan=0.0), 0, 255),
            "round to nearest": np.clip(np.nan_to_num(255.0 - np.rint(p * 255.0), nan=0.0), 0, 255),
            "trunc of the difference": np.clip(np.nan_to_num(np.trunc(255.0 - p * 255.0), nan=0.0), 0, 255),
            "times 256": np.clip(np.nan_to_num(255.0 - np.trunc(p * 256.0), nan=0.0), 0, 255),
            "NaN is white": np.clip(np.nan_to_num(255.0 - np.trunc(p * 255.0), nan=255.0), 0, 255),
        }
    for name, got in wrong.items():
        assert (got.astype(np.uint8) != want).any(), f"no case tells '{name}' from the spec"
    k = np.arange(256) / 255.0
    assert np.array_equal(S.colour(k), 255 - np.trunc(k * 255.0).astype(np.int64))


# ---- replay, as far as it goes without a GPU

def test_replay_arguments_and_output_names(tmp_path):
    from sand_crate_amd import replay, track
    a = replay.argument_parser().parse_args(["run/variant_03"])
    assert a.path == Path("run/variant_03") and not (a.gif or a.video or a.frames or a.hud or a.plain)
    assert (a.width, a.height, a.zoom, a.center, a.every, a.out, a.radius) == (1000, 1000, 1.0, None, 1, None, None)
    a = replay.argument_parser().parse_args("t.sctk --gif --video --frames --width 640 --height 480 --zoom 2.5 --center 100.5 80 "
                                            "--hud --plain --every 3 --out o".split())
    assert (a.gif, a.video, a.frames, a.hud, a.plain) == (True,) * 5 and a.center == [100.5, 80.0] and a.out == Path("o")
    assert (a.width, a.height, a.zoom, a.every) == (640, 480, 2.5, 3)
    with pytest.raises(SystemExit):
        replay.argument_parser().parse_args(["t.sctk", "--arrows"])           # frames carry no velocities
    variant = tmp_path / "variant_00"
    with track.TrackWriter(variant / track.FILE_NAME) as w:
        w.write(frame_of(3, 0)[0])
    assert not (variant / "config.yaml").exists()                            # (nothing to say: none written)
    for where in (variant, variant / track.FILE_NAME):
        assert replay.output_paths(where, None, True, True, True) == {
            "gif": variant / "video.gif", "video": variant / "video.avi", "frames": variant / "frames.npz"}
    assert replay.output_paths(variant, tmp_path / "o", True, False, False) == {"gif": tmp_path / "o" / "video.gif"}
    assert replay.output_paths(variant, None, False, False, False) == {}
    assert replay.selected(10, 3) == [0, 3, 6, 9] and replay.selected(0, 1) == []
    with pytest.raises(ValueError):
        replay.selected(4, 0)
    with pytest.raises(ValueError):
        replay.replay(variant)                                               # nothing asked for
    with pytest.raises(track.TrackError):
        replay.replay(variant, gif=True)                                     # no radius anywhere


def test_driver_takes_track():
    from sand_crate_amd.main import argument_parser
    ap = argument_parser()
    assert ap.parse_args(["c.yaml"]).track == 0 and ap.parse_args(["c.yaml", "--track"]).track == 1
    assert ap.parse_args(["c.yaml", "--track", "10"]).track == 10
