"""CPU checks of the inputs built to exercise the JPEG encoder (tests/jpeg_cases.py): each has the property it is named
for, by tests/jpeg_spec.py alone; together they code every symbol of the four Huffman tables; the specification stays a
valid JPEG on them; and one-line mutations of the specification change their bytes.  No GPU: the device encoder is held
to jpeg_spec on these inputs by tests/test_gpu_jpeg_cases.py."""
import inspect
import io

import numpy as np
import pytest

import jpeg_cases as K
import jpeg_spec as J

CASES = K.cases()


def zz_of(name):
    return J.coefficients(*CASES[name])


def position(v: int, u: int) -> int:
    """The zig-zag position of the natural coefficient (v, u)."""
    return int(np.nonzero(J.ZIGZAG == 8 * v + u)[0][0])


def restart_markers(data: bytes) -> list:
    """n of every RSTn in the entropy-coded data of a file, in order."""
    ecs = np.frombuffer(data[len(J.header(8, 8, 50)):-2], dtype=np.uint8)
    ff = np.nonzero(ecs[:-1] == 0xFF)[0]
    nxt = ecs[ff + 1]
    assert set(nxt.tolist()) <= {0} | set(range(0xD0, 0xD8))
    ff = ff[(ff == 0) | (ecs[ff - 1] != 0xFF) | (nxt != 0)]  # (the 0x00 behind an 0xFF is no marker's first byte)
    return [int(n) - 0xD0 for n in ecs[ff + 1] if n != 0]


# ---- the helpers of jpeg_cases against jpeg_spec's own functions -----------------------------------

@pytest.mark.parametrize("name", ["symbols_q100", "long_65_mcus", "rounds_noise_505", "edge_15x15", "dc11_cb"])
def test_block_bits_add_up_to_the_rows_of_the_spec(name):
    """block_bits is written from the tables; its sums equal the code lengths of row_symbols, for whole rows and for
    rows cut after each MCU (the DC predictor of what remains does not change)."""
    img, q = CASES[name]
    zz = J.coefficients(img, q)
    bits = K.block_bits(img, q)
    assert bits.shape == (zz.shape[0], 3 * zz.shape[1])
    for r, row in enumerate(zz):
        assert int(J.row_symbols(row)[1].sum()) == bits[r].sum() == K.row_bits(img, q)[r]
        for m in range(1, min(len(row), 24)):
            assert int(J.row_symbols(row[:m])[1].sum()) == bits[r, :3 * m].sum()
        assert len(K.row_bytes(img, q)[r]) == (bits[r].sum() + 7) // 8
    rounds = K.round_bits(img, q)
    assert rounds.shape == (zz.shape[0], -(-bits.shape[1] // 64)) and (rounds[:, -1] == bits.sum(axis=1)).all()
    if bits.shape[1] > 64:
        assert (rounds[:, 0] == bits[:, :64].sum(axis=1)).all()


def test_symbol_set_of_a_known_block():
    """DC 0; 127 behind no zero (0x07), 16 behind two (0x25) -- and an all-zero Cb and Cr."""
    img = K.grey_block(K.FF_FF_BLOCK)
    assert J.coefficients(img, 100)[0, 0, 0, :6].tolist() == [0, 127, 0, 0, 16, 0]
    got = K.symbol_set(img, 100)
    assert got >= {(0, "dc", 0), (0, "ac", 0x07), (0, "ac", 0x25), (1, "dc", 0), (1, "eob", True)}
    assert {x for x in got if x[0] == 1} == {(1, "dc", 0), (1, "eob", True)}
    # one coefficient at position 63 behind 62 zeros: three ZRLs, run 14, no EOB
    img = K.coefficient_blocks([0], [63], [5], 50)[0]
    assert np.nonzero(J.coefficients(img, 50)[0, 0, 0])[0].tolist() == [63]
    assert {(0, "zrl", 3), (0, "ac", 0xE3), (0, "eob", False)} <= K.symbol_set(img, 50)


# ---- the families ----------------------------------------------------------------------------------

def union_of(names) -> set:
    out = set()
    for name in names:
        out |= K.symbol_set(*CASES[name])
    return out


def test_symbols_code_every_ac_symbol_of_both_tables():
    names = [n for n in CASES if n.startswith("symbols_")]
    assert names and {CASES[n][1] for n in names} <= set(K.SYMBOL_QUALITIES)
    got = union_of(names)
    for t in (0, 1):
        assert {s for tt, kind, s in got if tt == t and kind == "ac"} == K.AC_SYMBOLS  # all 160: no exception
        assert {s for tt, kind, s in got if tt == t and kind == "zrl"} == {1, 2, 3}
        assert {s for tt, kind, s in got if tt == t and kind == "eob"} == {True, False}
    assert sum(CASES[n][0].size for n in names) // 192 <= 128  # a minimal subset: at most 128 blocks of the 50,000


def test_all_cases_code_every_symbol():
    got = union_of(CASES)
    for t in (0, 1):
        assert {s for tt, kind, s in got if tt == t and kind == "ac"} == K.AC_SYMBOLS
        assert {s for tt, kind, s in got if tt == t and kind == "dc"} == set(range(12))
        assert {s for tt, kind, s in got if tt == t and kind == "zrl"} == {1, 2, 3}
        assert {s for tt, kind, s in got if tt == t and kind == "eob"} == {True, False}


@pytest.mark.parametrize("comp,kind", enumerate(K.EXTREME_COLOURS))
def test_extremes_sit_on_the_edge_of_size_10(comp, kind):
    zz = zz_of(f"extreme_{kind}")
    assert zz.shape == (1, 6, 3, 64)
    for k, (v, u) in enumerate(K.EXTREME_BASES):
        assert zz[0, k, comp, position(v, u)] == 1020 and zz[0, k + 3, comp, position(v, u)] == -1020
    assert np.abs(zz[..., 1:]).max() == 1020
    table = min(comp, 1)
    assert (table, "dc", 11) in K.symbol_set(*CASES[f"dc11_{kind}"])
    dc = zz_of(f"dc11_{kind}")[0, :, comp, 0]
    assert sorted(set(dc.tolist())) == [-1024, 1016]


def test_dc_ladder_codes_the_middle_categories():
    got = K.symbol_set(*CASES["dc_ladder"])
    for t in (0, 1):
        assert {s for tt, kind, s in got if tt == t and kind == "dc"} >= {0, 4, 5, 6, 7, 8, 9, 10}


def test_long_rows_hold_the_longest_blocks():
    longest_block = longest_round = 0
    for name in ("long_65_mcus", "long_129_mcus"):
        img, q = CASES[name]
        assert q == 100 and set(np.unique(img).tolist()) == {0, 255} and img.shape[1] >= 64 * 8
        bits = K.block_bits(img, q)
        assert bits.mean() > 780  # (uniform noise: about 700)
        rounds = K.round_bits(img, q)
        per_round = np.diff(np.c_[np.zeros(len(rounds), dtype=np.int64), rounds], axis=1)
        longest_block = max(longest_block, int(bits.max()))
        longest_round = max(longest_round, int(per_round.max()))
        assert rounds.shape[1] >= 4
    assert (longest_block, longest_round) == (K.LONGEST_BLOCK, K.LONGEST_ROUND)  # what the module's docstring records
    assert longest_block <= K.BLOCK_BITS_BOUND and longest_round <= 64 * K.BLOCK_BITS_BOUND
    uniform = K.block_bits(K.noise(1, 24, 520), 100)
    assert uniform.mean() < bits.mean() - 50


@pytest.mark.parametrize("m", K.ROUND_MCUS)
def test_grey_rows_have_their_bits_in_closed_form(m):
    img, q = CASES[f"rounds_grey_{m}"]
    assert img.shape == (16, 8 * m, 3) and not zz_of(f"rounds_grey_{m}").any()
    bits = K.block_bits(img, q)
    assert (bits == np.tile([6, 4, 4], m)).all() and (K.row_bits(img, q) == K.grey_row_bits(m)).all()
    after = lambda blocks: 14 * (blocks // 3) + (0, 6, 10)[blocks % 3]  # noqa: E731
    ends = [*range(64, 3 * m, 64), 3 * m]
    assert K.round_bits(img, q).tolist() == [[after(b) for b in ends]] * 2
    for row in K.row_bytes(img, q):
        assert len(row) == -(-14 * m // 8)


def test_grey_rows_sit_on_the_edges_of_the_rounds():
    ends = {m: K.round_bits(*CASES[f"rounds_grey_{m}"])[0].tolist() for m in K.ROUND_MCUS}
    assert len(ends[21]) == 1 and 3 * 21 == 63  # one round, one block short
    assert ends[22] == [300, 308] and 300 >> 5 == 308 >> 5  # the second round: two blocks, 8 bits, no word completed
    assert [len(ends[m]) for m in (42, 43, 64, 65)] == [2, 3, 3, 4]  # 126, 129, 192 and 195 blocks
    assert 3 * 64 == 192 and ends[64][-1] == 896
    assert ends[65][2] == 896 == 28 * 32 and ends[65][3] == 910  # the third round ends a word, a fourth follows
    assert ends[16] == [224] and 224 == 7 * 32  # the row ends a word: nothing is left for the tail
    assert ends[4] == [56] and 56 % 8 == 0 and 56 % 32 != 0  # 7 bytes, no padding, a partial word


@pytest.mark.parametrize("m", K.ROUND_MCUS)
def test_noise_rows_carry_the_dc_prediction_across_rounds(m):
    for w in (8 * m, 8 * m - 7):
        img, q = CASES[f"rounds_noise_{w}"]
        assert img.shape == (9, w, 3) and q == 75
        zz, _, diff, _ = K._coded(img, q)
        assert zz.shape == (2, 3 * m, 64)
        for first in range(64, 3 * m, 64):  # the blocks that open a round: their predictor is in the round before
            blocks = slice(first, min(first + 3, 3 * m))
            assert (diff[0, blocks] != 0).all() and (zz[0, blocks, 0] != diff[0, blocks]).all()
        assert K.round_noise(w) is img


@pytest.mark.parametrize("pad", range(8))
def test_pads(pad):
    img, q = CASES[f"pad_{pad}"]
    assert img.shape[0] == 8 and img.shape[1] // 8 in range(1, 7) and q == 100
    bits = int(K.row_bits(img, q)[0])
    assert -bits % 8 == pad
    last = int(K.row_bytes(img, q)[0][-1])
    assert last & ((1 << pad) - 1) == (1 << pad) - 1  # 1-bits


def test_pads_come_from_every_width():
    assert {CASES[f"pad_{pad}"][0].shape[1] // 8 for pad in range(8)} == {1, 2, 3, 4, 5, 6}


def first_row(name) -> np.ndarray:
    img, q = CASES[name]
    rows = K.row_bytes(img, q)
    assert len(rows) == 2 and rows[0].tobytes() == rows[1].tobytes()  # the same row twice: a marker follows the first
    return rows[0]


def test_stuffing_row_lengths():
    lengths = {n: len(first_row(f"stuff_len_{n}")) for n in (255, 256, 257, 258, 512)}
    assert all(n == got for n, got in lengths.items())
    assert {n % 4 for n in lengths} == {0, 1, 2, 3} and 512 % 256 == 0


def test_stuffing_ff_positions():
    row = first_row("stuff_last_ff")
    assert row[-1] == 0xFF
    data = J.encode(*CASES["stuff_last_ff"])
    assert data.count(b"\xff\x00\xff\xd0") == 1 and data.endswith(b"\xff\x00\xff\xd9")
    at = np.nonzero(first_row("stuff_ff_at_every_mod_4") == 0xFF)[0]
    assert set((at & 3).tolist()) == {0, 1, 2, 3}
    for k in (255, 256):
        row = first_row(f"stuff_ff_at_{k}")
        assert row[k] == 0xFF and len(row) > 257


def test_stuffing_ff_runs():
    """Two and three 0xFF bytes in a row, across the words that the lanes of k_jpeg_stuff take."""
    row = first_row("stuff_ff_ff").tobytes()
    assert row.hex().startswith("2800" "f8" "ffff" "13") and b"\xff\xff\xff" not in row  # an all-zero MCU, a DC of 0
    assert row.index(b"\xff\xff") == 3  # bytes 3 and 4: two words
    assert b"\xff\x00\xff\x00\x13" in J.encode(*CASES["stuff_ff_ff"])
    row = first_row("stuff_ff_ff_ff").tobytes()
    assert row.index(b"\xff\xff\xff") == 7 and b"\xff\xff\xff\xff" not in row  # bytes 7, 8 and 9: two words
    assert b"\xff\x00\xff\x00\xff\x00" in J.encode(*CASES["stuff_ff_ff_ff"])


@pytest.mark.parametrize("h", K.ROW_HEIGHTS)
def test_rows_count_their_restart_intervals(h):
    img, q = CASES[f"rows_{h}"]
    assert img.shape == (h, 8, 3) and q == 50
    rows = -(-h // 8)
    assert rows in (64, 65, 128, 129) and len(K.row_bytes(img, q)) == rows
    assert restart_markers(J.encode(img, q)) == [k % 8 for k in range(rows - 1)]


def test_edges_and_tails():
    assert {(h % 8, w % 8) for h, w in K.EDGE_SIZES} == {(i, j) for i in range(8) for j in range(8)}
    for h, w in K.EDGE_SIZES:
        assert CASES[f"edge_{h}x{w}"][0].shape == (h, w, 3) and 8 <= h < 16 and 8 <= w < 16
    for k, (h, w) in K.TAIL_SIZES.items():
        assert CASES[f"tail_{k}"][0].shape == (h, w, 3) and K.blocks_of(h, w) % 32 == k


def test_strips():
    (h0, w0), (h1, w1) = K.STRIP_SIZES
    assert (w0, h1) == (16384, 16384)  # kRenderMaxSide, the largest side sc_jpeg_bound accepts
    assert K.blocks_of(h0, w0) == 2 * 6144 and 6144 == 96 * 64 and -(-h1 // 8) == 2048
    for h, w in K.STRIP_SIZES:
        assert CASES[f"strip_{h}x{w}"][0].shape == (h, w, 3)


def test_no_case_is_large():
    assert max(img.nbytes for img, _ in CASES.values()) <= 1 << 19
    assert sum(img.nbytes for img, _ in CASES.values()) < 3 << 20


# ---- the bound the buffers rest on -----------------------------------------------------------------

def test_quantised_ac_coefficients_stay_below_1024():
    """sc_jpeg.h sizes its LDS window and row buffers by "the quantised AC coefficients stay below 1024 in magnitude".
    The largest response of each of the 63 AC basis functions is that of its sign pattern: 1020 at most, at
    quality 100 (every Q is 1; any other quality divides further)."""
    assert (J.quant_tables(100) == 1).all()
    peak = np.zeros(64, dtype=np.int64)
    for v in range(8):
        for u in range(8):
            pattern = np.where(K.sign_pattern(v, u), 127, -128)
            s = np.stack([pattern, -1 - pattern])  # both polarities
            q = J.quantise(J.dct(np.broadcast_to(s[None, :, None], (1, 2, 3, 8, 8))), 100).reshape(2, 3, 64)
            assert np.abs(q[..., 1:]).max() <= 1023
            peak[8 * v + u] = np.abs(q[..., 8 * v + u]).max()
    assert peak[1:].max() == 1020 and peak[1:].min() >= 512  # every position reaches size 10, none size 11
    assert np.nonzero(peak[1:] == 1020)[0].tolist() == [3, 31, 35]  # (0, 4), (4, 0) and (4, 4)


def test_no_block_exceeds_the_bound():
    for name, (img, q) in CASES.items():
        assert K.max_ac(img, q) <= 1023, name
        assert K.block_bits(img, q).max() <= K.BLOCK_BITS_BOUND, name
    assert K.BLOCK_BITS_BOUND == 22 + 63 * 26 == 1660


# ---- validity --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(CASES))
def test_the_spec_decodes(name):
    pytest.importorskip("PIL")
    from PIL import Image
    from test_jpeg_cpu import psnr
    img, q = CASES[name]
    out = np.asarray(Image.open(io.BytesIO(J.encode(img, q))).convert("RGB"))
    assert out.shape == img.shape
    if q == 100:
        assert psnr(out, img) > 45


# ---- discrimination --------------------------------------------------------------------------------

def rewritten(name: str, old: str, new: str):
    """The function `name` of jpeg_spec with one piece of its source replaced."""
    src = inspect.getsource(getattr(J, name))
    assert src.count(old) == 1
    scope = {}
    exec(compile(src.replace(old, new), f"<mutated {name}>", "exec"), vars(J), scope)
    return scope[name]


def altered_code(table: int, symbol: int):
    tables = [(code.copy(), length.copy()) for code, length in J.AC_TABLES]
    tables[table][0][symbol] ^= 1
    return tables


def coding(symbol) -> list:
    """The `symbols` cases that code the symbol."""
    names = [n for n in sorted(CASES) if n.startswith("symbols_") and symbol in K.symbol_set(*CASES[n])]
    assert names
    return names


# name -> (attribute of jpeg_spec, its replacement, cases whose files must change).  The comments say what the images of
# tests/test_gpu_jpeg.py (noise at quality 75 at its nine sizes and at quality 100 at its two, the flat colours and the
# black / white blocks at qualities 1 and 100, the smooth and the noisy ramp at its twelve qualities: 46 images,
# rebuilt on the CPU) do under the same mutation.
MUTATIONS = {
    # the old images: none of the 46 changes
    "a size-10 code": ("AC_TABLES", lambda: altered_code(0, 0xBA), coding((0, "ac", 0xBA))),
    # the old images: none of the 46 changes
    "a run-15 code": ("AC_TABLES", lambda: altered_code(1, 0xF7), coding((1, "ac", 0xF7))),
    # the old images: the flat colours and the black / white blocks at quality 100 change, through DC differences of
    # categories 10 and 11; no AC coefficient of theirs has size 10.  extreme_grey changes through its AC value of 1020
    "extra bits masked to 9": ("_extra", lambda: (lambda v, size, f=J._extra: f(v, size) & 0x1FF), ["extreme_grey"]),
    # the old images: 18 change (the ramps at qualities up to 75)
    "the third ZRL dropped": ("row_symbols", lambda: rewritten("row_symbols", "nz = run >> 4",
                                                               "nz = np.minimum(run >> 4, 2)"),
                              coding((0, "zrl", 3)) + coding((1, "zrl", 3))),
    # the old images: 43 change
    "padding with 0-bits": ("pack_bits", lambda: rewritten("pack_bits", "bits = np.ones(", "bits = np.zeros("),
                            [f"pad_{pad}" for pad in range(1, 8)]),
    # the old images: 7 change (rows that happen to end in 0xFF among the thousands of the large frames)
    "no 0x00 behind a row's last 0xFF": ("stuff", lambda: rewritten("stuff", "ff = data == 0xFF\n",
                                                                     "ff = data == 0xFF\n    ff[-1:] = False\n"),
                                         ["stuff_last_ff"]),
    # the old images: one changes (the smooth ramp at quality 90 holds a pair); none of the noise does
    "no 0x00 behind the second 0xFF of a pair": ("stuff", lambda: rewritten(
        "stuff", "ff = data == 0xFF\n", "ff = data == 0xFF\n    ff[1:] &= ~(data[:-1] == 0xFF)\n"),
        ["stuff_ff_ff", "stuff_ff_ff_ff"]),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_mutations_of_the_spec_change_the_cases(monkeypatch, mutation):
    attribute, make, names = MUTATIONS[mutation]
    want = {name: J.encode(*CASES[name]) for name in names + ["rounds_grey_16"]}
    monkeypatch.setattr(J, attribute, make())
    for name in names:
        assert J.encode(*CASES[name]) != want[name], name
    assert J.encode(*CASES["rounds_grey_16"]) == want["rounds_grey_16"]  # (all-zero blocks in whole words: untouched)
    monkeypatch.undo()
    assert all(J.encode(*CASES[name]) == data for name, data in want.items())
