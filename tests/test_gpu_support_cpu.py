"""What the helpers of tests/gpu_support.py accept and reject, on CPU tensors and NumPy arrays: the smallest inputs at
which a comparison could silently accept a wrong result."""
import numpy as np
import pytest
import torch

import gpu_support as U

BASE = np.array([[1.0, -2.5, 0.0], [3.0, 1e-300, 7.0]])                             # 2 x 3 float64
NAN_LOW, NAN_NEG = (np.array([bits], dtype=np.uint64).view(np.float64)[0] for bits in (0x7FF8000000000001, 0xFFF8000000000000))


def changed(at, value, base=BASE):
    a = base.copy()
    a[at] = value
    return a


def raises(compare, a, b):
    try:
        compare(a, b)
    except AssertionError:
        return True
    return False


# every comparison as (got, want) -> accepted?, its inputs made from two NumPy arrays
COMPARISONS = {
    "same_bytes": lambda a, b: not raises(U.same_bytes, a, b),
    "same_frame": lambda a, b: not raises(U.same_frame, a, b),
    "same_bits": lambda a, b: U.same_bits(torch.from_numpy(a.copy()), b),
    "same_bits_or_nan": lambda a, b: U.same_bits_or_nan(torch.from_numpy(a.copy()), b),
    "same_values_signs": lambda a, b: U.same_values_signs(torch.from_numpy(a.copy()), b),
    "same_bits_on_device": lambda a, b: U.same_bits_on_device(torch.from_numpy(a.copy()), b),
}
# NaN against NaN, as the docstrings say: (the same NaN, another payload, the other sign)
NAN_RULE = {
    "same_bytes": (True, False, False),
    "same_frame": (False, False, False),              # array_equal: a NaN is no pixel value
    "same_bits": (True, False, False),
    "same_bits_or_nan": (True, True, True),
    "same_values_signs": (True, True, False),
    "same_bits_on_device": (True, False, False),
}
each = pytest.mark.parametrize("name", sorted(COMPARISONS))


@each
def test_an_identical_pair_passes(name):
    same = COMPARISONS[name]
    assert same(BASE, BASE.copy())
    assert same(BASE.astype(np.int64), BASE.astype(np.int64))
    assert same(np.zeros((0, 3)), np.zeros((0, 3)))


@each
def test_a_dtype_mismatch_fails(name):
    same = COMPARISONS[name]
    whole = np.array([[1.0, 2.0, 0.0], [3.0, 4.0, 7.0]])
    assert same(whole, whole.copy())
    assert not same(whole, whole.astype(np.float32)) and not same(whole.astype(np.int64), whole)
    assert not same(whole.astype(np.int32), whole.astype(np.int64))
    assert not same(np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64))


@each
def test_a_shape_mismatch_fails(name):
    same = COMPARISONS[name]
    assert not same(BASE, BASE.reshape(3, 2)) and not same(BASE, BASE.reshape(-1)) and not same(BASE, BASE[:1])


@each
@pytest.mark.parametrize("at", [(0, 0), (1, 2), (1, 1)])
def test_one_ulp_in_one_element_fails(name, at):
    same = COMPARISONS[name]
    for toward in (np.inf, -np.inf):
        assert not same(changed(at, np.nextafter(BASE[at], toward)), BASE)
        assert not same(BASE, changed(at, np.nextafter(BASE[at], toward)))


@pytest.mark.parametrize("name", sorted(set(COMPARISONS) - {"same_frame"}))       # (same_frame compares pixel values)
def test_the_sign_of_zero_fails(name):
    same = COMPARISONS[name]
    assert not same(changed((0, 2), -0.0), BASE) and not same(BASE, changed((0, 2), -0.0))
    assert same(changed((0, 2), -0.0), changed((0, 2), -0.0))


@each
def test_a_nan_against_a_number_fails(name):
    same = COMPARISONS[name]
    for at in ((0, 0), (1, 2)):
        assert not same(changed(at, np.nan), BASE) and not same(BASE, changed(at, np.nan))


@each
def test_nan_against_nan_is_what_the_docstring_says(name):
    same = COMPARISONS[name]
    want = changed((1, 0), np.nan)
    assert np.signbit(NAN_NEG) and not np.signbit(NAN_LOW) and np.isnan(NAN_NEG) and np.isnan(NAN_LOW)
    got = tuple(same(changed((1, 0), nan), want) for nan in (np.nan, NAN_LOW, NAN_NEG))
    assert got == NAN_RULE[name]
    # a NaN in another place than the rule's is no NaN of the rule
    assert not same(changed((1, 1), np.nan, base=changed((1, 0), 3.0)), want)


# ---- sentinels

def test_full_chooses_the_dtype_by_the_value_unless_told():
    a, b = U.full(3, "cpu"), U.full((2, 3), "cpu", U.SENTINEL_F)
    assert a.dtype == torch.int64 and a.shape == (3,) and a.tolist() == [U.SENTINEL] * 3
    assert b.dtype == torch.float64 and b.shape == (2, 3) and (b == U.SENTINEL_F).all()
    c, d = U.full(2, "cpu", dtype=torch.int32), U.full(2, "cpu", dtype=torch.float64)
    assert c.dtype == torch.int32 and c.tolist() == [U.SENTINEL] * 2
    assert d.dtype == torch.float64 and d.tolist() == [float(U.SENTINEL)] * 2
    assert U.full(2, "cpu", U.SENTINEL_FAR).tolist() == [-12345.5] * 2 and (U.SENTINEL, U.SENTINEL_F) == (-777, -1.5)


def test_untouched_is_false_when_one_element_of_one_tensor_is_altered():
    def tensors():
        return [U.full((2, 3), "cpu"), U.full(4, "cpu", U.SENTINEL_F), U.full(2, "cpu", dtype=torch.int32)]
    assert U.untouched(*tensors()) and U.untouched()
    for k, at in ((0, (1, 2)), (0, (0, 0)), (1, 3), (2, 0)):
        t = tensors()
        t[k][at] += 1
        assert not U.untouched(*t)
        assert U.untouched(*(x for j, x in enumerate(t) if j != k))


def test_untouched_holds_floats_to_the_float_sentinel_and_integers_to_the_integer_one():
    assert not U.untouched(U.full(3, "cpu", float(U.SENTINEL)))                     # a float tensor of the integer sentinel
    assert not U.untouched(U.full(3, "cpu", -1))
    assert not U.untouched(U.full(3, "cpu", U.SENTINEL_FAR))
    # a sentinel of the caller's holds for both kinds
    both = [U.full(3, "cpu", dtype=torch.float64), U.full(3, "cpu")]
    assert U.untouched(*both, sentinel=U.SENTINEL) and not U.untouched(*both)
    both[0][1] = U.SENTINEL_F
    assert not U.untouched(*both, sentinel=U.SENTINEL)


# ---- where the first difference is

def message(compare, a, b):
    with pytest.raises(AssertionError) as err:
        compare(a, b)
    return str(err.value)


def test_same_stream_names_the_first_byte():
    data = bytes(range(40))
    U.same_stream(data, bytes(data))
    U.same_stream(b"", b"")
    other = bytearray(data)
    other[17] ^= 1
    other[30] ^= 1
    assert message(U.same_stream, bytes(other), data) == "40 bytes vs 40, first difference at byte 17"
    other = bytearray(data)
    other[0] ^= 0x80
    assert message(U.same_stream, data, bytes(other)).endswith("first difference at byte 0")
    assert message(U.same_stream, data[:33], data) == "33 bytes vs 40, first difference at byte 33"
    assert message(U.same_stream, data, data[:33]) == "40 bytes vs 33, first difference at byte 33"
    assert message(U.same_stream, b"", data).endswith("first difference at byte 0")


def test_same_frame_names_the_first_pixel():
    colour = np.arange(36, dtype=np.uint8).reshape(3, 4, 3)
    U.same_frame(colour, colour.copy())
    got = colour.copy()
    got[1, 2, 1] += 1                                                               # one channel of one pixel
    got[2, 0] += 1
    text = message(U.same_frame, got, colour)
    assert text.startswith("2 pixels differ, the first at row 1, column 2: ")
    assert str(got[1, 2]) in text and str(colour[1, 2]) in text
    grey = np.arange(12, dtype=np.uint8).reshape(3, 4)
    U.same_frame(grey, grey.copy())
    got = grey.copy()
    got[2, 3], got[0, 1] = 0, 9
    assert message(U.same_frame, got, grey) == "2 pixels differ, the first at row 0, column 1: 9 vs 1"
    got = grey.copy()
    got[2, 3] = 0
    assert message(U.same_frame, got, grey) == "1 pixels differ, the first at row 2, column 3: 0 vs 11"
    with pytest.raises(AssertionError):
        U.same_frame(grey, grey.astype(np.int16))
    with pytest.raises(AssertionError):
        U.same_frame(colour, colour[:, :, :1])


def test_same_bytes_passes_its_place_on():
    with pytest.raises(AssertionError, match="in the third frame"):
        U.same_bytes(BASE, changed((0, 1), 2.5), "in the third frame")
    with pytest.raises(AssertionError, match="in the third frame"):
        U.same_bytes(BASE, BASE[:1], "in the third frame")
    U.same_bytes(BASE.T, np.ascontiguousarray(BASE.T))                              # the layout is not compared


# ---- code_of

def test_code_of_returns_the_code_of_the_error():
    from sand_crate_amd import _native as N

    def refuse(code, message="no"):
        raise N.NativeError(code, message)
    assert U.code_of(refuse, -3) == -3 and U.code_of(refuse, 7, message="room") == 7


def test_code_of_fails_the_test_when_nothing_is_raised():
    with pytest.raises(pytest.fail.Exception):
        U.code_of(lambda *a, **kw: 0, 1, key=2)


def test_code_of_lets_another_error_through():
    def wrong():
        raise ValueError("not the library's")
    with pytest.raises(ValueError):
        U.code_of(wrong)
