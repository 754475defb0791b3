"""GPU tests of the JPEG encoder (k_jpeg_dct, k_jpeg_rows, k_jpeg_scan, k_jpeg_stuff; sc_jpeg_encode_device,
sc_jpeg_bound) on the inputs of tests/jpeg_cases.py, each built to sit on one edge of the kernels' codes, rounds and rows
(tests/test_jpeg_cases_cpu.py proves that it does): every file equals tests/jpeg_spec.py byte for byte, fits the bound,
has the length a capacity query reports, and comes out the same when the workspace has held another frame before."""
import ctypes

import numpy as np
import pytest

import gpu_support as U
import jpeg_cases as K
import jpeg_spec as J

pytestmark = pytest.mark.gpu

CASES = K.cases()


@pytest.fixture(scope="module")
def engine():
    import sand_crate_amd
    eng = sand_crate_amd.Engine(capacity=1024)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def want():
    """The specification's file of every case, computed once."""
    return {name: J.encode(img, q) for name, (img, q) in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case(engine, want, name):
    import torch
    from sand_crate_amd import _native as N
    img, q = CASES[name]
    h, w = img.shape[:2]
    U.same_stream(engine.encode_jpeg(np.array(img), q), want[name])
    dev = torch.from_numpy(np.array(img)).cuda()
    U.same_stream(engine.encode_jpeg(dev, q), want[name])
    U.same_stream(engine.encode_jpeg(dev, q), want[name])  # the same device tensor again
    bound, n = ctypes.c_int64(0), ctypes.c_int64(-1)
    assert engine._lib.sc_jpeg_bound(w, h, ctypes.byref(bound)) == 0 and bound.value >= len(want[name])
    torch.cuda.synchronize()
    rc = engine._lib.sc_jpeg_encode_device(engine._ctx, N._P(dev.data_ptr()), w, h, q, None, 0, ctypes.byref(n))
    assert rc == N.ERR_CAPACITY and n.value == len(want[name])  # a capacity query


@pytest.mark.parametrize("first,second", [("long_129_mcus", "rounds_grey_22"), ("rounds_grey_22", "long_129_mcus"),
                                          ("long_65_mcus", "rounds_grey_65"), ("strip_9x16384", "stuff_ff_ff_ff")])
def test_the_window_and_workspace_are_reused(engine, want, first, second):
    """A frame of long codes and one of all-zero blocks in turn on one engine: what the first leaves in the LDS window,
    the rows' bit buffers and the output buffer is not the second's."""
    for name in (first, second, first):
        img, q = CASES[name]
        U.same_stream(engine.encode_jpeg(np.array(img), q), want[name])
