"""What the GPU tests share: the `sc` and `crate` fixtures, the scenes, tensors in and out, `code_of` and the
comparisons.  A test file takes the fixtures by name (`from gpu_support import sc  # noqa: F401`) and the rest through
`import gpu_support as U`.  torch and the package are imported inside the functions, so collecting the suite needs
neither a GPU nor the built library.

The comparisons say in their names how strict they are.  The ones that raise name the first difference; the ones
between a tensor and a NumPy array return a bool, for use inside an `assert`:

    same_bytes           host arrays: shape, dtype and every byte
    same_stream          encoder output: every byte
    same_frame           images: shape, dtype and every pixel
    same_bits            tensor against array: dtype, shape and every byte (so -0.0 is not 0.0, and a NaN is its bits)
    same_bits_or_nan     as same_bits, but where the rule has a NaN any NaN will do
    same_values_signs    equal values, NaN equal to NaN, and equal sign bits everywhere (also of a NaN)
    same_bits_on_device  same_bits, compared by torch on the device"""
import copy
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
SENTINEL = -777          # what integer outputs hold before a call
SENTINEL_F = -1.5        # ... and float outputs
SENTINEL_FAR = -12345.5  # the float sentinel of the pair list and the state exchange


# ---- fixtures

@pytest.fixture(scope="module")
def sc():
    import torch
    torch.cuda.init()  # torch's HIP runtime must come up before the library's in a process that uses both
    import sand_crate_amd
    return sand_crate_amd


@pytest.fixture(scope="module")
def crate(sc):
    """One small crate whose engine searches the callers' points."""
    return sc.Crate(scene(sc), noise="none", capacity=256)


# ---- scenes

def scene(sc, name="wave_machine"):
    return sc.load_config(ROOT / "config" / f"{name}.yaml").world_config


def spread_world(sc, n, least=1):
    """wave_machine with discs sized for max(n, least) particles and no sources."""
    wc = copy.deepcopy(scene(sc))
    d = float(np.sqrt(12.0 / (np.pi * max(n, least))))
    wc.coefficients.update(particle_radius=d / 2, dt=0.002 * (d / 0.01), max_particles=max(n, 1))
    wc.particle_sources = []
    return wc


def m2_world(sc, n, xy=None):
    """bench.py's M2 inputs: n uniform particles (or those at `xy`, which then costs no draw) in the wave_machine world,
    spacing scaled to n, no sources -> (world, positions, velocities)."""
    rs = np.random.RandomState(1234)
    p = rs.rand(n, 2) * 0.96 + 0.02 if xy is None else xy
    return spread_world(sc, n), p, (rs.rand(n, 2) - 0.5) * 0.1


def m2_crate(sc, n, xy=None, **kw):
    wc, p, v = m2_world(sc, n, xy)
    crate = sc.Crate(wc, noise="counter", noise_seed=1, capacity=n + 1024, **kw)
    crate.particles = p
    crate.particle_velocities = v
    return crate


def small_screen_config(tmp_path, width=160, height=120) -> Path:
    import yaml
    with open(ROOT / "config" / "wave_machine.yaml") as f:
        cfg = yaml.safe_load(f)
    cfg["playback"].update(screen_x=width, screen_y=height)
    path = tmp_path / "small_screen.yaml"
    with open(path, "w") as f:
        yaml.safe_dump(cfg, f)
    return path


# ---- tensors in and out

def tensor(a, width=2, requires_grad=False):
    """A CUDA float64 copy of `a` in rows of `width` (None: in its own shape), synchronised; None gives None."""
    import torch
    if a is None:
        return None
    a = np.array(a, dtype=np.float64)                                               # (a copy: the cases are read-only)
    t = torch.from_numpy(a if width is None else a.reshape(-1, width)).cuda()
    torch.cuda.synchronize()
    return t.requires_grad_() if requires_grad else t


def full(shape, device, value=SENTINEL, dtype=None):
    """A tensor filled with `value`; without a dtype, int64 for an int and float64 for a float."""
    import torch
    if dtype is None:
        dtype = torch.int64 if isinstance(value, int) else torch.float64
    return torch.full(shape if isinstance(shape, tuple) else (shape,), value, dtype=dtype, device=device)


def untouched(*tensors, sentinel=None):
    """Every element still holds its sentinel: SENTINEL_F in a float tensor and SENTINEL in an integer one, or `sentinel`
    in both."""
    def expected(t):
        return sentinel if sentinel is not None else SENTINEL_F if t.dtype.is_floating_point else SENTINEL
    return all(bool((t == expected(t)).all()) for t in tensors)


def code_of(call, *args, **kw):
    """The code of the NativeError that the call must raise."""
    from sand_crate_amd import _native as N
    with pytest.raises(N.NativeError) as err:
        call(*args, **kw)
    return err.value.code


# ---- comparisons that raise

def same_bytes(a, b, where=""):
    """Host arrays: the same shape, dtype and bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, where
    assert a.tobytes() == b.tobytes(), where


def same_stream(got: bytes, want: bytes):
    """Encoder output: the same bytes; names the first that differs."""
    if got != want:
        n = min(len(got), len(want))
        first = next((k for k in range(n) if got[k] != want[k]), n)
        raise AssertionError(f"{len(got)} bytes vs {len(want)}, first difference at byte {first}")


def same_frame(got, want):
    """Images, rows x columns (x channels): the same shape, dtype and pixels; counts the others and names the first."""
    assert got.shape == want.shape and got.dtype == want.dtype
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1)) if got.ndim == 3 else np.argwhere(got != want)
        raise AssertionError(f"{len(bad)} pixels differ, the first at row {bad[0][0]}, column {bad[0][1]}: "
                             f"{got[tuple(bad[0])]} vs {want[tuple(bad[0])]}")


def spec_frame(crate, width, height, **kw):
    """render_spec's frame of what the engine downloads and the walls as they stand."""
    import render_spec
    xy, _, pressure, ids = crate.engine.download()
    seg = crate.segments if crate.rigid_bodies else np.zeros((0, 2, 2))
    return render_spec.render(xy, pressure, ids, seg, width, height, crate.particle_radius, **kw)


# ---- comparisons of a tensor with the rule's NumPy array -> bool

def same_bits(got, want):
    """The same dtype, shape and bytes."""
    g = got.cpu().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and g.tobytes() == want.tobytes()


def same_bits_or_nan(got, want):
    """The same dtype and shape; NaN exactly where the rule has NaN, whichever NaN; every other element bit for bit."""
    g = got.detach().cpu().numpy()
    if g.dtype != want.dtype or g.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool((np.isnan(g) == nan).all()) and g[~nan].tobytes() == want[~nan].tobytes()


def same_values_signs(got, want):
    """The same dtype and shape; equal values, NaN equal to NaN; equal sign bits everywhere, also of a NaN."""
    g = got.cpu().numpy()
    return g.dtype == want.dtype and g.shape == want.shape and np.array_equal(g, want, equal_nan=True) and \
        np.array_equal(np.signbit(g), np.signbit(want))


def same_bits_on_device(got, want):
    """The same dtype and shape and torch.equal on the array's device copy, floats as their 64 bits."""
    import torch
    want = torch.from_numpy(np.ascontiguousarray(want)).to(got.device)
    got = got.detach()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == torch.float64:
        got, want = got.contiguous().view(torch.int64), want.view(torch.int64)
    return torch.equal(got, want)
