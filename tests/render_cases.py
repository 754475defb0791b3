"""Frames that sit on the edges of the raster rule (tests/test_render_cases_cpu.py, tests/test_gpu_render_cases.py).

The renderer (csrc/sc_render.h; render_prepare / render_launch in csrc/sc_host_frames.h) decides a pixel by a handful of
comparisons, each of which a scene reaches only by luck:
  kRenderWaveRadius = 4   a thread per disc up to R = 4, a wave per disc beyond (`radii`: R = 0 .. 6, and R = 4 | 5 at one
                          particle_radius through the zoom);
  the clip test           X + R >= 0, X - R <= W - 1 in float64, both axes (`clip`: a centre R - 1, R and R + 1 pixels
                          outside each edge and corner; `far`: coordinates whose product with W - 1 is huge, infinite
                          or NaN);
  trunc, then floor       cx = trunc(x (W - 1)), column floor((cx - center) zoom + W / 2) (`negative`: x < 0, where trunc
                          is not floor; `view`: screen coordinates that are negative and fractional before the floor);
  ex^2 + ey^2 <= R^2      every frame with a disc;
  4 e <= w^2              `wall_ties`: walls whose neighbouring rows are an exact tie; `wall_shapes`: len2 == 0, ends far
                          outside, SC_MAX_SEGMENTS walls, and the host's box lox .. hiy around each;
  the key buffer          zeroed when it grows, then only by the resolve of the frame just drawn (`frame_sizes`: frames
                          of different sizes in an order on ONE context);
  np = min(ns, nt)        which slots have a pressure (`pressures`: every slot after a tick, with overlapping discs of
                          different colours; `appended`: particles appended behind ticked ones).

With W = 64, H = 48, zoom 1 and the default centre the column of x is trunc(63 x): `col(k)` = (k + 0.5) / 63 lies in
column k for every k, and `radius(k)` = (k + 0.5) / 64 gives R = k; `negative` uses W - 1 = 64 and H - 1 = 32, so that
its products are exact.  Every builder asserts such premises itself; what a case claims about its frame is in `claims`
and is checked against tests/render_spec.py on the CPU.

`sc_upload_state` takes any float64: `far` includes +inf, -inf and NaN.  (sc_download_state leaves out slots whose x is
not finite, so the specification never sees those; a NaN or infinite y with a finite x it does see, and skips.)

Everything here is NumPy, tests/render_spec.py and, for `pressures`, the oracle: no device, no reference.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import render_spec as S

W, H = 64, 48
MAX_SEGMENTS = 16       # include/sandcrate_hip.h: SC_MAX_SEGMENTS
WAVE_RADIUS = 4         # csrc/sc_render.h: kRenderWaveRadius
NO_WALLS = np.zeros((0, 2, 2))


@dataclass
class Case:
    """One frame: the particles to upload (ids 0 .. P - 1, no pressure), the walls, the view, and what it claims."""
    name: str
    xy: np.ndarray
    segments: np.ndarray = field(default_factory=lambda: NO_WALLS)
    width: int = W
    height: int = H
    particle_radius: float = 0.0
    zoom: float = 1.0
    center: tuple | None = None
    segment_width: int = 2
    claims: dict = field(default_factory=dict)
    pressure: np.ndarray | None = None   # per particle, for the cases that are ticked (None: all zero)
    ticked: int = 0                      # the particles the last tick left live: the slots that have a pressure

    @property
    def view(self) -> dict:
        return dict(zoom=self.zoom, center=self.center, segment_width=self.segment_width)

    @property
    def R(self) -> int:
        return S.disc_radius(self.width, self.particle_radius, self.zoom)

    def screen(self):
        """(X, Y) of every particle before the floor."""
        cx, cy = (self.width / 2, self.height / 2) if self.center is None else self.center
        with np.errstate(invalid="ignore", over="ignore"):
            return (S.screen(self.xy[:, 0], self.width, cx, self.zoom), S.screen(self.xy[:, 1], self.height, cy, self.zoom))

    def spec(self, xy=None, pressure=None, ids=None):
        """tests/render_spec.py's frame of the case as it is uploaded (or of the given state)."""
        xy = self.xy if xy is None else xy
        if pressure is None:
            pressure = np.zeros(len(xy)) if self.pressure is None or len(self.pressure) != len(xy) else self.pressure
        ids = np.arange(len(xy)) if ids is None else ids
        with np.errstate(over="ignore"):  # (a wall's len2 may overflow: wall_shapes_1e300)
            return S.render(xy, pressure, ids, self.segments, self.width, self.height, self.particle_radius, **self.view)

    def walls(self, segments=None):
        """H x W bool: the pixels the case's walls (or these) cover."""
        with np.errstate(over="ignore"):
            return S.wall_mask(self.segments if segments is None else segments, self.width, self.height, self.zoom,
                               self.center, self.segment_width)


# ---------------------------------------------------------------- binary-friendly constructions
def col(k, side=W):
    """A world coordinate whose trunc(x (side - 1)) is k, half a pixel from either neighbour (k < 0: trunc rounds up)."""
    k = np.asarray(k, dtype=np.float64)
    x = np.where(k >= 0, k + 0.5, k - 0.5) / (side - 1)
    assert np.array_equal(np.trunc(x * (side - 1)), k)
    return x


def row(k):
    return col(k, H)


def radius(k, side=W):
    """A particle_radius with trunc(side * r) = k."""
    r = (k + 0.5) / side
    assert np.trunc(side * r) == k
    return r


def disc_count(R, X, Y, width=W, height=H):
    """Pixels of the disc of radius R around the pixel (X, Y) that lie in the frame, counted one by one."""
    return sum(1 for j in range(max(Y - R, 0), min(Y + R, height - 1) + 1) for i in range(max(X - R, 0), min(X + R, width - 1) + 1)
               if (i - X) ** 2 + (j - Y) ** 2 <= R * R)


def lit(img) -> int:
    return int(img.any(axis=2).sum())


def scattered(n, seed, lo=0.04, hi=0.96):
    return np.random.RandomState(seed).rand(n, 2) * (hi - lo) + lo


BOX = np.array([[[0.0, 0.0], [1.0, 0.0]], [[1.0, 0.0], [1.0, 1.0]], [[1.0, 1.0], [0.0, 1.0]], [[0.0, 1.0], [0.0, 0.0]]])


# ---------------------------------------------------------------- radii
def radii():
    """The same 40 particles at R = 0 .. 6 through particle_radius, and at R = 4 | 5 through the zoom alone."""
    xy = scattered(40, 40)
    out = []
    for k in range(7):
        c = Case(f"radii_R{k}", xy, particle_radius=radius(k), claims={"R": k, "wave": k > WAVE_RADIUS})
        out.append(c)
    for zoom, k in ((1.2, 4), (1.25, 5)):
        out.append(Case(f"radii_zoom{zoom}", xy, particle_radius=radius(4), zoom=zoom, claims={"R": k, "wave": k > WAVE_RADIUS}))
    for c in out:
        assert c.R == c.claims["R"]
    return out


# ---------------------------------------------------------------- clip
def clip():
    """At R = 3 and R = 6: disc centres R - 1, R and R + 1 pixels outside each of the four edges, and outside each corner
    in both axes at once.  claims["lit"]: the pixels each particle lights alone; the discs are disjoint, so the frame
    lights their sum.  A centre R outside an edge lights exactly one pixel, one R + 1 outside lights none."""
    out = []
    for R in (3, 6):
        X, Y, want = [], [], []
        step = 2 * R + 2
        for n, t in enumerate((R - 1, R, R + 1)):
            along_x, along_y = 8 + n * step, 6 + n * step   # where the three sit along their edge
            for x, y in ((-t, along_y), (W - 1 + t, along_y), (along_x, -t), (along_x, H - 1 + t),
                         (-t, -t), (W - 1 + t, -t), (-t, H - 1 + t), (W - 1 + t, H - 1 + t)):
                X.append(x)
                Y.append(y)
                want.append(disc_count(R, x, y))
        X, Y = np.array(X), np.array(Y)
        xy = np.column_stack((col(X), row(Y)))
        edge = np.tile(np.arange(8) < 4, 3)
        dist = np.repeat([R - 1, R, R + 1], 8)
        want = np.array(want)
        assert (want[edge & (dist == R)] == 1).all() and (want[dist == R + 1] == 0).all()
        assert (want[edge & (dist == R - 1)] == {3: 6, 6: 8}[R]).all()  # columns R - 1 and R of the disc: 5 + 1, 7 + 1
        assert (want[~edge & (dist == R)] == 0).all()  # a corner at (R, R): inside the clip test, outside the circle
        c = Case(f"clip_R{R}", xy, particle_radius=radius(R), claims={"R": R, "lit": want, "X": X, "Y": Y})
        assert c.R == R
        out.append(c)
    return out


# ---------------------------------------------------------------- negative
def negative():
    """x (W - 1) in {-0.5, -1, -1.5, -2.5}, exactly (W - 1 = 64): columns 0, -1, -1, -2 by trunc, where a floor gives
    -1, -1, -2, -3.  The same in y (H - 1 = 32).  R = 1: a disc centred on column 0 lights four pixels, one on column -1
    one, one further out none."""
    w, h = 65, 33
    t = np.array([-0.5, -1.0, -1.5, -2.5])
    rows_, cols_ = np.array([5, 11, 17, 23]), np.array([8, 20, 32, 44])
    xy = np.vstack((np.column_stack((t / 64, (rows_ + 0.5) / 32)), np.column_stack(((cols_ + 0.5) / 64, t / 32))))
    assert np.array_equal(xy[:4, 0] * 64, t) and np.array_equal(xy[4:, 1] * 32, t)
    c = Case("negative", xy, width=w, height=h, particle_radius=radius(1, w),
             claims={"R": 1, "columns": [0, -1, -1, -2], "floored": [-1, -1, -2, -3], "lit": [4, 1, 1, 0] * 2})
    X, Y = c.screen()
    assert c.R == 1
    assert np.floor(X[:4]).tolist() == c.claims["columns"] and np.floor(Y[4:]).tolist() == c.claims["columns"]
    assert np.floor(xy[:4, 0] * 64).tolist() == c.claims["floored"]
    return [c]


# ---------------------------------------------------------------- far
FAR = (1e6, -1e6, 1e18, -1e18, 1e300, -1e300, 1.7e308, np.inf, -np.inf, np.nan)


def far():
    """Ten ordinary particles and, among them, one per value of FAR in x and one in y: 63 * 1.7e308 overflows.  Only
    the ordinary ones are drawn (claims["ordinary"])."""
    plain = scattered(10, 12)
    other = scattered(2 * len(FAR), 13)[:, 0]
    odd = np.vstack([(v, other[2 * k]) for k, v in enumerate(FAR)] + [(other[2 * k + 1], v) for k, v in enumerate(FAR)])
    xy = np.empty((len(plain) + len(odd), 2))
    where = np.zeros(len(xy), dtype=bool)
    where[1::3][:len(plain)] = True   # the ordinary ones sit between the others
    xy[where], xy[~where] = plain, odd
    with np.errstate(over="ignore"):
        assert np.isinf(1.7e308 * (W - 1))
    return [Case("far", xy, segments=BOX, particle_radius=radius(2), claims={"R": 2, "ordinary": np.flatnonzero(where)})]


# ---------------------------------------------------------------- view
def view():
    """Zoom 1.5 and 0.5 about centres with fractional parts, over particles that also lie outside the unit square, so
    that screen coordinates come out negative and fractional before the floor (claims["negative_fractional"]: how many
    of them have a disc that reaches the frame); and a zoom at which R = 0 although trunc(W r) = 2."""
    rs = np.random.RandomState(77)
    xy = rs.rand(400, 2) * 3.0 - 1.0
    out = [Case("view_zoom1.5", xy, segments=BOX, particle_radius=radius(2), zoom=1.5, center=(40.25, 10.75), segment_width=3,
                claims={"R": 3}),
           Case("view_zoom0.5", xy, segments=BOX, particle_radius=radius(4), zoom=0.5, center=(-3.5, 60.0), segment_width=1,
                claims={"R": 2}),
           Case("view_zoom0.4", xy, segments=BOX, particle_radius=radius(2), zoom=0.4, center=(30.0, 20.5), claims={"R": 0})]
    for c in out:
        assert c.R == c.claims["R"]
        X, Y = c.screen()
        R = c.R
        seen = (np.floor(X) + R >= 0) & (np.floor(X) - R <= W - 1) & (np.floor(Y) + R >= 0) & (np.floor(Y) - R <= H - 1)
        frac = ((X < 0) & (X != np.floor(X)) | (Y < 0) & (Y != np.floor(Y))) & seen
        c.claims["negative_fractional"] = int(frac.sum())
    assert out[0].claims["negative_fractional"] >= 3 and out[1].claims["negative_fractional"] >= 3
    return out


# ---------------------------------------------------------------- wall_ties
def _axis_walls():
    """A horizontal wall along row 11, columns 6 .. 26, and a vertical one along column 45, rows 8 .. 40 (zoom 1)."""
    return np.array([[[col(6), row(11)], [col(26), row(11)]], [[col(45), row(8)], [col(45), row(40)]]])


def wall_ties():
    """Axis-aligned walls on integer screen coordinates: row 11 + k is covered iff 4 k^2 <= w^2 -- k = 0 for w = 0, 1;
    |k| <= 1 for w = 2 (the tie) and 3; |k| <= 2 for w = 5.  At zoom 0.5 about (32, 24) the same walls lie on
    half-integers (row 17.5, column 38.5): the rows at distance 1/2, 3/2, 5/2 are ties at w = 1, 3, 5, and w = 0 covers
    nothing.  claims["rows"]: the rows covered in column `at_col` of the horizontal wall; claims["cols"]: the columns
    covered in row `at_row` of the vertical one.  Then a 45-degree wall and a steep wall at zoom 4."""
    seg = _axis_walls()
    out = []
    reach = {0: 0, 1: 0, 2: 1, 3: 1, 5: 2}
    for w, k in reach.items():
        out.append(Case(f"wall_ties_w{w}", np.zeros((0, 2)), segments=seg, segment_width=w,
                        claims={"at_col": 16, "rows": list(range(11 - k, 11 + k + 1)), "at_row": 24,
                                "cols": list(range(45 - k, 45 + k + 1))}))
    half = {0: [], 1: [17, 18], 2: [17, 18], 3: [16, 17, 18, 19], 5: [15, 16, 17, 18, 19, 20]}
    for w, rows_ in half.items():
        c = Case(f"wall_ties_half_w{w}", np.zeros((0, 2)), segments=seg, zoom=0.5, segment_width=w,
                 claims={"at_col": 24, "rows": rows_, "at_row": 22, "cols": [r + 21 for r in rows_]})
        assert S.screen(seg[0, 0, 1], H, H / 2, 0.5) == 17.5 and S.screen(seg[1, 0, 0], W, W / 2, 0.5) == 38.5
        out.append(c)
    # 45 degrees through integer pixels: (i, i +- 1) is at squared distance 1/2, 4 e = 2 <= 4; (i, i +- 2) at 2
    diag = np.array([[[col(10), row(10)], [col(30), row(30)]]])
    out.append(Case("wall_ties_diagonal", np.zeros((0, 2)), segments=diag, segment_width=2,
                    claims={"covered": [(20, 20), (20, 21), (21, 20)], "bare": [(20, 22), (22, 20)]}))
    # steep, at zoom 4: from (24, -52) to (32, 88) on the screen, both ends outside
    steep = np.array([[[col(30), row(5)], [col(32), row(40)]]])
    c = Case("wall_ties_steep", np.zeros((0, 2)), segments=steep, zoom=4.0, segment_width=3, claims={"every_row": True})
    assert S.screen(steep[0, :, 1], H, H / 2, 4.0).tolist() == [-52.0, 88.0]
    out.append(c)
    return out


# ---------------------------------------------------------------- wall_shapes
def wall_shapes():
    """A zero-length segment (len2 == 0: a blob of diameter w -- 21 pixels at w = 5 on a pixel centre), a segment that
    crosses the frame with both ends outside, one wholly outside, one whose far end is at 1e300 (len2 overflows, t = 0
    for every pixel: the blob of its near end), SC_MAX_SEGMENTS at once, and none -- each over the same 30 particles."""
    xy = scattered(30, 30)
    r = radius(2)
    a = [col(20), row(20)]
    fan = np.array([[[0.5, 0.5], [0.5 + 0.7 * np.cos(k * np.pi / 8), 0.5 + 0.7 * np.sin(k * np.pi / 8)]] for k in range(MAX_SEGMENTS)])
    out = [Case("wall_shapes_point", xy, segments=np.array([[a, a]]), particle_radius=r, segment_width=5,
                claims={"wall_pixels": 21}),
           Case("wall_shapes_crossing", xy, segments=np.array([[[-0.5, 0.2], [1.5, 0.7]]]), particle_radius=r, segment_width=2,
                claims={"every_column": True}),
           Case("wall_shapes_outside", xy, segments=np.array([[[1.2, 0.1], [1.8, 0.9]], [[0.2, -0.3], [0.9, -0.6]]]),
                particle_radius=r, segment_width=5, claims={"wall_pixels": 0}),
           Case("wall_shapes_1e300", xy, segments=np.array([[a, [1e300, row(20)]]]), particle_radius=r, segment_width=5,
                claims={"wall_pixels": 21}),
           Case("wall_shapes_sixteen", xy, segments=fan, particle_radius=r, segment_width=2, claims={"segments": MAX_SEGMENTS}),
           Case("wall_shapes_none", xy, particle_radius=r, claims={"wall_pixels": 0})]
    assert len(fan) == MAX_SEGMENTS
    return out


# ---------------------------------------------------------------- frame_sizes
def frame_sizes():
    """An ORDERED list of frames of one state for ONE context (run it forwards, and backwards on a second context): a key
    that a resolve left behind, or a buffer sized by the wrong frame, shows in the next one.  The sixth frame looks at an
    empty region and must be black."""
    xy = scattered(300, 300)
    out = [Case("frame_64x48_R6", xy, segments=BOX, particle_radius=radius(6), claims={"R": 6}),
           Case("frame_5x3", xy, segments=BOX, width=5, height=3, particle_radius=0.3, claims={"R": 1}),
           Case("frame_1x1", xy, width=1, height=1, particle_radius=0.3, claims={"R": 0}),
           Case("frame_7x2", xy, segments=BOX, width=7, height=2, particle_radius=0.3, segment_width=0, claims={"R": 2}),
           Case("frame_13x1", xy, width=13, height=1, particle_radius=0.3, claims={"R": 3}),
           Case("frame_64x48_empty", xy, segments=BOX, particle_radius=radius(6), zoom=4.0, center=(300.0, 300.0),
                claims={"R": 24, "black": True}),
           Case("frame_48x64", xy, segments=BOX, width=48, height=64, particle_radius=radius(3, 48), claims={"R": 3})]
    for c in out:
        assert c.R == c.claims["R"]
    return out


# ---------------------------------------------------------------- pressures, appended
PRESSURE_N = 3000
PRESSURE_R = radius(1, 128)     # R = 1 in a frame of 128 pixels; the diameter is 3 / 128
PRESSURE_COEF = dict(dt=0.0005, particle_radius=PRESSURE_R, wall_collision_decay=0.3, pressure_amplifier=30.0,
                     ignored_pressure=0.3, collider_noise_level=0.0, viscosity=4.0, surface_smoothing=80.0,
                     target_pressure=-1.0, gravity=[0.0, 9.8], max_particles=100000)
PRESSURE_BODIES = [{"fixed": {"name": "box", "segments": BOX.tolist()}}]
APPENDED_N = 200


def pressure_blob():
    """(positions, velocities) of the blob about (0.42, 0.58), cut off at 0.33 from its centre, which leaves the corner
    beyond x = 0.8, y = 0.2 empty: a Gaussian heap, dense in the middle, over a thin uniform disc in which a particle has
    one or two others within a diameter -- many have none."""
    rs = np.random.RandomState(3000)
    n_thin = 400
    rad, phi = 0.33 * np.sqrt(rs.rand(n_thin)), 2 * np.pi * rs.rand(n_thin)
    p = np.column_stack((rad * np.cos(phi), rad * np.sin(phi)))
    while len(p) < PRESSURE_N:
        q = rs.randn(PRESSURE_N, 2) * 0.06
        p = np.vstack((p, q[(q * q).sum(1) < 0.33 ** 2]))[:PRESSURE_N]
    p = p[rs.permutation(PRESSURE_N)]
    return p + np.array([0.42, 0.58]), (rs.rand(PRESSURE_N, 2) - 0.5) * 0.1


def appended_particles():
    rs = np.random.RandomState(200)
    return np.column_stack((0.84 + rs.rand(APPENDED_N) * 0.12, 0.04 + rs.rand(APPENDED_N) * 0.12)), np.zeros((APPENDED_N, 2))


def pressure_premises(xy, pressure, ids, case):
    """What `pressures` needs of a state -- the oracle's here, the device's own in the GPU test: no particle lost,
    pressures of 0, strictly between 0 and 1 and of 1 and above (at least 50 of each), where the colour byte is clipped to
    0; and at least 50 pixels under two or more discs whose colour bytes differ."""
    assert len(xy) == PRESSURE_N and np.isfinite(xy).all() and np.array_equal(ids, np.arange(PRESSURE_N))
    assert (pressure == 0).sum() >= 50 and ((pressure > 0) & (pressure < 1)).sum() >= 50 and (pressure >= 1).sum() >= 50
    c = S.colour(pressure)
    assert (c[pressure >= 1] == 0).all() and (c[pressure == 0] == 255).all()
    # per pixel the smallest and the largest colour byte of the discs over it: two particle_keys runs, ordered by colour
    order = np.argsort(c, kind="stable")
    rank = np.empty(len(c), dtype=np.int64)
    rank[order] = np.arange(len(c))
    kw = dict(zoom=case.zoom, center=case.center)
    hi = S.particle_keys(xy, pressure, rank, case.width, case.height, case.particle_radius, **kw) & np.uint64(0xFF)
    lo = S.particle_keys(xy, pressure, len(c) - 1 - rank, case.width, case.height, case.particle_radius, **kw) & np.uint64(0xFF)
    mixed = int((hi != lo).sum())
    assert mixed >= 50, mixed
    return mixed


@functools.lru_cache(maxsize=None)
def oracle_tick():
    """The blob after one tick of the oracle: (positions, velocities, pressure)."""
    from oracle.scene import OracleCrate
    from oracle.world import World
    orc = OracleCrate(World(PRESSURE_BODIES, [], dict(PRESSURE_COEF)))
    orc.particles, orc.particle_velocities = pressure_blob()
    orc.physics_tick()
    out = orc.particles, orc.particle_velocities, orc.particles_pressure
    for a in out:
        a.setflags(write=False)
    return out


def pressures():
    """The blob, ticked once, in a frame of 128 x 128 with R = 1: discs of every colour overlap, so "the highest id wins"
    decides hundreds of pixels (claims["mixed"])."""
    xy, _, pr = oracle_tick()
    c = Case("pressures", xy, segments=BOX, width=128, height=128, particle_radius=PRESSURE_R, claims={"R": 1}, pressure=pr,
             ticked=PRESSURE_N)
    assert c.R == 1
    c.claims["mixed"] = pressure_premises(xy, pr, np.arange(len(xy)), c)
    return [c]


def appended_premises(xy, pressure, ids, case):
    """`appended` needs: the appended particles are the last APPENDED_N ids, have no pressure, lie in the corner, and no
    ticked disc reaches a pixel of theirs; and the ticked ones still have pressures of every kind."""
    n = PRESSURE_N
    assert len(xy) == n + APPENDED_N and np.array_equal(ids, np.arange(n + APPENDED_N))
    assert (pressure[n:] == 0).all() and (pressure[:n] > 0).sum() >= 200
    kw = dict(zoom=case.zoom, center=case.center)
    old = S.particle_keys(xy[:n], pressure[:n], ids[:n], case.width, case.height, case.particle_radius, **kw) != 0
    new = S.particle_keys(xy[n:], pressure[n:], ids[n:], case.width, case.height, case.particle_radius, **kw) != 0
    assert new.sum() >= APPENDED_N and not (old & new).any()
    return old, new


def appended():
    """The ticked blob plus APPENDED_N particles appended in the empty corner, rendered before another tick: the new
    slots are white, the ticked ones keep their colours (np = min(ns, nt) = PRESSURE_N)."""
    xy, _, pr = oracle_tick()
    new, _ = appended_particles()
    c = Case("appended", np.vstack((xy, new)), width=128, height=128, particle_radius=PRESSURE_R, claims={"R": 1},
             pressure=np.concatenate((pr, np.zeros(APPENDED_N))), ticked=PRESSURE_N)
    appended_premises(c.xy, c.pressure, np.arange(len(c.xy)), c)
    return [c]


# ---------------------------------------------------------------- all of them
GROUPS = {"radii": radii, "clip": clip, "negative": negative, "far": far, "view": view, "wall_ties": wall_ties,
          "wall_shapes": wall_shapes, "frame_sizes": frame_sizes, "pressures": pressures, "appended": appended}
UPLOADED = ("radii", "clip", "negative", "far", "view", "wall_ties", "wall_shapes")  # one upload, one frame, no tick


@functools.lru_cache(maxsize=None)
def group(name):
    cases = tuple(GROUPS[name]())
    for c in cases:
        assert c.width <= 128 and c.height <= 128 and len(c.xy) <= 5000 and c.R <= 24
        c.xy.setflags(write=False)
    return cases
