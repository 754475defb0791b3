"""The device's NumPy stream at the borders of its 624-word blocks: the cases tests/test_gpu_rng_blocks.py runs, and
a word-level model of the block loop that says what each of them meets (tests/test_rng_block_cases_cpu.py proves it).

Three kernels of csrc/sc_rng.h draw from the MT19937 state the device holds: `k_rng_noise` and `k_rng_noise_small`
through `rng_noise_block` -- the tick's rand(P, 2), P = sum C_i --, and `k_rng_emit` through `RngSerial`.  What they
have to get right sits at the ends of a state block:
  regeneration  a block of 624 words is made from the previous one in three dependent phases of 227 words;
  the carry     from an odd position a double's first word is word 623 and its second word 0 of the next block;
  the empty     a loop round that starts at 623 draws no whole double at all;
  stretch
  the end       a draw that ends at 624 leaves 624 and regenerates nothing; the next one regenerates before it draws;
  write-back    the key goes back to memory -- after a refill only, in `k_rng_emit`.
An odd position is a legal state (`sc_rng_set_state` takes 0..624): one 32-bit integer drawn from np.random before the
stream is handed over leaves one, and `rand` and `binomial` consume words in pairs, so it stays odd from then on.

`block_walk` restates `rng_noise_block` word for word and records the events it meets; its `fault` argument makes the
wrong generators the cases have to tell from the right one.  The worlds are isolated touching pairs on a lattice four
diameters apart -- every pair member has C = 1, so k pairs consume rand(2k, 2), 8k words, whatever the noise does to
them -- and lone particles, C = 0.

Everything here is NumPy and the oracle: no device, no reference."""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace
from pathlib import Path

import numpy as np

import rng_cases as rc

ROOT = Path(__file__).resolve().parent.parent

N, M = 624, 397          # sc_rng.h kMtN, kMtM
SPAN = N - M             # 227: the words of a regeneration phase
SMALL_IDS = 1 << 16      # sc_rng.h kSmallIds: the host's id bound up to which k_rng_noise_small takes the tick's noise
SMALL_BLOCK = 256        # sc_rng.h kSmallBlock: its workgroup; thread t scans ids [t per, (t + 1) per), per = ceil(ids / 256)
_UPPER, _LOWER, _A = np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)


def key_of(seed: int) -> np.ndarray:
    return np.random.RandomState(seed).get_state()[1].copy()


KEY = key_of(624)        # the state block every case starts from


# ------------------------------------------------------------------ the block loop, word for word
def temper(y: np.ndarray) -> np.ndarray:
    y = np.array(y, dtype=np.uint32)
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def twist(cur, succ, far):
    y = (cur & _UPPER) | (succ & _LOWER)
    return far ^ (y >> np.uint32(1)) ^ np.where(y & np.uint32(1), _A, np.uint32(0))


def to_double(a, b):
    """NumPy's random_sample: (a >> 5, b >> 6) -> (a 2^26 + b) / 2^53."""
    return ((a >> np.uint32(5)).astype(np.float64) * 67108864.0 + (b >> np.uint32(6)).astype(np.float64)) / 9007199254740992.0


FAULTS = ("drop_carry", "swap_straddle", "stale_phase2")
# drop_carry     word 623 is not carried: the double that straddles the border is drawn from words 0 and 1 instead
# swap_straddle  the straddling double takes its two words in the wrong order
# stale_phase2   the third phase of a regeneration reads word kk - 227 of the OLD block (a phase that did not wait for
#                the one before it, or the wrong half of the double buffer)


def regenerate(cur: np.ndarray, fault: str | None = None) -> np.ndarray:
    """The next state block as `rng_noise_block` makes it: word kk from words kk and kk + 1 of the current block and
    word kk + 397 -- of the current block up to kk = 226, of the new one beyond --, in the phases [0, 227), [227, 454),
    [454, 624), each a word per thread; word 623 takes the NEW word 0 as its successor."""
    nxt = np.zeros(N, dtype=np.uint32)
    for phase in range(3):
        kk = np.arange(phase * SPAN, min((phase + 1) * SPAN, N))
        succ = np.where(kk + 1 < N, cur[(kk + 1) % N], nxt[0])
        made = cur if fault == "stale_phase2" and phase == 2 else nxt
        far = np.where(kk + M < N, cur[(kk + M) % N], made[(kk + M) % N])
        nxt[kk] = twist(cur[kk], succ, far)
    return nxt


@dataclass(frozen=True)
class Walk:
    doubles: np.ndarray      # (rows, 2)
    key: np.ndarray          # the state block the walk leaves
    pos: int                 # ... and the position in it: the end position
    regenerations: int
    carry_taken: int         # times word 623 was set aside as a double's first word
    carry_used: int          # times a double was finished with word 0 of the next block
    empty_stretch: int       # rounds that drew no whole double although doubles were left (they start at 623)
    trace: tuple             # the events in order: "regenerate", "carry_used", "draw <doubles>", "carry_taken"


def block_walk(pos: int, rows: int, key=None, fault: str | None = None) -> Walk:
    """`rng_noise_block` for rand(rows, 2) from (key, pos), restated: the round structure is the kernel's -- regenerate
    when the block is used up, finish a carried double, draw the whole doubles the block still holds, set word 623
    aside when one word is left and doubles are wanted."""
    assert 0 <= pos <= N and rows >= 0 and fault in (None,) + FAULTS
    cur = np.array(KEY if key is None else key, dtype=np.uint32)
    need = 2 * rows
    out = np.empty(need)
    w = regenerations = taken = used = empty = 0
    carry = None
    trace = []
    while w < need:
        if pos >= N:
            cur = regenerate(cur, fault)
            pos = 0
            regenerations += 1
            trace.append("regenerate")
        start = pos
        if carry is not None:
            second = temper(cur[start:start + 1])
            a, b = (second, carry) if fault == "swap_straddle" else (carry, second)
            out[w] = to_double(a, b)[0]
            w += 1
            start += 1
            carry = None
            used += 1
            trace.append("carry_used")
        left = need - w
        nd = min((N - start) // 2, left)
        t = temper(cur[start:start + 2 * nd])
        out[w:w + nd] = to_double(t[0::2], t[1::2])
        trace.append(f"draw {nd}")
        empty += nd == 0 and left > 0
        w += nd
        start += 2 * nd
        if w < need and start == N - 1:
            if fault != "drop_carry":
                carry = temper(cur[N - 1:N])
            start = N
            taken += 1
            trace.append("carry_taken")
        pos = start
    return Walk(out.reshape(rows, 2), cur, pos, regenerations, taken, used, int(empty), tuple(trace))


def numpy_state(pos: int, key=None) -> np.random.RandomState:
    rs = np.random.RandomState()
    rs.set_state(("MT19937", np.array(KEY if key is None else key, dtype=np.uint32), int(pos)))
    return rs


def numpy_walk(pos: int, rows: int, key=None):
    """-> (rand(rows, 2), key, position) of NumPy's own generator from (key, pos)."""
    rs = numpy_state(pos, key)
    doubles = rs.rand(rows, 2)
    _, after, at, _, _ = rs.get_state()
    return doubles, after, int(at)


# ------------------------------------------------------------------ worlds
D = 0.01                 # the diameter: config/wave_machine.yaml's own, so wave_world(sc, D, 0.1) keeps its dt of 0.002
PITCH = 4 * D            # lattice sites 0.1 + 0.04 i: x up to 0.7 -- clear of the motored wall, which leans in to
COLS, LINES = 16, 21     # x ~ 0.8 -- and y up to 0.9; the box's walls are at 0 and 1
TOUCH = 0.9              # a pair's distance in diameters: inside `norm <= d` by far more than the arithmetic's error
NOISE_LEVEL = 0.1


@dataclass(frozen=True)
class World:
    """Particles in id order (what `download` returns and the oracle computes on: the noise is drawn in id order),
    their ids ascending, and the order they are stored in on upload."""
    name: str
    p: np.ndarray
    v: np.ndarray
    ids: np.ndarray          # int64, ascending
    order: np.ndarray        # storage slot -> index into p, v, ids
    pairs: int

    @property
    def rows(self) -> int:
        return 2 * self.pairs

    def stored(self):
        """The arguments of `Engine.upload_with_ids`."""
        return self.p[self.order], self.v[self.order], self.ids[self.order]

    def with_top_id(self, top: int) -> "World":
        """The same world with its largest id moved up to `top`: the id order, and with it the drawing order, stays."""
        assert top > self.ids[-1]
        ids = self.ids.copy()
        ids[-1] = top
        return replace(self, name=f"{self.name}_top{top}", ids=ids)


def host_id_bound(ids) -> int:
    """What the host takes for the bound of the ids after `upload_with_ids` (sandcrate_hip.hip: put_from_device): a
    reset zeroes `next_id`, ids with the largest `max_id` raise it to max(next_id, max_id + 1 - n), and the n particles
    are added: max(max_id + 1, n) -- one more than the largest id, for distinct ids.  `k_rng_noise_small` scans that many
    ids while the bound is at most SMALL_IDS; beyond, the id count, the two-level scan and `k_rng_noise` take over."""
    ids = np.asarray(ids)
    return max(int(ids.max()) + 1, len(ids)) if len(ids) else 0


@functools.lru_cache(maxsize=None)
def pair_world(pairs: int, singles: int = 5, seed: int = 0) -> World:
    """`pairs` touching pairs, each alone on a lattice site and turned by its own angle (so its two particles share a
    strip or sit in consecutive ones), and `singles` lone particles on further sites.  Ids 0..n-1 are dealt at random,
    a pair's two ids are not neighbours, and the storage order is another shuffle."""
    n_sites = pairs + singles
    assert n_sites <= COLS * LINES
    rs = np.random.RandomState(7000 + 17 * pairs + singles + 1000 * seed)
    site = rs.permutation(COLS * LINES)[:n_sites]
    centre = np.stack((0.1 + PITCH * (site % COLS), 0.1 + PITCH * (site // COLS)), axis=1)
    angle = rs.rand(pairs) * np.pi
    half = 0.5 * TOUCH * D * np.stack((np.cos(angle), np.sin(angle)), axis=1)
    points = np.vstack((centre[:pairs] - half, centre[:pairs] + half, centre[pairs:]))
    n = len(points)
    p = points[rs.permutation(n)]
    v = (rs.rand(n, 2) - 0.5) * 0.1
    return World(f"pairs{pairs}_singles{singles}", p, v, np.arange(n, dtype=np.int64), rs.permutation(n), pairs)


def lone_world(m: int = 37) -> World:
    """`m` particles, each alone on its site: P = 0 in a world that is not empty."""
    return pair_world(0, singles=m)


# ------------------------------------------------------------------ the named noise cases
@dataclass(frozen=True)
class NoiseCase:
    name: str
    family: str              # quiet, ends, begins, blocks, second_tick
    start: int               # the position the stream is handed over at
    rows: int                # P of the (first) tick
    ticks: int = 1


def _noise_cases():
    out = [NoiseCase(f"quiet_s{s}", "quiet", s, 0) for s in (0, 1, 623, 624)]
    out += [NoiseCase(f"ends_at_{(s + 4 * rows - 1) % N + 1}_s{s}_P{rows}", "ends", s, rows)
            for s, rows in ((8, 154), (616, 2), (0, 156), (7, 154), (615, 2), (623, 156))]
    out += [NoiseCase(f"begins_s{s}_P{rows}", "begins", s, rows) for s in (624, 623, 622, 621) for rows in (2, 156)]
    out += [NoiseCase(f"blocks_s{s}_P480", "blocks", s, 480) for s in (1, 312, 623)]
    out += [NoiseCase("second_tick_s1_P160", "second_tick", 1, 160, ticks=2)]
    return tuple(out)


NOISE_CASES = _noise_cases()
ORACLE_CASES = tuple(c for c in NOISE_CASES if c.family in ("ends", "begins"))  # the ones also run against the oracle


def world_of(case: NoiseCase) -> World:
    return lone_world() if case.rows == 0 else pair_world(case.rows // 2)


# ------------------------------------------------------------------ id bounds of the small kernel
ID_BOUNDS = (2, 255, 256, 257, 511, 513, 65535, 65536)  # per = 1, 1, 1, 2, 2, 3, 256, 256
ID_BOUND_START = 621     # one double, a carry, a regeneration: the scan's offsets feed a block loop that is not idle
ID_BOUND_PAIRS, ID_BOUND_SINGLES = 20, 7
ID_BOUND_ORACLE = 513


def scan_run(bound: int) -> int:
    """`per` of k_rng_noise_small: the ids each of its 256 threads scans."""
    return (bound + SMALL_BLOCK - 1) // SMALL_BLOCK


@functools.lru_cache(maxsize=None)
def id_bound_world(bound: int) -> World:
    """A pair world whose ids make the host's bound exactly `bound`: sparse below it, the ends of the first thread's
    run and the start of the second's among them (ids 0, per - 1, per), the largest bound - 1; storage order shuffled,
    so id order is not slot order.  (A bound of 2 leaves room for one pair, ids 0 and 1, stored as 1, 0.)"""
    if bound == 2:
        w = pair_world(1, singles=0)
        return replace(w, name="id_bound_2", order=np.array([1, 0]))
    w = pair_world(ID_BOUND_PAIRS, ID_BOUND_SINGLES, seed=bound)
    n = len(w.p)
    per = scan_run(bound)
    forced = sorted({0, per - 1, per, bound - 1})
    rs = np.random.RandomState(bound)
    rest = np.setdiff1d(np.arange(bound - 1), forced)
    ids = np.sort(np.concatenate((forced, rs.choice(rest, n - len(forced), replace=False)))).astype(np.int64)
    return replace(w, name=f"id_bound_{bound}", ids=ids)


# ------------------------------------------------------------------ emission
EMIT_DT = 0.002
EMIT_CALLS = 3           # calls per case: the later ones start where the earlier ones stopped
EMIT_ROOM = 1000         # the store is emptied before a call that might pass this many particles
EMIT_MAX_PARTICLES = 10 ** 9
EMIT_STARTS = (0, 1, 2, 620, 621, 622, 623, 624)
LAUNCH_SOURCES = 8       # sc_rng.h kMaxSources: sc_emit_particles launches k_rng_emit once per eight sources


def _src(flow, k=0):
    return rc.source(flow, radius=0.07 + 0.01 * k, position=(0.3 + 0.02 * k, 0.6), velocity=(1.5, -0.25 * (k + 1)), noise=0.2)


EMIT_LISTS = {
    "flow_1": [_src(1)],                                        # one double a call, almost always nothing emitted
    "inversion_500": [_src(500)],
    "btpe_20000": [_src(20000)],
    "mixed_9": rc.mixed_sources(9),                             # two launches
    # eight doubles, then a second launch: from 608 it starts at 624, from 607 inside the double that straddles
    "eight_quiet_then_btpe": [_src(1, k) for k in range(8)] + [_src(20000, 8)],
}
EMIT_CASES = tuple((name, s) for name in ("flow_1", "inversion_500", "btpe_20000", "mixed_9") for s in EMIT_STARTS) + \
    (("eight_quiet_then_btpe", 608), ("eight_quiet_then_btpe", 607))


def call_bound(sources, dt: float = EMIT_DT) -> int:
    """The most particles one call can emit: every source's restart bound (oracle/rng.py: binomial_setup)."""
    return int(sum(min(s.flow, s.flow * dt + 10 * np.sqrt(s.flow * dt * (1 - dt) + 1)) for s in sources))


def emission_trace(name: str, start: int):
    """The case on NumPy's generator, launch by launch: -> [dict(call, launch, flows, start, end, refilled, emitted)],
    `refilled` saying whether the launch regenerated the state block (its key changed)."""
    sources = EMIT_LISTS[name]
    rs = numpy_state(start)
    stored, out = 0, []
    for call in range(EMIT_CALLS):
        if stored + call_bound(sources) > EMIT_ROOM:
            stored = 0
        for g in range(0, len(sources), LAUNCH_SOURCES):
            group = sources[g:g + LAUNCH_SOURCES]
            _, key0, pos0, _, _ = rs.get_state()
            spec = rc.numpy_emit(rs, group, EMIT_DT, stored, EMIT_MAX_PARTICLES)
            _, key1, pos1, _, _ = rs.get_state()
            emitted = sum(0 if p is None else len(p) for _, p, _ in spec)
            stored += emitted
            out.append(dict(call=call, launch=g // LAUNCH_SOURCES, flows=[s.flow for s in group], start=int(pos0),
                            end=int(pos1), refilled=not np.array_equal(key0, key1), emitted=emitted))
    return out


# ------------------------------------------------------------------ the oracle's side of a tick
def oracle_stage():
    """The oracle's crate for the worlds above: config/wave_machine.yaml with test_gpu_parity.wave_world's edits --
    the diameter D (its own), dt scaled with it, collider_noise_level 0.1, no sources."""
    from oracle.scene import OracleCrate
    from oracle.world import World as OracleWorld, load_scene
    world = load_scene(ROOT / "config" / "wave_machine.yaml").world
    coef = dict(world.coefficients)
    coef.update(particle_radius=D / 2, dt=0.002 * (D / 0.01), collider_noise_level=NOISE_LEVEL)
    return OracleCrate(OracleWorld(world.rigid_bodies, [], coef))


def oracle_tick(stage, p, v, block):
    """One tick of `stage` on (p, v) in id order: the walls move, then `tick_core` with `block` as the tick's
    rand(P, 2) -- which must have as many rows as the oracle counts neighbour slots --, or with what `block(P)` draws."""
    from oracle.tick import tick_core
    for b in stage.rigid_bodies:
        b.advance(stage.coef["dt"])

    def eta(total):
        assert total == len(block), (total, len(block))
        return block
    return tick_core(p, v, stage.segments, stage.body_states(), stage.coef, eta_u01=block if callable(block) else eta)
