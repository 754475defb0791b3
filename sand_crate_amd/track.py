"""Recordings as packed frames: the format of `Crate.capture_frame` / `Crate.tracked` (sc_track_*, csrc/sc_track.h) on
the host, the ``track.sctk`` file, and a player that turns frames back into pictures.

A frame (format 1, little-endian) is a 64-byte header -- ``b"SCTK"``, u32 version, i64 tick, i64 n, i32 n_segments,
i32 flags (bit 0: the pressure was valid), f64 lo, f64 span --, the walls of its tick as n_segments x 4 float64, and four
planes, each zero-padded to a multiple of 8 bytes: u32 id, u16 qx, u16 qy, u8 colour.  Nine bytes per particle; a
position comes back within half a step of the 65534 across [-0.25, 1.25], 1.14445e-5.  tests/track_spec.py is the rule.

``track.sctk``: 16 bytes -- ``b"SCTKFILE"``, u32 version = 1, zeros -- then frames back to back; every frame's own header
gives its length.  Importing this module needs no GPU; `Player` does.
"""
from __future__ import annotations

import struct
from pathlib import Path

import numpy as np
import yaml

MAGIC = b"SCTK"
VERSION = 1
HEADER = 64
LO, SPAN = -0.25, 1.5
CODES = 65534
NOT_FINITE = 65535
FILE_MAGIC = b"SCTKFILE"
FILE_VERSION = 1
FILE_HEADER = 16
FILE_NAME = "track.sctk"
MAX_SEGMENTS = 16
PLAIN_COLOUR = 100  # the reference's PLAYBACK_PARTICLE_COLOR is (100, 100, 255)
_HEADER = struct.Struct("<4sIqqiidd")


class TrackError(ValueError):
    pass


def _pad8(b: int) -> int:
    return (int(b) + 7) & ~7


def _planes(n: int, n_segments: int):
    o_id = HEADER + 32 * int(n_segments)
    o_qx = o_id + _pad8(4 * n)
    o_qy = o_qx + _pad8(2 * n)
    o_c = o_qy + _pad8(2 * n)
    return o_id, o_qx, o_qy, o_c, o_c + _pad8(n)


def frame_bytes(n: int, n_segments: int) -> int:
    """The size of a frame of `n` particles and `n_segments` walls (sc_track_bound)."""
    if n < 0 or not 0 <= n_segments <= MAX_SEGMENTS:
        raise TrackError(f"no frame has {n} particles and {n_segments} segments")
    return _planes(n, n_segments)[4]


def frame_length(head) -> int:
    """The length of the frame whose first 64 bytes are `head`; TrackError if they are no frame header."""
    if len(head) < HEADER:
        raise TrackError("a frame header has 64 bytes")
    magic, version, _tick, n, nseg, _flags, _lo, _span = _HEADER.unpack_from(head, 0)
    if magic != MAGIC:
        raise TrackError(f"not a track frame: magic {magic!r}")
    if version != VERSION:
        raise TrackError(f"track frame of version {version}; this reads {VERSION}")
    return frame_bytes(n, nseg)


def dequantise(q) -> np.ndarray:
    q = np.asarray(q, dtype=np.uint16)
    return np.where(q == NOT_FINITE, np.inf, LO + q.astype(np.float64) * (SPAN / CODES))


def parse(frame) -> dict:
    """-> {tick, n, flags, pressure_valid, segments (S x 2 x 2), ids (n,) int64, particles (n x 2) dequantised float64,
    colour (n,) uint8, pressure (n,) what the colour byte stands for} of one frame, records in the frame's order."""
    frame = bytes(frame)
    if frame_length(frame) != len(frame):
        raise TrackError(f"{len(frame)} bytes; the header announces {frame_length(frame)}")
    _, _, tick, n, nseg, flags, lo, span = _HEADER.unpack_from(frame, 0)
    o_id, o_qx, o_qy, o_c, _ = _planes(n, nseg)
    buf = np.frombuffer(frame, dtype=np.uint8)
    qx = buf[o_qx:o_qx + 2 * n].view("<u2")
    qy = buf[o_qy:o_qy + 2 * n].view("<u2")
    step = span / CODES
    xy = np.stack([np.where(qx == NOT_FINITE, np.inf, lo + qx.astype(np.float64) * step),
                   np.where(qy == NOT_FINITE, np.inf, lo + qy.astype(np.float64) * step)], axis=1)
    c = buf[o_c:o_c + n].copy()
    return dict(tick=tick, n=n, flags=flags, pressure_valid=bool(flags & 1),
                segments=buf[HEADER:o_id].view("<f8").reshape(nseg, 2, 2).copy(),
                ids=buf[o_id:o_id + 4 * n].view("<u4").astype(np.int64), particles=xy, colour=c,
                pressure=(255.0 - c.astype(np.float64) + 0.5) / 255.0)


def split(blob) -> list[bytes]:
    """Frames standing back to back (what sc_track_read delivers) as a list."""
    blob = bytes(blob)
    frames, at = [], 0
    while at < len(blob):
        size = frame_length(blob[at:at + HEADER])
        if at + size > len(blob):
            raise TrackError("the last frame is cut off")
        frames.append(blob[at:at + size])
        at += size
    return frames


def resolve_path(path) -> Path:
    """`path` itself when it is a file, else the track.sctk of that (variant) directory."""
    path = Path(path)
    return path / FILE_NAME if path.is_dir() else path


class TrackWriter:
    """Streams frames into a track file: nothing is kept in memory.  `config` (a plain dict, e.g. the driver's
    deep_dictify(config)) or `particle_radius` / `coefficients` go into a ``config.yaml`` next to the file -- the frame
    does not carry the particle radius, and a player needs it -- unless one is there already."""

    def __init__(self, path, *, particle_radius: float | None = None, coefficients: dict | None = None,
                 config: dict | None = None) -> None:
        self.path = Path(path)
        self.path.parent.mkdir(exist_ok=True, parents=True)
        self.frames = 0
        self._f = open(self.path, "wb")
        self._f.write(FILE_MAGIC + struct.pack("<I", FILE_VERSION) + bytes(4))
        side = self.path.parent / "config.yaml"
        if config is None and (particle_radius is not None or coefficients is not None):
            coef = dict(coefficients or {})
            if particle_radius is not None:
                coef["particle_radius"] = float(particle_radius)
            config = {"world_config": {"coefficients": coef}}
        if config is not None and not side.exists():
            with open(side, "w") as f:
                yaml.safe_dump(config, f)

    def write(self, frame) -> None:
        frame = bytes(frame)
        if frame_length(frame) != len(frame):
            raise TrackError(f"{len(frame)} bytes; the header announces {frame_length(frame)}")
        self._f.write(frame)
        self.frames += 1

    def write_all(self, frames) -> None:
        for frame in frames:
            self.write(frame)

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class TrackReader:
    """Indexes the frames of a track file (or of the track.sctk in a directory): `len()`, `reader[k]` (bytes), iteration.
    A file cut off in the middle of a frame yields the complete frames before the cut; `truncated` says so."""

    def __init__(self, path) -> None:
        self.path = resolve_path(path)
        self._f = open(self.path, "rb")
        head = self._f.read(FILE_HEADER)
        if len(head) < FILE_HEADER or head[:8] != FILE_MAGIC:
            self._f.close()
            raise TrackError(f"{self.path} is not a track file")
        if struct.unpack_from("<I", head, 8)[0] != FILE_VERSION:
            self._f.close()
            raise TrackError(f"track file of version {struct.unpack_from('<I', head, 8)[0]}; this reads {FILE_VERSION}")
        size = self.path.stat().st_size
        self._index: list[tuple[int, int]] = []
        self.truncated = False
        at = FILE_HEADER
        while at < size:
            self._f.seek(at)
            head = self._f.read(HEADER)
            if len(head) < HEADER:
                self.truncated = True
                break
            length = frame_length(head)
            if at + length > size:
                self.truncated = True
                break
            self._index.append((at, length))
            at += length

    def __len__(self) -> int:
        return len(self._index)

    def __getitem__(self, k: int) -> bytes:
        at, length = self._index[k]
        self._f.seek(at)
        return self._f.read(length)

    def __iter__(self):
        for k in range(len(self)):
            yield self[k]

    def ticks(self) -> list[int]:
        out = []
        for at, _ in self._index:
            self._f.seek(at + 8)
            out.append(struct.unpack("<q", self._f.read(8))[0])
        return out

    def particle_radius(self) -> float | None:
        """From the config.yaml next to the file, if there is one."""
        side = self.path.parent / "config.yaml"
        if not side.exists():
            return None
        with open(side) as f:
            doc = yaml.safe_load(f) or {}
        try:
            return float(doc["world_config"]["coefficients"]["particle_radius"])
        except (KeyError, TypeError, ValueError):
            return None

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def hud_text(frame) -> str:
    """What `hud=True` writes: the first two lines of the live HUD, from the frame's header."""
    _, _, tick, n, _, _, _, _ = _HEADER.unpack_from(frame, 0)
    return f"Tick: {tick}\nParticles: {n}"


class Player:
    """Turns frames into pictures through the engine's own render paths, at any view: owns an `Engine`, loads a frame into
    it (sc_track_load) and renders with the frame's own walls.  `particle_radius` (world units) sizes the discs -- the
    frame does not carry it; give it here or per call.  `capacity` is the most particles a frame may hold (default: the
    engine grows to the largest frame seen)."""

    def __init__(self, capacity: int | None = None, device: int = 0, particle_radius: float | None = None) -> None:
        from .addons import Overlay
        from .engine import Engine
        self._Engine = Engine
        self.device = int(device)
        self.particle_radius = particle_radius
        self._fixed = capacity is not None
        self._engine = Engine(max(int(capacity or 1024), 1), device=self.device)
        self._overlay = Overlay()  # (the HUD text the engine was last told to draw)

    @property
    def engine(self):
        return self._engine

    def close(self) -> None:
        self._engine.close()

    def load(self, frame, plain: bool = False) -> dict:
        """The frame becomes the engine's state; -> its parsed header fields and walls (`parse` without the planes)."""
        frame = bytes(frame)
        _, _, tick, n, nseg, flags, _, _ = _HEADER.unpack_from(frame, 0) if len(frame) >= HEADER else (0,) * 8
        if len(frame) >= HEADER and frame[:4] == MAGIC and n > self._engine.capacity and not self._fixed:
            self._engine.close()
            self._engine = self._Engine(int(n * 1.25) + 1024, device=self.device)
            self._overlay.enter(self._engine)  # (a new context has no HUD)
        self._engine.track_load(frame, plain)
        seg = np.frombuffer(frame, dtype="<f8", count=4 * nseg, offset=HEADER).reshape(nseg, 2, 2)
        return dict(tick=tick, n=n, flags=flags, segments=seg)

    def _prepare(self, frame, width, zoom, center, segment_width, hud, plain, particle_radius, height):
        from .addons import hud_request
        radius = self.particle_radius if particle_radius is None else particle_radius
        if radius is None:
            raise TrackError("the frame does not carry the particle radius: give particle_radius to Player or to the call")
        info = self.load(frame, plain)
        self._overlay.send(self._engine, "hud", hud_request(hud, hud_text(frame) if hud is True else None, width))
        view = self._Engine.view(width, height, radius, zoom=zoom, center=center, segment_width=segment_width)
        return view, info["segments"]

    def render(self, frame, width: int = 1000, height: int = 1000, *, zoom: float = 1.0, center=None,
               segment_width: int = 2, hud=None, plain: bool = False, particle_radius: float | None = None) -> np.ndarray:
        """`Crate.render`'s picture of the frame: height x width x 3 uint8.  `hud=True` writes ``Tick: ...`` and
        ``Particles: ...`` from the frame's header, a str that string; `plain` paints every disc (100, 100, 255), the
        reference's colour for recorded particles."""
        view, seg = self._prepare(frame, width, zoom, center, segment_width, hud, plain, particle_radius, height)
        return self._engine.render(view, seg)

    def render_jpeg(self, frame, width: int = 1000, height: int = 1000, *, quality: int = 95, zoom: float = 1.0,
                    center=None, segment_width: int = 2, hud=None, plain: bool = False,
                    particle_radius: float | None = None) -> bytes:
        view, seg = self._prepare(frame, width, zoom, center, segment_width, hud, plain, particle_radius, height)
        return self._engine.render_jpeg(view, seg, quality)

    def render_gif(self, frame, width: int = 1000, height: int = 1000, *, zoom: float = 1.0, center=None,
                   segment_width: int = 2, hud=None, plain: bool = False, particle_radius: float | None = None) -> bytes:
        view, seg = self._prepare(frame, width, zoom, center, segment_width, hud, plain, particle_radius, height)
        return self._engine.render_gif(view, seg)
