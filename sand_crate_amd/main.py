"""Headless driver: the reference's CLI (``src/main.py:19-40``) and frame loop
(``src/playback.py:51-65``) without a window.

    python -m sand_crate_amd.main config/wave_machine.yaml [play_recording_dir] [--variants 1] [--ticks N]

Like the reference it walks the 48 coefficient combinations of ``options`` (main.py:10-16, :26-36) --
mutating the loaded config in place, variant after variant -- and runs ``ticks_to_record`` ticks
for each.  Instead of rendering, a variant's recording is the particle state itself: where the
reference writes config.yaml + AVI + GIF (playback.py:109-118) this writes config.yaml + state.npz
(positions, pressure and segments every ``--record-every`` ticks), the state dump the reference
left commented out (playback.py:112-113).  ``--frames`` also renders a ``screen_x`` x ``screen_y`` picture at every
recorded tick on the GPU (`Crate.render`, what Playback.draw_scene draws) and writes them as ``frames.npz`` and, when PIL
is installed, ``video.gif`` (playback.py:131-138).  ``--video`` renders the same frames and encodes them as JPEG on the GPU
(`Crate.render_jpeg`, quality ``--video-quality``, default 95 as cv2's); only the compressed frames leave it, and they
are streamed into ``video.avi``, Motion-JPEG at 50 fps as playback.py:120-129 writes it.  ``--gif`` does the same for
``video.gif``: every recorded tick is rendered and LZW-compressed on the GPU (`Crate.render_gif`) and streamed into the file
(`gif.GifWriter`; 10 ms per frame, looping, as playback.py:131-138), without PIL and without keeping frames in memory;
with ``--frames`` as well, ``frames.npz`` is still written and this ``video.gif`` is the one kept.  ``--hud`` writes the
HUD text the reference's viewer shows (`Crate.debug_prints`: tick, particle count, timing and the coefficient list --
what tells one variant's video from the next) on every frame of ``--frames``, ``--video`` and ``--gif``, on the GPU, in
a built-in bitmap font.  ``--arrows [EVERY]`` draws the viewer's debug-arrow layer on the same frames, fed from the
device: a green arrow along the velocity of every EVERY-th particle (`Crate.render(arrows="velocity")`).
``--observe [BINS]`` records numbers instead of pictures: every tick the device reduces the state to the sixteen
observables of `probe.FIELDS` (particle count, momentum and kinetic-energy sums, extents, pressure) and, with BINS, a
profile of the free surface in BINS columns over the world's width, into a log in device memory (`Crate.observe`) that is
read every 4096 ticks and written as ``observables.npz`` next to ``config.yaml``.
``--track [EVERY]`` records the run itself as packed frames (`Crate.track`): every EVERY-th tick the device packs the state
into nine bytes per particle in a log in device memory -- no download and no synchronisation in the tick loop -- which is
read when the host's bound of the particle count says the next frames may no longer fit, and streamed into ``track.sctk``
(`track.TrackWriter`); ``python -m sand_crate_amd.replay`` turns that file into frames or videos at any view.
``--trajectory [EVERY]`` records the run at full precision (`Crate.record_trajectory`): every EVERY-th tick the device writes
positions and velocities as float64 into a log in device memory, one row per particle id -- no sort, no download and no
synchronisation in the tick loop; the log holds a frame for the initial state and for every EVERY-th of the variant's ticks,
is read once at the end of the variant and written as ``trajectory.npz`` (states, ticks, counts, outside, dropped, id0).
``--checkpoint-every K`` also writes resumable checkpoints
(``checkpoint_<tick>.npz``: `Crate.begin_checkpoint` captures the state on the device and sends it to pinned host
memory on a side stream while the following ticks run); ``--resume FILE`` continues such a run.
"""
from __future__ import annotations

import argparse
import time
from datetime import datetime
from itertools import product
from pathlib import Path
from typing import Optional

import numpy as np
import yaml

from .avi import AviWriter
from .crate import Crate
from .gif import GifWriter
from .load_config import Config, load_config
from .probe import FIELDS, concatenate
from .track import FILE_NAME as TRACK_FILE, TrackWriter, frame_bytes

OBSERVE_EVERY = 4096  # ticks between two reads of the device log of --observe (its capacity)
TRACK_LOG_BYTES = 1 << 26  # the device log of --track: at least this, and at least four frames of max_particles

options = {
    "pressure_amplifier": [20, 40],
    "ignored_pressure": [0.3, 0.1],
    "viscosity": [4, 8],
    "surface_smoothing": [40, 100],
    "target_pressure": [-5, -2, 2],
}


def config_options(options: dict, config: Config):
    """Every combination of the listed coefficient values, written into the SAME config object
    (the reference's generator semantics, main.py:26-36)."""
    names = list(options)
    for values in product(*(options[name] for name in names)):
        for name, value in zip(names, values):
            config.world_config.coefficients[name] = value
        yield config


def deep_dictify(obj):
    """Plain-data view of a config for yaml.safe_dump (objects_utils.py:21-33)."""
    if isinstance(obj, (str, int, float)) or obj is None:
        return obj
    if isinstance(obj, Path):
        return str(obj)
    if isinstance(obj, np.ndarray):
        return obj.tolist()
    if isinstance(obj, (list, tuple)):
        return [deep_dictify(x) for x in obj]
    if isinstance(obj, dict):
        return {str(k): deep_dictify(v) for k, v in obj.items()}
    return {str(k): deep_dictify(v) for k, v in vars(obj).items()}


class HeadlessPlayback:
    """`Playback` minus pygame: owns a `Crate`, ticks it, records state (and, with `frames`, rendered pictures)."""

    def __init__(self, config: Config, recording_dir_path: Optional[Path] = None, *, noise: str = "host",
                 record_every: int = 10, device: int = 0, checkpoint_every: int = 0,
                 resume: Optional[Path] = None, frames: bool = False, video: bool = False,
                 video_quality: int = 95, gif: bool = False, hud: bool = False, arrows: int = 0,
                 observe: Optional[int] = None, track: int = 0, trajectory: int = 0) -> None:
        self.config = config
        if recording_dir_path is None:
            stamp = datetime.now().strftime("%Y%m%d_%H%M%S")
            self.recording_dir_path = Path(config.playback_config.recording_output_dir_path) / stamp
        else:
            self.recording_dir_path = Path(recording_dir_path)
        self.crate = (Crate.from_checkpoint(resume, device=device) if resume is not None
                      else Crate(config.world_config, noise=noise, device=device))
        self.checkpoint_every = max(int(checkpoint_every), 0)
        self.checkpoints: list[Path] = []
        self._checkpoint_tick = None
        self.record_every = max(int(record_every), 1)
        self.frames: list[dict] = []
        self.render_frames = bool(frames)
        self.images: list[np.ndarray] = []
        self.video = bool(video)
        self.video_quality = int(video_quality)
        self.video_frames = 0
        self.gif = bool(gif)
        self.gif_frames = 0
        self.hud = bool(hud)
        self.arrows = max(int(arrows or 0), 0)  # velocity arrows for every this-many-th particle; 0: none
        self.observe = None if observe is None else max(int(observe), 0)  # bins of the profile (0: none); None: no log
        self.observed: list[dict] = []
        self.observables: Optional[dict] = None
        self.track = max(int(track or 0), 0)  # a packed frame every this-many-th tick into track.sctk; 0: none
        self.track_frames = 0
        self.track_dropped = 0
        self._track_writer = None  # the TrackWriter of track.sctk while a variant with --track runs
        self.trajectory = max(int(trajectory or 0), 0)  # a full-precision frame every this-many-th tick; 0: none
        self.recorded: Optional[dict] = None  # what trajectory.npz holds, once the variant has run
        self.done = False
        self.seconds = 0.0

    def run_live_simulation(self, ticks: Optional[int] = None) -> None:
        n = self.config.playback_config.ticks_to_record if ticks is None else ticks
        t0 = time.perf_counter()
        pb = self.config.playback_config
        avi = None
        if self.video:
            self.recording_dir_path.mkdir(exist_ok=True, parents=True)
            avi = AviWriter(self.recording_dir_path / "video.avi", int(pb.screen_x), int(pb.screen_y), fps=50)
        gif = None
        try:
            if self.gif:
                self.recording_dir_path.mkdir(exist_ok=True, parents=True)
                gif = GifWriter(self.recording_dir_path / "video.gif", int(pb.screen_x), int(pb.screen_y), delay_cs=1, loop=0,
                                arrows=self.arrows > 0)
            if getattr(self, "track", 0):
                self._track_begin()
            if getattr(self, "trajectory", 0):  # the initial state and every `trajectory`-th of the n ticks
                self.crate.record_trajectory(int(n) // self.trajectory + 2, every=self.trajectory)
            self._run(int(n), avi, gif)
            self._trajectory_end()
        finally:
            self.crate.stop_trajectory()
            self._track_end()
            if avi is not None:
                self.video_frames = avi.frames
                avi.close()
            if gif is not None:
                self.gif_frames = gif.frames
                gif.close()
        self._collect_checkpoint()
        self.crate.synchronize()
        self.seconds = time.perf_counter() - t0
        if self.config.playback_config.save_recording:
            self.save_recording(self.recording_dir_path)

    def _run(self, n: int, avi: Optional[AviWriter], gif: Optional[GifWriter] = None) -> None:
        pb = self.config.playback_config
        hud = True if self.hud else None
        arrows = dict(arrows="velocity", arrow_every=self.arrows) if self.arrows else {}
        observe = getattr(self, "observe", None)
        if observe is not None:
            self.crate.observe(capacity=max(min(n, OBSERVE_EVERY), 1), bins=observe, x_range=(0.0, 1.0))
        for k in range(n):
            self.crate.physics_tick()
            if self._track_writer is not None and self.crate.tick % self.track == 0:
                self._track_tick()
            if observe is not None and (k + 1) % OBSERVE_EVERY == 0:
                self.observed.append(self.crate.observations())
            if self.checkpoint_every and self.crate.tick % self.checkpoint_every == 0:
                self._collect_checkpoint()        # the previous one has long arrived
                self.crate.begin_checkpoint()     # returns at once; the transfer overlaps the next ticks
                self._checkpoint_tick = self.crate.tick
            if self.crate.tick % self.record_every == 0:
                self.frames.append({"tick": self.crate.tick, "particles": self.crate.particles.copy(),
                                    "pressure": self.crate.particles_pressure.copy(),
                                    "segments": self.crate.segments.copy()})
                if self.render_frames:
                    self.images.append(self.crate.render(int(pb.screen_x), int(pb.screen_y), hud=hud, **arrows))
                if avi is not None:
                    avi.write(self.crate.render_jpeg(int(pb.screen_x), int(pb.screen_y), quality=self.video_quality,
                                                     hud=hud, **arrows))
                if gif is not None:
                    gif.write(self.crate.render_gif(int(pb.screen_x), int(pb.screen_y), hud=hud, **arrows))
            if self.done:
                break
        if observe is not None:
            self.observed.append(self.crate.observations())
            self.crate.observe(False)
            self.observables = concatenate(self.observed, observe)
            self.observed = []

    # --track: the log lives on the device; the host only keeps an upper bound of the bytes it may hold by now
    def _track_frame_bound(self) -> int:
        crate = self.crate
        most = max(int(crate.max_particles), crate.engine.capacity)  # (the device never stores more than either)
        return frame_bytes(most, len(crate.segments) if crate.rigid_bodies else 0)

    def _track_begin(self) -> None:
        self.recording_dir_path.mkdir(exist_ok=True, parents=True)
        self._track_writer = TrackWriter(self.recording_dir_path / TRACK_FILE, config=deep_dictify(self.config))
        self._track_capacity = max(TRACK_LOG_BYTES, 4 * self._track_frame_bound())
        self._track_used = 0
        self.crate.track(every=self.track, capacity_bytes=self._track_capacity)

    def _track_drain(self) -> None:
        frames, dropped = self.crate.tracked()
        self._track_writer.write_all(frames)
        self.track_dropped += dropped
        self._track_used = 0

    def _track_tick(self) -> None:
        """After a tick that logged a frame: read the log out when the next frame may no longer fit."""
        self._track_used += self._track_frame_bound()
        if self._track_used + self._track_frame_bound() > self._track_capacity:
            self._track_drain()

    def _track_end(self) -> None:
        writer = self._track_writer
        if writer is None:
            return
        try:
            self._track_drain()
            self.crate.track(False)
        finally:
            self.track_frames = writer.frames
            writer.close()
            self._track_writer = None

    def _trajectory_end(self) -> None:
        """--trajectory: the log is read once, when the variant has run."""
        recording = getattr(self.crate, "_trajectory", None)
        if recording is None:
            return
        got = recording.read()
        self.recorded = {name: got[name].cpu().numpy() for name in ("states", "ticks", "counts", "outside")}
        self.recorded.update(dropped=np.int64(got["dropped"]), id0=np.int64(recording.id0))

    def _collect_checkpoint(self) -> None:
        if self._checkpoint_tick is None:
            return
        self.recording_dir_path.mkdir(exist_ok=True, parents=True)
        path = self.recording_dir_path / f"checkpoint_{self._checkpoint_tick:06d}.npz"
        self.crate.finish_checkpoint(path)
        self.checkpoints.append(path)
        self._checkpoint_tick = None

    def save_recording(self, out_dir: Path) -> None:
        out_dir.mkdir(exist_ok=True, parents=True)
        with open(out_dir / "config.yaml", "w") as f:
            yaml.safe_dump(deep_dictify(self.config), f)
        arrays = {}
        for k, frame in enumerate(self.frames):
            arrays[f"particles_{k}"] = frame["particles"]
            arrays[f"pressure_{k}"] = frame["pressure"]
            arrays[f"segments_{k}"] = frame["segments"]
        arrays["ticks"] = np.array([f["tick"] for f in self.frames], dtype=np.int64)
        np.savez_compressed(out_dir / "state.npz", **arrays)
        observables = getattr(self, "observables", None)
        if observables is not None:
            np.savez_compressed(out_dir / "observables.npz", fields=np.array(FIELDS), x_range=np.array([0.0, 1.0]),
                                dt=np.float64(self.crate.dt), **observables)
        recorded = getattr(self, "recorded", None)
        if recorded is not None:
            np.savez_compressed(out_dir / "trajectory.npz", **recorded)
        if self.render_frames:
            write_frames(out_dir, self.images, arrays["ticks"], gif=not self.gif)


def write_frames(out_dir: Path, frames, ticks, gif: bool = True) -> None:
    """frames.npz (`frames` T x H x W x 3 uint8, `ticks`) and, with `gif` and when PIL is installed, video.gif as
    playback.py:131-138 writes it (`gif=False`: the caller has written, or does not want, a video.gif)."""
    out_dir = Path(out_dir)
    frames = [np.asarray(f, dtype=np.uint8) for f in frames]
    stack = np.stack(frames) if frames else np.zeros((0, 0, 0, 3), dtype=np.uint8)
    np.savez_compressed(out_dir / "frames.npz", frames=stack, ticks=np.asarray(ticks, dtype=np.int64))
    if not frames or not gif:
        return
    try:
        from PIL import Image
    except ImportError:
        return
    images = [Image.fromarray(f, "RGB") for f in frames]
    images[0].save(out_dir / "video.gif", format="GIF", append_images=images[1:], save_all=True, duration=10, loop=0)


def main(config_file_path, play_recording: Optional[Path] = None, *, variants: Optional[int] = None,
         ticks: Optional[int] = None, noise: str = "host", record_every: int = 10, checkpoint_every: int = 0,
         resume: Optional[Path] = None, frames: bool = False, video: bool = False,
         video_quality: int = 95, gif: bool = False, hud: bool = False, arrows: int = 0,
         observe: Optional[int] = None, track: int = 0, trajectory: int = 0) -> list[dict]:
    config = load_config(config_file_path=config_file_path)
    summary = []
    for k, variant in enumerate(config_options(options, config)):
        if variants is not None and k >= variants:
            break
        out = Path(play_recording) / f"variant_{k:02d}" if play_recording is not None else None
        playback = HeadlessPlayback(config=variant, recording_dir_path=out, noise=noise, record_every=record_every,
                                    checkpoint_every=checkpoint_every, resume=resume if k == 0 else None, frames=frames,
                                    video=video, video_quality=video_quality, gif=gif, hud=hud, arrows=arrows,
                                    **({} if observe is None else {"observe": observe}),
                                    **({"track": track} if track else {}),
                                    **({"trajectory": trajectory} if trajectory else {}))
        playback.run_live_simulation(ticks)
        summary.append({"variant": k, "ticks": playback.crate.tick, "particles": playback.crate.particle_count,
                        "seconds": playback.seconds,
                        "coefficients": {name: variant.world_config.coefficients[name] for name in options}})
        last = ""
        if observe is not None:  # the last logged tick in numbers
            obs = playback.observables
            for name in ("sum_ke", "max_speed2", "n"):
                summary[-1][name] = float(obs[name][-1]) if len(obs[name]) else float("nan")
            last = f", sum_ke {summary[-1]['sum_ke']:.6g}, max_speed2 {summary[-1]['max_speed2']:.6g}, n {summary[-1]['n']:.0f}"
        print(f"variant {k}: {summary[-1]['ticks']} ticks, {summary[-1]['particles']} particles, "
              f"{playback.seconds:.2f} s{last} -> {playback.recording_dir_path}")
    return summary


def argument_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("config_file_path", type=Path)
    ap.add_argument("play_recording", type=Path, nargs="?", default=None)
    ap.add_argument("--variants", type=int, default=None, help="stop after this many of the 48 combinations")
    ap.add_argument("--ticks", type=int, default=None, help="override playback.ticks_to_record")
    ap.add_argument("--noise", default="host", choices=["host", "host-sync", "counter", "none"])
    ap.add_argument("--record-every", type=int, default=10)
    ap.add_argument("--checkpoint-every", type=int, default=0, help="write a resumable checkpoint every K ticks (0 = never)")
    ap.add_argument("--resume", type=Path, default=None, help="continue the first variant from this checkpoint file")
    ap.add_argument("--frames", action="store_true", help="also render a frame every --record-every ticks (frames.npz, "
                    "video.gif)")
    ap.add_argument("--video", action="store_true", help="also render and JPEG-encode a frame on the GPU every "
                    "--record-every ticks, streamed into video.avi (Motion-JPEG, 50 fps)")
    ap.add_argument("--video-quality", type=int, default=95, help="JPEG quality of --video, 1..100 (default 95)")
    ap.add_argument("--gif", action="store_true", help="also render and LZW-compress a frame on the GPU every "
                    "--record-every ticks, streamed into video.gif (10 ms per frame, looping); replaces the video.gif "
                    "of --frames")
    ap.add_argument("--hud", action="store_true", help="write the HUD text (tick, particle count, timing, coefficients) on "
                    "every frame of --frames, --video and --gif")
    ap.add_argument("--arrows", type=int, nargs="?", const=1, default=0, metavar="EVERY", help="draw a green arrow along "
                    "the velocity of every EVERY-th particle (default: every one) on every frame of --frames, --video and "
                    "--gif")
    ap.add_argument("--observe", type=int, nargs="?", const=0, default=None, metavar="BINS", help="log the observables of "
                    "every tick on the GPU (particle count, momentum and kinetic-energy sums, extents, pressure) and, "
                    "with BINS, the free surface in BINS columns; written as observables.npz")
    ap.add_argument("--track", type=int, nargs="?", const=1, default=0, metavar="EVERY", help="record every EVERY-th tick "
                    "(default: every one) as a packed frame on the GPU, nine bytes per particle, streamed into track.sctk; "
                    "python -m sand_crate_amd.replay draws it at any view")
    ap.add_argument("--trajectory", type=int, nargs="?", const=1, default=0, metavar="EVERY", help="record every EVERY-th "
                    "tick (default: every one) at full precision on the GPU, float64 positions and velocities in one row "
                    "per particle id, read once at the end and written as trajectory.npz")
    return ap


if __name__ == "__main__":
    a = argument_parser().parse_args()
    main(a.config_file_path, a.play_recording, variants=a.variants, ticks=a.ticks, noise=a.noise,
         record_every=a.record_every, checkpoint_every=a.checkpoint_every, resume=a.resume, frames=a.frames,
         video=a.video, video_quality=a.video_quality, gif=a.gif, hud=a.hud, arrows=a.arrows, observe=a.observe,
         track=a.track, trajectory=a.trajectory)
