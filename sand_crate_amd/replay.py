"""Replay a recording of packed frames as pictures, at any view, without simulating again.

    python -m sand_crate_amd.replay PATH [--gif] [--video] [--frames] [--width W] [--height H] [--zoom Z]
                                         [--center X Y] [--hud] [--plain] [--every K] [--out DIR]

PATH is a ``track.sctk`` (`main --track` writes one per variant) or a variant directory that holds one.  Every K-th
frame of it is loaded into a GPU context (`track.Player`: sc_track_load) and drawn through the render paths the live
driver uses, with the frame's own walls: ``--gif`` streams ``video.gif`` (`gif.GifWriter`), ``--video`` ``video.avi``
(`avi.AviWriter`, Motion-JPEG at 50 fps), ``--frames`` writes ``frames.npz``.  The view is free -- size, ``--zoom``,
``--center`` in screen pixels -- because nothing of it is baked into the recording.  ``--hud`` writes the tick and the
particle count of each frame's header; ``--plain`` paints every particle in the reference's playback colour,
(100, 100, 255), instead of by its recorded pressure.  The particle radius comes from the ``config.yaml`` next to the
file, or from ``--radius``.  Frames carry no velocities, so there are no velocity arrows here.
"""
from __future__ import annotations

import argparse
from pathlib import Path
from typing import Optional

import numpy as np

from .track import TrackError, TrackReader, resolve_path

OUTPUT_NAMES = {"gif": "video.gif", "video": "video.avi", "frames": "frames.npz"}


def argument_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m sand_crate_amd.replay", description=__doc__.split("\n\n")[0])
    ap.add_argument("path", type=Path, help="a track.sctk, or a variant directory that holds one")
    ap.add_argument("--gif", action="store_true", help="write video.gif (10 ms per frame, looping)")
    ap.add_argument("--video", action="store_true", help="write video.avi (Motion-JPEG, 50 fps)")
    ap.add_argument("--video-quality", type=int, default=95, help="JPEG quality of --video, 1..100 (default 95)")
    ap.add_argument("--frames", action="store_true", help="write frames.npz (frames T x H x W x 3 uint8, ticks)")
    ap.add_argument("--width", type=int, default=1000)
    ap.add_argument("--height", type=int, default=1000)
    ap.add_argument("--zoom", type=float, default=1.0)
    ap.add_argument("--center", type=float, nargs=2, default=None, metavar=("X", "Y"),
                    help="the view's centre in screen pixels (default: the frame's centre)")
    ap.add_argument("--segment-width", type=int, default=2)
    ap.add_argument("--hud", action="store_true", help="write each frame's tick and particle count on it")
    ap.add_argument("--plain", action="store_true", help="every particle in the playback colour (100, 100, 255)")
    ap.add_argument("--every", type=int, default=1, metavar="K", help="draw every K-th frame of the recording")
    ap.add_argument("--radius", type=float, default=None, help="particle radius in world units (default: from the "
                    "config.yaml next to the recording)")
    ap.add_argument("--out", type=Path, default=None, metavar="DIR", help="where to write (default: next to the recording)")
    ap.add_argument("--device", type=int, default=0)
    return ap


def output_paths(path, out: Optional[Path], gif: bool, video: bool, frames: bool) -> dict:
    """{"gif" | "video" | "frames": file} for the outputs asked for: in `out`, else next to the recording."""
    where = Path(out) if out is not None else resolve_path(path).parent
    return {kind: where / name for kind, name in OUTPUT_NAMES.items() if {"gif": gif, "video": video, "frames": frames}[kind]}


def selected(n_frames: int, every: int) -> list[int]:
    if every < 1:
        raise ValueError("--every must be at least 1")
    return list(range(0, n_frames, every))


def replay(path, *, gif: bool = False, video: bool = False, frames: bool = False, width: int = 1000, height: int = 1000,
           zoom: float = 1.0, center=None, segment_width: int = 2, hud: bool = False, plain: bool = False, every: int = 1,
           radius: Optional[float] = None, out: Optional[Path] = None, video_quality: int = 95, device: int = 0) -> dict:
    """-> {"frames": how many were drawn, "ticks": theirs, "truncated": the file was cut off, "outputs": {kind: path}}."""
    from .avi import AviWriter
    from .gif import GifWriter
    from .track import Player
    outputs = output_paths(path, out, gif, video, frames)
    if not outputs:
        raise ValueError("nothing to write: give --gif, --video or --frames")
    with TrackReader(path) as reader:
        if radius is None:
            radius = reader.particle_radius()
        if radius is None:
            raise TrackError(f"no config.yaml with a particle_radius next to {reader.path}: give --radius")
        picks = selected(len(reader), every)
        for target in outputs.values():
            target.parent.mkdir(exist_ok=True, parents=True)
        player = Player(device=device, particle_radius=radius)
        view = dict(zoom=zoom, center=center, segment_width=segment_width, hud=True if hud else None, plain=plain)
        avi = gif_writer = None
        images, ticks = [], []
        try:
            if "video" in outputs:
                avi = AviWriter(outputs["video"], int(width), int(height), fps=50)
            if "gif" in outputs:
                gif_writer = GifWriter(outputs["gif"], int(width), int(height), delay_cs=1, loop=0)
            for k in picks:
                frame = reader[k]
                ticks.append(int.from_bytes(frame[8:16], "little", signed=True))
                if "frames" in outputs:
                    images.append(player.render(frame, width, height, **view))
                if avi is not None:
                    avi.write(player.render_jpeg(frame, width, height, quality=video_quality, **view))
                if gif_writer is not None:
                    gif_writer.write(player.render_gif(frame, width, height, **view))
        finally:
            if avi is not None:
                avi.close()
            if gif_writer is not None:
                gif_writer.close()
            player.close()
        if "frames" in outputs:
            stack = np.stack(images) if images else np.zeros((0, height, width, 3), dtype=np.uint8)
            np.savez_compressed(outputs["frames"], frames=stack, ticks=np.asarray(ticks, dtype=np.int64))
        return {"frames": len(picks), "ticks": ticks, "truncated": reader.truncated, "outputs": outputs}


def main(argv=None) -> dict:
    a = argument_parser().parse_args(argv)
    done = replay(a.path, gif=a.gif, video=a.video, frames=a.frames, width=a.width, height=a.height, zoom=a.zoom,
                  center=a.center, segment_width=a.segment_width, hud=a.hud, plain=a.plain, every=a.every, radius=a.radius,
                  out=a.out, video_quality=a.video_quality, device=a.device)
    cut = " (the file is cut off: the complete frames before the cut)" if done["truncated"] else ""
    print(f"{done['frames']} frames{cut} -> " + ", ".join(str(p) for p in done["outputs"].values()))
    return done


if __name__ == "__main__":
    main()
