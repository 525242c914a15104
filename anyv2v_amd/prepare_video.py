"""Crop and resize source clips to the working size on the GPU -- the counterpart of the reference's top-level ``prepare_video.py``
for what can be read here: a directory of ``%05d.png`` frames, or an mp4 that ``anyv2v_amd.mp4`` reads.

    python -m anyv2v_amd.prepare_video --video_path demo/clip --output_folder processed_video_data --width 512 --height 512 \
                                       --n_frames 16 --center_crop --x_offset -0.3

``--video_path`` names one clip, ``--input_folder`` a folder of them (its mp4 files and its frame directories).  Of the ``N`` frames a
clip has, frame ``(i * N) // n_frames`` becomes output frame ``i`` (the reference's ``extract_frames`` takes ``n_frames`` evenly spaced
instants from 0, the end excluded); fewer than ``n_frames`` available is refused.  With ``--center_crop`` the frame is scaled until it
covers ``width x height`` and cropped at the offsets (-1 left / top .. 1 right / bottom), otherwise it is resized to ``width x height``;
every resize is Pillow's LANCZOS byte for byte (``anyv2v_amd.prepare``).  The frames are written as ``<output_folder>/<name>/%05d.png``:
a directory the runners read, whose frame 0 is the one to edit.  ``--start_time`` / ``--end_time`` / ``--clip_duration`` cut a clip
by a decoder's timestamps and are refused: there is no decoder here, select the frames instead."""
from __future__ import annotations

import argparse
import glob
import os

import torch
from PIL import Image

from . import prepare
from .utils import load_image


def read_clip(path):
    """Every frame of a clip at its own size: a directory of consecutive ``%05d.png`` files from 00000, or an mp4."""
    if os.path.isdir(path):
        frames = []
        while os.path.isfile(os.path.join(path, "%05d.png" % len(frames))):
            frames.append(load_image(os.path.join(path, "%05d.png" % len(frames))))
        if not frames:
            raise ValueError(f"{path}: no 00000.png in this directory")
        return frames
    from .mp4 import Mp4Unsupported, read_mp4
    try:
        return list(read_mp4(path)[0])
    except Mp4Unsupported as e:
        raise ValueError(f"cannot decode {path}: {e}; no video decoder library is available here -- give a directory of %05d.png frames") from e


def select_frames(frames, n_frames):
    n = len(frames)
    if n_frames < 1 or n < n_frames:
        raise ValueError(f"n_frames={n_frames}: the clip has {n} frames")
    return [frames[(i * n) // n_frames] for i in range(n_frames)]


def prepare_clip(path, output_folder, width, height, n_frames, center_crop, x_offset, y_offset, device):
    if not center_crop and (x_offset != 0 or y_offset != 0):
        raise ValueError("--x_offset / --y_offset without --center_crop: nothing is cropped")
    frames = select_frames(read_clip(path), n_frames)
    out = prepare.prepare_frames(frames, height, width, fit="crop" if center_crop else "stretch", x_offset=x_offset, y_offset=y_offset,
                                 device=device)
    name = os.path.splitext(os.path.basename(os.path.normpath(path)))[0]
    out_dir = os.path.join(output_folder, name)
    prepare.save_frames([Image.fromarray(f) for f in out.cpu().numpy()], out_dir)
    print(f"Processed {path}, saved {n_frames} frames of {width} x {height} to {out_dir}")
    return out_dir


def main(argv=None):
    parser = argparse.ArgumentParser(description="Crop and resize video clips to the working size.")
    parser.add_argument("--input_folder", type=str, help="folder of clips: its *.mp4 files and its frame directories")
    parser.add_argument("--video_path", type=str, default=None, help="one clip: a directory of %%05d.png frames, or an mp4")
    parser.add_argument("--output_folder", type=str, default="processed_video_data")
    parser.add_argument("--width", type=int, default=512)
    parser.add_argument("--height", type=int, default=512)
    parser.add_argument("--n_frames", type=int, default=16, help="frames to take from each clip, evenly spaced")
    parser.add_argument("--center_crop", action="store_true", help="scale to cover width x height, then crop")
    parser.add_argument("--x_offset", type=float, default=0, help="horizontal crop position, -1 (left) .. 1 (right)")
    parser.add_argument("--y_offset", type=float, default=0, help="vertical crop position, -1 (top) .. 1 (bottom)")
    parser.add_argument("--device", type=str, default="cuda:0")
    for name in ("--start_time", "--end_time", "--clip_duration"):
        parser.add_argument(name, type=float, default=None, help="refused: needs a decoder's timestamps")
    args = parser.parse_args(argv)
    for name in ("start_time", "end_time", "clip_duration"):
        if getattr(args, name) is not None:
            parser.error(f"--{name} cuts the clip by a decoder's timestamps, and there is no decoder here: pass the frames you want "
                         "(a %05d.png directory) and choose among them with --n_frames")
    if (args.video_path is None) == (args.input_folder is None):
        parser.error("give one of --video_path and --input_folder")
    if args.video_path is not None:
        clips = [args.video_path]
    else:
        clips = sorted(glob.glob(os.path.join(args.input_folder, "*.mp4"))
                       + [d for d in glob.glob(os.path.join(args.input_folder, "*")) if os.path.isfile(os.path.join(d, "00000.png"))])
        if not clips:
            parser.error(f"no clips found in {args.input_folder}")
    with torch.no_grad():
        return [prepare_clip(c, args.output_folder, args.width, args.height, args.n_frames, args.center_crop, args.x_offset, args.y_offset,
                             torch.device(args.device)) for c in clips]


if __name__ == "__main__":
    main()
