"""Cost of the tiled VAE decode at the pipeline's default frame (704 x 1280, 16 frames): the stitch launch alone next to a
device-to-device copy of the same output bytes, and the whole tiled decode.  Prints a markdown table (profiles/vae_tiling_cost.md).

    python tools/vae_tiling_cost.py [--frames 16] [--reps 20]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anyv2v_amd import ops  # noqa: E402
from anyv2v_amd.vae import AutoencoderKL, VAEConfig, init_random_weights_  # noqa: E402


def timed(fn, reps):
    """Median of ``reps`` event-timed calls (ms), after two warm-up calls."""
    fn()
    fn()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2], min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = "cuda"
    vae = init_random_weights_(AutoencoderKL(VAEConfig()), 0).to(dev)
    vae.enable_tiling()
    plan = vae.tiling_params().decode_plan(88, 160)
    m = vae.tile_frames                                    # images per stitch launch
    bases, rows = [], 0
    for th in plan.ay.sizes:
        bases.append([])
        for tw in plan.ax.sizes:
            bases[-1].append(rows)
            rows += m * th * tw
    raw = torch.randn(rows, 8, device=dev).half()
    out = torch.empty(m, 3, plan.H, plan.W, dtype=torch.float16, device=dev)
    src = torch.randn_like(out)
    launches = -(-args.frames // m)
    st = timed(lambda: ops.tile_blend(raw, 3, plan, bases, m, out=out), args.reps)
    cp = timed(lambda: out.copy_(src), args.reps)
    z = torch.randn(args.frames, 4, 88, 160, device=dev)
    whole = timed(lambda: vae.decode(z), 3)
    mb = out.numel() * 2 / 2 ** 20
    print(f"| what ({args.frames} frames of 704 x 1280, {m} frames per stitch launch, {launches} launches) | median ms | min | max |")
    print("|---|---|---|---|")
    print(f"| stitch launch, {m} frames: reads {rows * 16 / 2 ** 20:.0f} MiB of raw tiles, writes {mb:.0f} MiB | {st[0]:.3f} | {st[1]:.3f} | {st[2]:.3f} |")
    print(f"| device-to-device copy of the same {mb:.0f} MiB of output | {cp[0]:.3f} | {cp[1]:.3f} | {cp[2]:.3f} |")
    print(f"| stitch for all {args.frames} frames ({launches} x the launch) | {st[0] * launches:.3f} | | |")
    print(f"| whole tiled decode of {args.frames} frames (8 tile positions x {launches} passes + stitch) | {whole[0]:.1f} | {whole[1]:.1f} | {whole[2]:.1f} |")


if __name__ == "__main__":
    main()
