"""What the pixel-space composite of a masked edit costs (profiles/composite_cost.md): the new ops alone at 16 f x 512 x 512 with
``feather_px`` 0, 4 and 16, and the whole post-decode path -- decode output on the device -> bytes on the host -- with the composite beside
the path without it (``vae.to_pil``'s quantisation, which this feature does not touch), alternating in one process.  The default path
(option off) is measured by ``bench.py`` against the parent commit, not here.

    python tools/composite_cost.py [--rounds 5] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from anyv2v_amd import ops  # noqa: E402
from anyv2v_amd.encoders import SyntheticVAE  # noqa: E402
from anyv2v_amd.pipeline import I2VGenXLPipeline  # noqa: E402

lines = []
F, H, W = 16, 512, 512


def say(s):
    lines.append(s)
    print(s, flush=True)


def operands(device):
    g = torch.Generator().manual_seed(0)
    video = (torch.rand(1, 3, F, H, W, generator=g) * 2.2 - 1.1).half().to(device)
    source = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).to(device)
    mask = torch.zeros(F, H, W, dtype=torch.bool)
    for f in range(F):                      # a box that drifts over the clip: a per-frame mask, about a fifth of the frame
        mask[f, 96 + 4 * f: 320 + 4 * f, 128 + 8 * f: 352 + 8 * f] = True
    return video, source, mask.to(device)


def op_cost(video, source, mask):
    lm = ops.latent_mask(mask.half(), 0, 0.0)
    alpha = None
    for sigma in (0.0, 4.0, 16.0):
        out = torch.empty(F, H, W, dtype=torch.float32, device=video.device)
        ms = bench.measure_kernel(lambda: ops.pixel_alpha(lm, 4, sigma, out=out), iters=50, warm=5)
        n = 2 if sigma == 0 else 4
        say(f"op pixel_alpha 16 x 64 x 64 -> 16 x 512 x 512, grow_px 4, feather_px {sigma:4.1f} (R {len(ops.gaussian_taps(sigma, 48)) // 2:2d}; "
            f"{n} launches + the workspace allocation): {ms * 1e3:8.1f} us per call")
        alpha = out if sigma == 4.0 else alpha
    rec = torch.empty(256, 16, dtype=torch.int64, device=video.device)
    ms = bench.measure_kernel(lambda: ops.composite_stats(video, source, alpha, out=rec), iters=50, warm=5)
    moved = (video.numel() * 2 + source.numel() + alpha.numel() * 4) / 1e6
    say(f"op composite_stats (fixed 256 x 256 grid; reads up to {moved:.1f} MB): {ms * 1e3:8.1f} us per call")
    out = torch.empty_like(source)
    ms = bench.measure_kernel(lambda: ops.composite(video, source, alpha, out=out), iters=50, warm=5)
    moved += source.numel() / 1e6
    say(f"op composite, no colour match (4-pixel path; {video.numel() * 2 / 1e6:.1f} MB video + {source.numel() / 1e6:.1f} MB source + "
        f"{alpha.numel() * 4 / 1e6:.1f} MB alpha + {source.numel() / 1e6:.1f} MB out = {moved:.1f} MB): {ms * 1e3:8.1f} us per call "
        f"({moved / ms / 1e3:.2f} TB/s)")
    ms = bench.measure_kernel(lambda: ops.composite(video, source, alpha, match_color=True, out=out), iters=50, warm=5)
    say(f"op composite with the colour match (statistics + paste, two launches): {ms * 1e3:8.1f} us per call")


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def path_cost(video, source, mask, rounds):
    pipe = I2VGenXLPipeline(unet=None, scheduler=None)
    quant = SyntheticVAE().to_pil.__func__     # the adapters share it: ((v + 1) * 127.5).round().clamp(0, 255).to(uint8).cpu() + PIL images
    src_host = source.cpu()
    paths = {
        "without the composite (to_pil: quantise on the device, bytes to the host, PIL images)": lambda: quant(None, video),
        "composite, hard (grow_px 0, feather_px 0), source frames already on the device": lambda: pipe.composite_over_source(video, source, mask).cpu(),
        "composite, grow_px 4, feather_px 4, source frames from the host (uint8 tensor)": lambda: pipe.composite_over_source(video, src_host, mask, grow_px=4, feather_px=4.0).cpu(),
        "composite, grow_px 4, feather_px 16, colour match, source frames from the host": lambda: pipe.composite_over_source(video, src_host, mask, grow_px=4, feather_px=16.0, match_color=True).cpu(),
    }
    times = {k: [] for k in paths}
    for r in range(rounds + 1):            # round 0 warms up; the paths alternate within every round
        for k, fn in paths.items():
            t = wall(fn)
            if r:
                times[k].append(t)
    for k, ts in times.items():
        say(f"post-decode path, {k}: " + ", ".join(f"{t:.2f}" for t in ts) + f" ms (median {sorted(ts)[len(ts) // 2]:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.cuda.set_device(0)
    video, source, mask = operands(torch.device("cuda", 0))
    for _ in range(2):   # the first pass doubles as the clock warm-up
        lines.clear()
        op_cost(video, source, mask)
    path_cost(video, source, mask, args.rounds)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
