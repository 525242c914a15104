"""What tracking a first-frame edit mask costs (profiles/mask_track_cost.md): every launch of ``track.hip`` alone at 16 f x 512 x 512, HIP
events on the launching stream -- the block match at radius 16 and 32 on a moving texture -- and ``propagate_edit_mask`` as a whole (host
frames in, mask on the device).  The edit step and the whole clip it stands beside come from ``bench.py`` in the same session.

    python tools/track_cost.py [--out FILE]
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
from anyv2v_amd.pipeline import I2VGenXLPipeline  # noqa: E402

lines = []
F, H, W = 16, 512, 512


def say(s):
    lines.append(s)
    print(s, flush=True)


def operands():
    """A blurred random texture drifting by (2, -3) pixels per frame, its right half by (1, -1): a field with two motions."""
    g = torch.Generator().manual_seed(0)
    big = torch.randint(0, 256, (3, H + 128, W + 128), generator=g).float()
    big = torch.nn.functional.avg_pool2d(big[None], 5, stride=1, padding=2)[0].round().to(torch.uint8)
    frames = []
    for k in range(F):
        a = big[:, 64 + 2 * k: 64 + 2 * k + H, 64 - 3 * k: 64 - 3 * k + W].clone()
        a[:, :, W // 2:] = big[:, 64 + k: 64 + k + H, 64 - k + W // 2: 64 - k + W]
        frames.append(a.permute(1, 2, 0))
    frames = torch.stack(frames).contiguous()
    edited = frames[0].clone()
    edited[160:352, 128:320] = 255 - edited[160:352, 128:320]
    return frames, edited


def op_cost(frames, edited):
    dev = frames.cuda()
    ms = bench.measure_kernel(lambda: ops.luma_u8(dev), iters=50, warm=5)
    say(f"op luma_u8 16 x 512 x 512 ({dev.numel() / 1e6:.1f} MB in, {dev.numel() / 3e6:.1f} MB out): {ms * 1e3:8.1f} us per call")
    y = ops.luma_u8(dev)
    flow = None
    for R in (16, 32):
        ms = bench.measure_kernel(lambda: ops.block_match(y, R), iters=20, warm=3)
        sads = (F - 1) * (H // 8) * (W // 8) * (2 * R + 1) ** 2 * 256
        say(f"op block_match radius {R:2d} ({(F - 1) * (H // 8) * (W // 8)} cells x {(2 * R + 1) ** 2} candidates x 256 pixels = {sads:.2e} "
            f"absolute differences): {ms * 1e3:8.1f} us per call ({sads / ms / 1e9:.2f} T differences / s)")
        flow = ops.block_match(y, R) if R == 16 else flow
    vecs, counts = flow[1:].reshape(-1, 2).cpu().unique(dim=0, return_counts=True)
    top = counts.argsort(descending=True)[:3]
    say("   field at radius 16, most frequent (dy, dx): " + ", ".join(f"{tuple(vecs[i].tolist())} x {int(counts[i])}" for i in top))
    ms = bench.measure_kernel(lambda: ops.flow_median(flow), iters=50, warm=5)
    say(f"op flow_median 16 x 64 x 64 x 2: {ms * 1e3:8.1f} us per call")
    med = ops.flow_median(flow)
    m0 = ops.first_frame_mask(dev[0].contiguous(), edited.cuda())
    ms = bench.measure_kernel(lambda: ops.first_frame_mask(dev[0], edited.cuda()), iters=50, warm=5)
    say(f"op first_frame_mask 512 x 512 (with the edited frame's upload): {ms * 1e3:8.1f} us per call; {int(m0.sum())} pixels set")
    ms = bench.measure_kernel(lambda: ops.mask_propagate(m0[0], med), iters=50, warm=5)
    say(f"op mask_propagate 16 x 512 x 512 (chains of up to 15 steps): {ms * 1e3:8.1f} us per call")
    return m0


def whole(frames, m0):
    pipe = I2VGenXLPipeline(unet=None, scheduler=None)
    pipe._device = torch.device("cuda", 0)
    for name, src in (("uint8 tensor on the host", frames), ("uint8 tensor on the device", frames.cuda())):
        ts = []
        for r in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.propagate_edit_mask(src, m0)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        say(f"propagate_edit_mask, radius 16, median, frames a {name}: " + ", ".join(f"{t:.2f}" for t in ts[1:])
            + f" ms wall (median {sorted(ts[1:])[2]:.2f}; the first call {ts[0]:.2f})")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.cuda.set_device(0)
    frames, edited = operands()
    for _ in range(2):   # the first pass doubles as the clock warm-up
        lines.clear()
        m0 = op_cost(frames, edited)
    whole(frames, m0)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
