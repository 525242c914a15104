"""Cost of preparing a 1920 x 1080 clip to 512 x 512 (``fit="crop"``, lanczos) for profiles/prepare_cost.md: the two launches of
``ops.resample_u8`` (device events, warm-up, median of 20), the resize of the whole 910 x 512 frame for comparison, the host-to-device copy
of the source (pageable and pinned), and Pillow's ``resize(...).crop(...)`` of the same frames on this machine's CPU; the GPU result is
compared with Pillow's byte for byte.  Needs a GPU.

    python tools/prepare_cost.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyv2v_amd import ops, prepare  # noqa: E402


def med_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "prepare_cost.py measures on the GPU"
    res = {"device": torch.cuda.get_device_name(0), "cpus": os.cpu_count()}
    resize_to, window = prepare.fit_geometry((1920, 1080), (512, 512), "crop")
    wx, wy, ww, wh = window
    res["geometry"] = [resize_to, window]
    base = np.random.default_rng(0).integers(0, 256, (16, 1080, 1920, 3), dtype=np.uint8)
    for F in (16, 128):
        host = torch.from_numpy(np.concatenate([base] * (F // 16)))
        pinned = host.pin_memory()
        dev = host.cuda()
        r = {"resample_ms": med_ms(lambda: ops.resample_u8(dev, resize_to, "lanczos", window=window), 20)}
        _, _, rows, h, v = ops.resample_passes(1080, 1920, resize_to, "lanczos", None, window)
        r["passes"] = {"h": h is not None, "v": v is not None, "rows": rows, "ksize_h": h[0] if h else None, "ksize_v": v[0] if v else None}
        r["resample_whole_910x512_ms"] = med_ms(lambda: ops.resample_u8(dev, resize_to, "lanczos"), 10)
        r["h2d_pageable_ms"] = med_ms(lambda: host.cuda(), 5, warm=1)
        r["h2d_pinned_ms"] = med_ms(lambda: pinned.cuda(non_blocking=True), 5, warm=1)
        got = ops.resample_u8(dev, resize_to, "lanczos", window=window).cpu().numpy()
        imgs = [Image.fromarray(f) for f in host.numpy()]
        t = []
        for _ in range(3 if F == 16 else 1):
            t0 = time.perf_counter()
            want = [np.asarray(im.resize(resize_to, resample=Image.Resampling.LANCZOS).crop((wx, wy, wx + ww, wy + wh))) for im in imgs]
            t.append((time.perf_counter() - t0) * 1e3)
        r["pillow_ms"] = [statistics.median(t), min(t), max(t)]
        r["equal_to_pillow"] = bool(np.array_equal(got, np.stack(want)))
        r["bytes_in"], r["bytes_out"] = int(host.numel()), int(got.size)
        res[f"F{F}"] = r
        del dev, pinned, host
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
