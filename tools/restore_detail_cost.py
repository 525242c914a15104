"""Cost of the detail-preserving way back for profiles/restore_detail_cost.md: a 16-frame 512 x 512 edit to its 1920 x 1080 source
(``fit="crop"``, lanczos), ``ops.restore_u8`` and ``ops.restore_detail_u8`` (the gate given) timed interleaved in one process -- every round
times each variant once, 10 calls between two device events, so that a drift of the box's clocks lands on all of them alike --, the two
launches of ``ops.detail_gate_u8`` on their own, with and without alpha; median (min - max) of 30 rounds after 5 warm-up rounds, in
microseconds per clip.  At the same size it checks that a gate of 0 gives ``restore_u8`` and that an unchanged edit gives the source.
Needs a GPU.

    python tools/restore_detail_cost.py [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyv2v_amd import ops, prepare  # noqa: E402

CALLS, ROUNDS, WARM = 10, 30, 5


def interleaved_us(variants):
    """name -> callable; -> name -> (median, min, max) microseconds per call, the variants alternated round by round."""
    times = {name: [] for name in variants}
    for r in range(WARM + ROUNDS):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(CALLS):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r >= WARM:
                times[name].append(a.elapsed_time(b) * 1000.0 / CALLS)
    return {name: [round(v, 2) for v in (statistics.median(t), min(t), max(t))] for name, t in times.items()}


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "restore_detail_cost.py measures on the GPU"
    F, h, w, sh, sw = 16, 512, 512, 1080, 1920
    dest, box = prepare.restore_geometry((sw, sh), (w, h), "crop")
    res = {"device": torch.cuda.get_device_name(0), "geometry": [list(dest), list(box)], "calls_per_sample": CALLS, "rounds": ROUNDS}
    rng = np.random.default_rng(0)
    S = torch.from_numpy(rng.integers(0, 256, (F, sh, sw, 3), dtype=np.uint8)).cuda()
    P = prepare.prepare_frames(S, h, w, "crop", device="cuda")
    # an edit that keeps the left half within +-3 of the prepared source and replaces the right half: the gate holds 0, 255 and the ramp
    E = (P.to(torch.int16) + torch.from_numpy(rng.integers(-3, 4, (F, h, w, 3), dtype=np.int16)).cuda()).clamp(0, 255).to(torch.uint8)
    E[:, :, w // 2:] = torch.from_numpy(rng.integers(0, 256, (F, h, w - w // 2, 3), dtype=np.uint8)).cuda()
    E = E.contiguous()
    A = torch.from_numpy(rng.integers(0, 256, (F, h, w), dtype=np.uint8)).cuda()
    G = ops.detail_gate_u8(E, P)
    res["gate_values"] = {"zero": int((G == 0).sum()), "full": int((G == 255).sum()), "between": int(((G > 0) & (G < 255)).sum())}
    res["us"] = interleaved_us({
        "restore_u8": lambda: ops.restore_u8(E, S, dest, box, "lanczos"),
        "restore_detail_u8": lambda: ops.restore_detail_u8(E, P, G, S, dest, box, "lanczos"),
        "restore_u8_alpha": lambda: ops.restore_u8(E, S, dest, box, "lanczos", A),
        "restore_detail_u8_alpha": lambda: ops.restore_detail_u8(E, P, G, S, dest, box, "lanczos", A),
        "detail_gate_u8": lambda: ops.detail_gate_u8(E, P),
        "detail_gate_u8_radius16": lambda: ops.detail_gate_u8(E, P, 8, 32, 16),
        "device_copy": lambda: torch.empty_like(S).copy_(S),
    })
    us = res["us"]
    res["ratio_detail_to_plain"] = round(us["restore_detail_u8"][0] / us["restore_u8"][0], 3)
    res["ratio_detail_to_plain_alpha"] = round(us["restore_detail_u8_alpha"][0] / us["restore_u8_alpha"][0], 3)
    res["ratio_gate_and_detail_to_plain"] = round((us["restore_detail_u8"][0] + us["detail_gate_u8"][0]) / us["restore_u8"][0], 3)
    zero = torch.zeros((1, h, w), dtype=torch.uint8, device="cuda")
    res["gate_zero_equals_restore_u8"] = bool(torch.equal(ops.restore_detail_u8(E, P, zero, S, dest, box, "lanczos", A),
                                                          ops.restore_u8(E, S, dest, box, "lanczos", A)))
    res["unchanged_edit_equals_source"] = bool(torch.equal(ops.restore_detail_u8(P, P, ops.detail_gate_u8(P, P), S, dest, box, "lanczos", A), S))
    plain, detail = ops.restore_u8(E, S, dest, box, "lanczos"), ops.restore_detail_u8(E, P, G, S, dest, box, "lanczos")
    inside = (slice(None), slice(dest[1], dest[3]), slice(dest[0], dest[0] + (dest[2] - dest[0]) // 2 - 8))   # the left half, the gate open
    err = lambda x: round(float((x[inside].float() - S[inside].float()).abs().mean()), 3)
    res["mean_abs_error_to_source_left_half"] = {"restore_u8": err(plain), "restore_detail_u8": err(detail)}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
