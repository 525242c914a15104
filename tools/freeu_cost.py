"""What FreeU costs (profiles/freeu_cost.md): the op alone at the two production shapes -- 48 images (3 branches x 16 frames) at 8 x 8
and at 16 x 16, 1280 + 1280 channels -- and the benchmark's serial step pair (inversion step B = 1 + PnP edit step B = 3 with every
injection on, 16 f x 64 x 64 latents, HIP graphs) with FreeU on against off, the two settings alternating in one process.
Traffic model of the op: one read and one write of hidden, two reads and one write of skip.

    python tools/freeu_cost.py [--pairs 30] [--rounds 3] [--out FILE]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from anyv2v_amd import ops, pnp_utils  # noqa: E402
from anyv2v_amd.pipeline import I2VGenXLPipeline, _StepEngine  # noqa: E402
from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler  # noqa: E402

FREEU = (0.9, 0.2, 1.2, 1.4)
lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def op_cost(n_img, H, W, C):
    rows = n_img * H * W
    hidden = (1.5 * torch.randn(rows, C, device="cuda") + 2).half()
    skip = (1.5 * torch.randn(rows, C, device="cuda") + 2).half()
    out = (torch.empty_like(hidden), torch.empty_like(skip))
    ms = bench.measure_kernel(lambda: ops.freeu(hidden, skip, n_img, H, W, 1.4, 0.2, out=out), iters=200, warm=20)
    moved = 5 * rows * C * 2
    say(f"op {n_img} images {H}x{W} C {C}+{C}: {ms * 1e3:7.1f} us per call, {moved / 1e6:6.1f} MB moved, {moved / ms / 1e9:5.2f} TB/s")
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    torch.set_grad_enabled(False)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    for _ in range(2):   # the first pass doubles as the clock warm-up
        lines.clear()
        ms8, ms16 = op_cost(48, 8, 8, 1280), op_cost(48, 16, 16, 1280)
    say(f"per three-branch UNet evaluation (3 calls per level): {3 * (ms8 + ms16) * 1e3:.1f} us")

    pipe = I2VGenXLPipeline.from_pretrained("ali-vilab/i2vgen-xl", torch_dtype=torch.float16, variant="fp16", random_init_seed=0)
    pipe.to(device)
    lat, ehs, ie, il_all = bench.synthetic_clip(device, 8888)
    S = bench.STEPS_PER_STAGE
    inv, fwd = DDIMInverseScheduler(), DDIMScheduler()
    inv.set_timesteps(S)
    fwd.set_timesteps(S)
    ts_inv, ts_pnp = [int(t) for t in inv.timesteps], [int(t) for t in fwd.timesteps]
    for reg in (pnp_utils.register_conv_injection, pnp_utils.register_spatial_attention_pnp, pnp_utils.register_temp_attention_pnp):
        reg(pipe, fwd.timesteps)
    fps1, fps3 = torch.tensor([8], device=device), torch.tensor([8, 8, 8], device=device)
    cond1 = dict(encoder_hidden_states=ehs[:1].contiguous(), fps=fps1, image_latents=il_all[:1].contiguous(), image_embeddings=ie[:1].contiguous())
    cond3 = dict(encoder_hidden_states=ehs, fps=fps3, image_latents=il_all, image_embeddings=ie)
    tt_inv = torch.tensor(ts_inv, dtype=torch.float32, device=device)[:, None].contiguous()
    tt_pnp = torch.tensor(ts_pnp, dtype=torch.float32, device=device)[:, None].expand(-1, 3).contiguous()
    cf_inv, cf_pnp = inv.coefficient_table(ts_inv, device), fwd.coefficient_table(ts_pnp, device)

    def make_pair(freeu):
        """The benchmark's serial pair on engines of their own, captured under this FreeU setting."""
        if freeu:
            pipe.enable_freeu(*FREEU)
        else:
            pipe.disable_freeu()
        s_inv, s_pnp = lat.clone(), lat.repeat(3, 1, 1, 1, 1).contiguous()
        traj = torch.zeros(S, *lat.shape[1:], dtype=torch.float16, device=device)
        pnp_utils.clear_time(pipe)
        e_inv = _StepEngine(pipe, s_inv, cond1, b_unc=-1, b_cond=0, guidance=1.0, dup_slots=[])
        e_pnp = _StepEngine(pipe.sibling(ws_slot=1), s_pnp, cond3, b_unc=1, b_cond=2, guidance=9.0, dup_slots=[1], shared_stem=True)
        e_pnp.drop_src_tail = True

        def pair(i):
            j = i % S
            pnp_utils.clear_time(pipe)
            e_inv.step(tt_inv[j], cf_inv[j], key=("inv",))
            traj[j].copy_(s_inv[0])
            s_pnp[0].copy_(traj[j])
            pnp_utils.register_time(pipe, ts_pnp[j])
            e_pnp.step(tt_pnp[j], cf_pnp[j], key=("pnp",) + pnp_utils.injection_state(pipe))
        for i in range(2):   # warm-up + graph capture under this setting (the graphs hold the setting; replays ignore the UNet's)
            pair(i)
        torch.cuda.synchronize()
        return pair, s_pnp

    pairs = {"off": make_pair(False), "on": make_pair(True)}
    pipe.disable_freeu()
    times = {"off": [], "on": []}
    for r in range(args.rounds):
        for name in ("off", "on"):
            pair, _ = pairs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.pairs):
                pair(i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / args.pairs * 1e3)
            say(f"round {r} FreeU {name:3s}: {times[name][-1]:8.3f} ms per serial step pair ({args.pairs} pairs)")
    off, on = min(times["off"]), min(times["on"])
    say(f"serial step pair, best of {args.rounds}: off {off:.3f} ms, on {on:.3f} ms, difference {on - off:+.3f} ms = {100 * (on - off) / off:+.2f} %"
        f" (spread of the off rounds: {max(times['off']) - off:.3f} ms)")
    finite = all(bool(torch.isfinite(p[1].float()).all()) for p in pairs.values())
    say(f"latents finite: {finite}; FreeU on differs from off: {not torch.equal(pairs['on'][1], pairs['off'][1])}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
