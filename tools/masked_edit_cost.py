"""What the masked edit costs (profiles/masked_edit_cost.md): the blend launch and the mask-preparation launches alone at the production
shape (16 f x 64 x 64 latents, a 512 x 512 pixel mask), and the benchmark's serial step pair (inversion step B = 1 + PnP edit step B = 3
with every injection on, HIP graphs) with a mask on the edit engine against the same tree with it off, the two settings alternating in
one process.  "On" includes what happens outside the graph: the copy of the step's partner latent into the engine's static buffer.
The "off" engine is the default one: the same launches as before the option existed.

    python tools/masked_edit_cost.py [--pairs 30] [--rounds 3] [--out FILE]
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

lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def op_cost(device):
    F, H, W = 16, 64, 64
    x, s = torch.randn(1, 4, F, H, W, device=device).half(), torch.randn(1, 4, F, H, W, device=device).half()
    out = torch.empty_like(x)
    pix = (torch.rand(F, 8 * H, 8 * W, device=device) > 0.5).half()
    for Fm in (1, F):
        lm = ops.latent_mask(pix[:Fm].contiguous(), 2, 1.5)
        ms = bench.measure_kernel(lambda: ops.masked_blend(x, s, lm, out=out), iters=200, warm=20)
        say(f"op masked_blend [1,4,16,64,64], mask frames {Fm:2d}: {ms * 1e3:7.1f} us per call")
    ms = bench.measure_kernel(lambda: ops.masked_blend(x, s, lm, out=x), iters=200, warm=20)
    say(f"op masked_blend in place (as the step engine calls it): {ms * 1e3:7.1f} us per call")
    ms = bench.measure_kernel(lambda: s.copy_(x), iters=200, warm=20)
    say(f"copy of the partner latent into the static buffer (outside the graph): {ms * 1e3:7.1f} us per call")
    # mask preparation, once per clip: the calls differ by one launch each (pool; + grow; + feather), allocation of the result and of the
    # workspace included
    for Fm in (1, F):
        m = pix[:Fm].contiguous()
        prev = 0.0
        for name, grow, sigma in (("pool", 0, 0.0), ("pool + grow 2", 2, 0.0), ("pool + grow 2 + feather 1.5", 2, 1.5)):
            ms = bench.measure_kernel(lambda: ops.latent_mask(m, grow, sigma), iters=100, warm=10)
            say(f"op latent_mask {Fm:2d} x 512 x 512, {name}: {ms * 1e3:7.1f} us per call (+{(ms - prev) * 1e3:6.1f} us for the last launch)")
            prev = ms
        ms = bench.measure_kernel(lambda: ops.latent_mask(m, 8, 8.0), iters=50, warm=5)
        say(f"op latent_mask {Fm:2d} x 512 x 512, the largest window and radius (grow 8, feather 8: 17 x 17 maximum, 49 x 49 taps): {ms * 1e3:7.1f} us per call")


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
        op_cost(device)

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
    _, _, F, h, w = lat.shape
    pix = torch.zeros(1, 8 * h, 8 * w, device=device).half()
    pix[:, :, : 4 * w] = 1.0                                    # the left half is edited
    lat_mask = ops.latent_mask(pix, 2, 1.5)

    def make_pair(on):
        """The benchmark's serial pair on engines of their own; the edit engine with or without the mask."""
        s_inv, s_pnp = lat.clone(), lat.repeat(3, 1, 1, 1, 1).contiguous()
        traj = torch.zeros(S, *lat.shape[1:], dtype=torch.float16, device=device)
        pnp_utils.clear_time(pipe)
        sib = pipe.sibling(ws_slot=1)
        sib.scheduler = fwd
        opts = dict(blend=(torch.zeros_like(lat), lat_mask)) if on else {}
        e_inv = _StepEngine(pipe, s_inv, cond1, b_unc=-1, b_cond=0, guidance=1.0, dup_slots=[])
        e_pnp = _StepEngine(sib, s_pnp, cond3, b_unc=1, b_cond=2, guidance=9.0, dup_slots=[1], shared_stem=True, **opts)
        e_pnp.drop_src_tail = True

        def pair(i):
            j = i % S
            pnp_utils.clear_time(pipe)
            e_inv.step(tt_inv[j], cf_inv[j], key=("inv",))
            traj[j].copy_(s_inv[0])
            s_pnp[0].copy_(traj[j])
            pnp_utils.register_time(pipe, ts_pnp[j])
            extra = dict(partner=traj[j][None]) if on else {}
            e_pnp.step(tt_pnp[j], cf_pnp[j], key=("pnp",) + pnp_utils.injection_state(pipe), **extra)
        for i in range(2):   # warm-up + graph capture
            pair(i)
        torch.cuda.synchronize()
        return pair, s_pnp

    pairs = {"off": make_pair(False), "on": make_pair(True)}
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
            say(f"round {r} mask {name:3s}: {times[name][-1]:8.3f} ms per serial step pair ({args.pairs} pairs)")
    off, on = min(times["off"]), min(times["on"])
    say(f"serial step pair, best of {args.rounds}: off {off:.3f} ms, on {on:.3f} ms, difference {on - off:+.3f} ms = {100 * (on - off) / off:+.2f} %"
        f" (spread of the off rounds: {max(times['off']) - off:.3f} ms)")
    finite = all(bool(torch.isfinite(p[1].float()).all()) for p in pairs.values())
    say(f"latents finite: {finite}; mask on differs from off: {not torch.equal(pairs['on'][1], pairs['off'][1])}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
