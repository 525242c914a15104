"""What the automatic edit mask costs (profiles/auto_mask_cost.md): the new launches alone at the production shape (16 f x 64 x 64 latents),
``generate_edit_mask`` at 16 f x 512^2 with 10 noise draws and with the trajectory (one map), beside one PnP edit step (B = 3, every
injection on, HIP graphs) of the same build.  The default path (option off) is measured by ``bench.py`` against the parent commit, not here.

    python tools/auto_mask_cost.py [--calls 3] [--out FILE]
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
from anyv2v_amd.schedulers import DDIMScheduler  # noqa: E402
from anyv2v_amd.utils import LatentTrajectory  # noqa: E402

lines = []


def say(s):
    lines.append(s)
    print(s, flush=True)


def op_cost(device):
    F, H, W = 16, 64, 64
    n = F * H * W
    vtok = torch.randn(2 * n, 8, device=device).half()
    acc = torch.zeros(n, dtype=torch.float32, device=device)
    flag = torch.zeros(1, dtype=torch.int32, device=device)
    ms = bench.measure_kernel(lambda: ops.diff_map_accum(vtok, 4, F, H * W, acc, flag), iters=200, warm=20)
    say(f"op diff_map_accum [2 x 16 x 64 x 64, ld 8] (device flag, as in the graph): {ms * 1e3:7.1f} us per call")
    ops.diff_map_accum(vtok, 4, F, H * W, acc, True)
    out = (torch.empty(F, H, W, dtype=torch.float16, device=device), torch.empty(F, 8 * H, 8 * W, dtype=torch.bool, device=device))
    ms = bench.measure_kernel(lambda: ops.diff_map_finish(acc, F, H, W, 3.0, 0.5, out=out), iters=200, warm=20)
    say(f"op diff_map_finish 16 x 64 x 64 -> map + 16 x 512 x 512 pixel mask (two launches, 16-byte path): {ms * 1e3:7.1f} us per call")
    x0 = torch.randn(1, 4, F, H, W, device=device).half()
    sched = DDIMScheduler()
    gen = torch.Generator(device=device).manual_seed(0)
    ms = bench.measure_kernel(lambda: sched.add_noise(x0, sched.draw_noise(x0, gen), torch.tensor([481])), iters=100, warm=10)
    say(f"noising x_t in torch, outside the graph (draw_noise + add_noise): {ms * 1e3:7.1f} us per map")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
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
    _, _, F, h, w = lat.shape
    fwd = DDIMScheduler()
    fwd.set_timesteps(bench.STEPS_PER_STAGE)
    pipe.register_modules(scheduler=fwd)
    ts = [int(t) for t in fwd.timesteps]
    traj = LatentTrajectory()
    for t in ts:
        traj[t] = lat.clone()
    kw = dict(prompt_embeds=ehs[2:3], image_embeddings=ie[2:3], image_latents=il_all[2:3], ddim_inv_prompt_embeds=ehs[:1],
              ddim_inv_image_embeddings=ie[:1], ddim_inv_image_latents=il_all[:1], height=8 * h, width=8 * w, num_frames=F, target_fps=8,
              num_inference_steps=bench.STEPS_PER_STAGE)
    pnp_utils.clear_time(pipe)
    for name, src in (("N = 10 noise draws", dict(source_latents=lat, num_maps_per_mask=10, generator=torch.Generator(device=device).manual_seed(1))),
                      ("trajectory, one map", dict(ddim_inv_latents_path=traj))):
        for call in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pm = pipe.generate_edit_mask(**kw, **src)
            torch.cuda.synchronize()
            say(f"generate_edit_mask 16 f x 512^2, {name}, call {call}: {(time.perf_counter() - t0) * 1e3:9.2f} ms "
                f"(conditioning, warm-up forward, graph capture, replays, finish; mask covers {100 * float(pm.float().mean()):.1f} %)")

    # one PnP edit step of the same build: B = 3, every injection on, HIP graphs
    for reg in (pnp_utils.register_conv_injection, pnp_utils.register_spatial_attention_pnp, pnp_utils.register_temp_attention_pnp):
        reg(pipe, fwd.timesteps)
    s_pnp = lat.repeat(3, 1, 1, 1, 1).contiguous()
    cond3 = dict(encoder_hidden_states=ehs, fps=torch.tensor([8, 8, 8], device=device), image_latents=il_all, image_embeddings=ie)
    tt = torch.tensor(ts, dtype=torch.float32, device=device)[:, None].expand(-1, 3).contiguous()
    cf = fwd.coefficient_table(ts, device)
    eng = _StepEngine(pipe, s_pnp, cond3, b_unc=1, b_cond=2, guidance=9.0, dup_slots=[1], shared_stem=True)
    eng.drop_src_tail = True

    def step(i):
        j = i % len(ts)
        pnp_utils.register_time(pipe, ts[j])
        eng.step(tt[j], cf[j], key=("pnp",) + pnp_utils.injection_state(pipe))
    for i in range(2):
        step(i)
    for r in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(20):
            step(i)
        torch.cuda.synchronize()
        say(f"round {r}: PnP edit step (B = 3, injections on, graphs): {(time.perf_counter() - t0) / 20 * 1e3:8.3f} ms per step")
    pnp_utils.clear_time(pipe)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
