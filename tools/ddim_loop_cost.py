"""What a DDIM step costs against a DDPM step, and what fewer steps buy.  (1) The fused loop of BASELINE configuration 2
(35 400 nodes, 100 steps, the default two-stream schedule): codlad_ddim_loop (eta = 0) against codlad_sample_loop,
alternated, three repeats.  (2) structures/s of the fused DDIM loop at T = 100, 50, 25 and 10 respaced steps (the loop
alone: features are hoisted, decoding is not included).  HIP events on the caller's stream, warm-up first.  Prints the
numbers and one JSON line.  No trained denoiser exists here, so nothing is said about sample quality at fewer steps.

    python tools/ddim_loop_cost.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
wl = bench.Workload(dev, "cfg2")
wl.prepass()
n = wl.job.n_nodes
n_struct = len(wl.job.sample_struct)
ddim_coef = wl.tables.ddim_coefficients(eta=0.0)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def ddpm():
    wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False)


def ddim():
    wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False, coef=ddim_coef, kind="ddim")


ddpm(), ddim()                                                          # warm-up (features, step tables, streams)
torch.cuda.synchronize()
loops = {"ddpm": [], "ddim": []}
for _ in range(3):
    loops["ddpm"].append(event_ms(ddpm, 2))
    loops["ddim"].append(event_ms(ddim, 2))
ratios = [a / b for a, b in zip(loops["ddim"], loops["ddpm"])]
print(f"cfg2 loop ({n} nodes, {n_struct} structures, {bench.T_STEPS} steps): DDPM {['%.2f' % v for v in loops['ddpm']]} ms, "
      f"DDIM {['%.2f' % v for v in loops['ddim']]} ms, DDIM/DDPM {['%.4f' % r for r in ratios]}", flush=True)

per_T = {}
for T in (100, 50, 25, 10):
    tb = Tables(named_betas("linear", 1000), space_timesteps(1000, str(T)))
    coef = tb.ddim_coefficients(eta=0.0)
    noise = wl.noise[:T].contiguous()
    run = lambda: wl.den.sample(wl.job, wl.x_T, noise, tb, check=False, coef=coef, kind="ddim")   # noqa: E731
    run()
    torch.cuda.synchronize()
    ms = [event_ms(run, 2) for _ in range(3)]
    per_T[T] = {"loop_ms": ms, "structures_per_s": [n_struct / (m * 1e-3) for m in ms]}
    print(f"DDIM T={T:3d}: loop {['%.2f' % v for v in ms]} ms, {['%.1f' % s for s in per_T[T]['structures_per_s']]} "
          f"structures/s (loop only)", flush=True)
out = wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, coef=ddim_coef, kind="ddim")     # with the finiteness check
assert bool(torch.isfinite(out).all())
print(json.dumps({"tool": "ddim_loop_cost", "config": "cfg2", "n_nodes": n, "n_structures": n_struct, "steps": bench.T_STEPS,
                  "loop_ms": loops, "ddim_over_ddpm": ratios, "ddim_by_steps": per_T,
                  "device": torch.cuda.get_device_name(dev)}))
