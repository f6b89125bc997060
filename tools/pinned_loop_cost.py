"""What residue pinning costs.  (1) The fused DDPM loop of BASELINE configuration 2 (35 400 nodes, 100 steps, the default
two-stream schedule) unpinned against the same loop with 25 % of the residues pinned (codlad_sample_loop_pinned: one
extra 13-byte read per node and step in final_kernel).  (2) The per-step update of the same job: codlad_ddpm_update
(the per-step path without hooks) against the split step codlad_ddpm_pred_xstart + a trivial Python denoised_fn +
codlad_ddpm_posterior_step; one denoiser forward for scale.  HIP events on the caller's stream, warm-up first, the two
variants alternated, three repeats.  Prints the numbers and one JSON line.

    python tools/pinned_loop_cost.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from codlad_amd.engine import Denoiser  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
wl = bench.Workload(dev, "cfg2")
wl.prepass()
n = wl.job.n_nodes
g = torch.Generator(device=dev).manual_seed(5)
pin = (torch.randn(n, 3, generator=g, device=dev), torch.arange(n, device=dev) % 4 == 0)   # every fourth residue


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def plain():
    wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False)


def pinned():
    wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False, pin=pin)


plain(), pinned()                                                       # warm-up (features, step tables, streams)
torch.cuda.synchronize()
loops = {"unpinned": [], "pinned": []}
for _ in range(3):
    loops["unpinned"].append(event_ms(plain, 2))
    loops["pinned"].append(event_ms(pinned, 2))
ratios = [p / u for p, u in zip(loops["pinned"], loops["unpinned"])]
print(f"cfg2 loop ({n} nodes, {bench.T_STEPS} steps, 25 % pinned): unpinned {['%.2f' % v for v in loops['unpinned']]} ms, "
      f"pinned {['%.2f' % v for v in loops['pinned']]} ms, pinned/unpinned {['%.4f' % r for r in ratios]}", flush=True)

# per-step update of the same node count, model output of a real forward
i = bench.T_STEPS // 2
x = wl.x_T.clone()
out = wl.den.forward(wl.job, x, wl.tables.timestep_map[i])
eps = wl.noise[0]
coef = wl.tables.step_coefficients()[i]
identity = lambda v: v                                                  # noqa: E731  (a trivial denoised_fn)


def update():
    wl.den.ddpm_update(x, out, eps, wl.tables, i)


def split():
    raw = Denoiser.ddpm_pred_xstart(x, out, coef)
    Denoiser.ddpm_posterior_step(x, identity(raw), out, eps, coef)


def forward():
    wl.den.forward(wl.job, x, wl.tables.timestep_map[i], check=False)


update(), split(), forward()
torch.cuda.synchronize()
steps = {"ddpm_update": [], "split": [], "forward": []}
for _ in range(3):
    steps["ddpm_update"].append(event_ms(update, 50))
    steps["split"].append(event_ms(split, 50))
    steps["forward"].append(event_ms(forward, 5))
print(f"per-step update, {n} nodes: codlad_ddpm_update {['%.1f' % (v * 1e3) for v in steps['ddpm_update']]} us, "
      f"split step with an identity denoised_fn {['%.1f' % (v * 1e3) for v in steps['split']]} us "
      f"(one denoiser forward: {['%.2f' % v for v in steps['forward']]} ms)", flush=True)
print(json.dumps({"tool": "pinned_loop_cost", "config": "cfg2", "n_nodes": n, "steps": bench.T_STEPS,
                  "pinned_fraction": float(pin[1].float().mean()), "loop_ms": loops, "pinned_over_unpinned": ratios,
                  "per_step_ms": steps, "device": torch.cuda.get_device_name(dev)}))
