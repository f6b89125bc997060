"""What a DPM-Solver++(2M) step costs against a DDIM step, and what 20 log-SNR steps cost against 100 DDPM steps.
(1) At 400 PED-shaped structures (BASELINE configuration 2, 35 400 nodes, the default two-stream schedule) and at one
structure of 87 residues: the fused loops codlad_dpm_loop (order 2) and codlad_ddim_loop (eta 0) over the same "logsnr20"
tables, alternated, REPEATS repeats of each; microseconds per step, and the DDIM loop's own run-to-run spread, which is the
margin a difference has to exceed to be one.  The expectation: a DPM step is a DDIM step plus one 12-byte read per node.
(2) structures/s of the loop alone (features hoisted, decoding not included) for DPM-Solver++ at 20 log-SNR steps next to
the 100-step DDPM loop.  HIP events on the caller's stream, warm-up first.  Prints the numbers and one JSON line.
A cost figure: no trained denoiser exists here, so nothing is said about sample quality at 20 steps.

    python tools/dpm_loop_cost.py
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from codlad_amd import synth  # noqa: E402
from codlad_amd.diffusion_and_flow.schedule import Tables, logsnr_timesteps, named_betas  # noqa: E402

REPEATS = 7
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
betas = named_betas("linear", 1000)
tb = Tables(betas, logsnr_timesteps(betas, 20))
T = tb.num_timesteps
dpm_coef, ddim_coef = tb.dpm_solver_coefficients(2), tb.ddim_coefficients(eta=0.0)


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(label, den, job, x_T, noise, reps):
    """-> per-step microseconds of both loops, REPEATS alternated windows of `reps` loops each."""
    dpm = lambda: den.sample(job, x_T, None, tb, check=False, coef=dpm_coef, kind="dpmpp")            # noqa: E731
    ddim = lambda: den.sample(job, x_T, noise, tb, check=False, coef=ddim_coef, kind="ddim")          # noqa: E731
    for _ in range(2):                                                   # warm-up: features, step tables, streams
        dpm(), ddim()
    torch.cuda.synchronize()
    us = {"ddim": [], "dpm": []}
    for _ in range(REPEATS):
        us["ddim"].append(event_ms(ddim, reps) * 1e3 / T)
        us["dpm"].append(event_ms(dpm, reps) * 1e3 / T)
    med = {k: statistics.median(v) for k, v in us.items()}
    spread = (max(us["ddim"]) - min(us["ddim"])) / med["ddim"]
    diff = med["dpm"] / med["ddim"] - 1.0
    print(f"{label}: {job.n_nodes} nodes, {T} steps, {REPEATS} x {reps} loops each, us per step", flush=True)
    for k in ("ddim", "dpm"):
        print(f"  {k:4s} median {med[k]:9.2f}  min {min(us[k]):9.2f}  max {max(us[k]):9.2f}  all {['%.2f' % v for v in us[k]]}")
    print(f"  DPM / DDIM - 1 = {diff:+.4%} (medians); the DDIM loop's own spread (max - min) / median = {spread:.4%}: "
          f"{'within' if abs(diff) <= spread else 'OUTSIDE'} it", flush=True)
    out = den.sample(job, x_T, None, tb, coef=dpm_coef, kind="dpmpp")     # with the finiteness check
    assert bool(torch.isfinite(out).all())
    return {"n_nodes": job.n_nodes, "us_per_step": us, "median": med, "dpm_over_ddim_minus_1": diff, "ddim_spread": spread}


wl = bench.Workload(dev, "cfg2")
wl.prepass()
n_struct = len(wl.job.sample_struct)
res = {"cfg2": compare("400 PED-shaped structures", wl.den, wl.job, wl.x_T, wl.noise[:T].contiguous(), 2)}

prot = synth.make_protein(87, 1001, n_frames=1)
st = wl.den.prepare_structures([torch.from_numpy(prot["xyz_full"])[0, 1:-1]], [torch.from_numpy(prot["z_full"])[1:-1]])
job87 = wl.den.make_job(st, [0])
g = torch.Generator(device=dev).manual_seed(7)
res["L87"] = compare("one structure of 87 residues", wl.den, job87, torch.randn(87, 3, device=dev, generator=g),
                     torch.randn(T, 87, 3, device=dev, generator=g), 20)

# the loop alone at the headline size: DPM-Solver++ over 20 log-SNR steps next to the 100-step DDPM loop
ddpm = lambda: wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False)                          # noqa: E731
dpm = lambda: wl.den.sample(wl.job, wl.x_T, None, tb, check=False, coef=dpm_coef, kind="dpmpp")         # noqa: E731
ddpm(), dpm()
torch.cuda.synchronize()
loop = {"ddpm100": [], "dpm20": []}
for _ in range(5):
    loop["ddpm100"].append(event_ms(ddpm, 1))
    loop["dpm20"].append(event_ms(dpm, 4))
rate = {k: n_struct / (statistics.median(v) * 1e-3) for k, v in loop.items()}
print(f"loop alone, {n_struct} structures: DDPM {bench.T_STEPS} steps {['%.2f' % v for v in loop['ddpm100']]} ms = "
      f"{rate['ddpm100']:.1f} structures/s; DPM-Solver++ {T} log-SNR steps {['%.2f' % v for v in loop['dpm20']]} ms = "
      f"{rate['dpm20']:.1f} structures/s ({rate['dpm20'] / rate['ddpm100']:.2f} x).  A cost figure, not a quality claim.", flush=True)
print(json.dumps({"tool": "dpm_loop_cost", "steps": T, "repeats": REPEATS, "per_step": res, "loop_ms": loop,
                  "structures_per_s": rate, "n_structures": n_struct, "device": torch.cuda.get_device_name(dev)}))
