"""What scoring a checkpoint costs against sampling from it.  (1) The fused loops of BASELINE configuration 2 (35 400 nodes,
400 structures, 100 steps, the default two-stream schedule), built as bench.py builds it: Denoiser.bpd (codlad_bpd_loop)
against Denoiser.sample (codlad_sample_loop), alternated, three repeats.  (2) The per-sample-timestep path: training-loss
terms of one 96-frame batch (L = 87) with 96 distinct timesteps out of 1000 (96 ragged one-sample sub-jobs on two streams)
against the same batch at one shared timestep.  HIP events on the caller's stream, warm-up first.  Prints the numbers and
one JSON line.

    python tools/loss_eval_timing.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from codlad_amd import synth  # noqa: E402
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps  # noqa: E402

torch.set_grad_enabled(False)
dev = torch.device("cuda", 0)
wl = bench.Workload(dev, "cfg2")
wl.prepass()
n = wl.job.n_nodes
n_struct = len(wl.job.sample_struct)
x0 = wl.x_T                                                   # any latents do: the cost does not depend on the values


def event_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def sample():
    wl.den.sample(wl.job, wl.x_T, wl.noise, wl.tables, check=False)


def bpd():
    return wl.den.bpd(wl.job, x0, wl.noise, wl.tables, check=False)


sample(), bpd()                                                        # warm-up (features, step tables, streams)
torch.cuda.synchronize()
loops = {"sample": [], "bpd": []}
for _ in range(3):
    loops["sample"].append(event_ms(sample, 2))
    loops["bpd"].append(event_ms(bpd, 2))
ratios = [a / b for a, b in zip(loops["bpd"], loops["sample"])]
print(f"cfg2 loop ({n} nodes, {n_struct} structures, {bench.T_STEPS} steps): sampling {['%.2f' % v for v in loops['sample']]} ms "
      f"({['%.1f' % (n_struct / (v * 1e-3)) for v in loops['sample']]} structures/s), bpd {['%.2f' % v for v in loops['bpd']]} ms "
      f"({['%.1f' % (n_struct / (v * 1e-3)) for v in loops['bpd']]} structures/s), bpd/sampling {['%.4f' % r for r in ratios]}",
      flush=True)
res = wl.den.bpd(wl.job, x0, wl.noise, wl.tables)                      # with the finiteness check
assert all(bool(torch.isfinite(v).all()) for v in res.values())

# (2) one 96-frame batch, 96 distinct timesteps
F, L = 96, 87
prot = synth.make_protein(L, 1001, n_frames=F)
frames = torch.from_numpy(prot["xyz_full"])[:, 1:-1]
z = torch.from_numpy(prot["z_full"])[1:-1]
st = wl.den.prepare_structures([f for f in frames], [z for _ in frames])
job = wl.den.make_job(st, list(range(F)))
tb = Tables(named_betas("linear", 1000), space_timesteps(1000, "1000"))
g = torch.Generator(device=dev)
g.manual_seed(5)
xs = torch.randn(F * L, 3, device=dev, generator=g)
nz = torch.randn(F * L, 3, device=dev, generator=g)
distinct = [(10 * k + 3) % 1000 for k in range(F)]
shared = 503
per_sample = lambda: wl.den.loss_terms(job, xs, distinct, nz, tb, check=False)     # noqa: E731
one_t = lambda: wl.den.loss_terms(job, xs, shared, nz, tb, check=False)            # noqa: E731
per_sample(), one_t()
torch.cuda.synchronize()
ms_distinct = [event_ms(per_sample, 3) for _ in range(3)]
ms_shared = [event_ms(one_t, 3) for _ in range(3)]
print(f"training-loss terms, {F} frames x L={L}: 96 distinct timesteps {['%.2f' % v for v in ms_distinct]} ms "
      f"({['%.0f' % (F / (v * 1e-3)) for v in ms_distinct]} structures/s), one shared timestep {['%.2f' % v for v in ms_shared]} ms "
      f"({['%.0f' % (F / (v * 1e-3)) for v in ms_shared]} structures/s)", flush=True)
print(json.dumps({"tool": "loss_eval_timing", "config": "cfg2", "n_nodes": n, "n_structures": n_struct, "steps": bench.T_STEPS,
                  "loop_ms": loops, "bpd_over_sampling": ratios,
                  "per_sample_t": {"frames": F, "L": L, "distinct_ms": ms_distinct, "shared_ms": ms_shared},
                  "device": torch.cuda.get_device_name(dev)}))
