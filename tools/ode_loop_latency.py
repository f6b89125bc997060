"""What a model evaluation costs in the ODE sampler of the flow-matching models: the fused path (Denoiser.sample_ode: one
codlad_ode_loop call per fixed grid, one codlad_ode_dopri5_attempt per attempted adaptive step) against the step-wise one
(ode.odeint over a callable: per evaluation a device-to-host read of t, an upload and a one-block launch for the adaLN row,
the forward with its logits write, a stream synchronise, one codlad_ode_combine launch per stage), alternated on the same
seeded inputs; the step-wise run is repeated to get the run-to-run spread.  Sizes: one 87-residue protein, and the job of
BASELINE configuration 2 (400 PED-shaped structures).  Methods: euler over 100 intervals, dopri5 at rtol = atol = 1e-5.
For context, the DDPM loop's time per step at the same sizes (the forward is the same, only the tail differs).  Host
clock around calls that end in a device synchronise, warm-up first; a timed sample repeats its call until the window is
at least --window seconds long.  Writes the report (default profiles/ode_fused_latency.txt) and prints one JSON line.

    python tools/ode_loop_latency.py [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from codlad_amd import synth  # noqa: E402
from codlad_amd.diffusion_and_flow import ode  # noqa: E402
from codlad_amd.engine import Denoiser  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ode_fused_latency.txt"))
ap.add_argument("--repeats", type=int, default=4, help="step-wise samples per pair (the fused path runs between them)")
ap.add_argument("--window", type=float, default=0.5, help="least length of a timed sample, seconds")
args = ap.parse_args()

torch.set_grad_enabled(False)
if not torch.cuda.is_available():
    raise SystemExit("ode_loop_latency.py needs an MI355X: a time taken anywhere else says nothing")
dev = torch.device("cuda", 0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def timed(fn, calls=1):
    """(seconds per call, the last call's result) over `calls` calls in one window."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls, out


def calls_for(seconds_per_call):
    return max(1, int(args.window / seconds_per_call + 0.999))


def size_single():
    prot = synth.make_protein(87, 1001, n_frames=1)
    xyz = [torch.from_numpy(prot["xyz_full"])[0, 1:-1]]
    z = [torch.from_numpy(prot["z_full"])[1:-1]]
    return "one 87-residue protein", xyz, z, [0]


def size_cfg2():
    wl = bench.Workload(dev, "cfg2")
    s_key = sorted({u[:2] for u in wl.units})
    s_of = {k: i for i, k in enumerate(s_key)}
    xyz = [torch.from_numpy(wl.proteins[p]["xyz_full"])[f, 1:-1] for p, f in s_key]
    z = [torch.from_numpy(wl.proteins[p]["z_full"])[1:-1] for p, _f in s_key]
    return "BASELINE configuration 2", xyz, z, [s_of[u[:2]] for u in wl.units]


flow = Denoiser(synth.denoiser_state_dict(bench.WEIGHT_SEED, flow=True), dev)
ddpm = Denoiser(synth.denoiser_state_dict(bench.WEIGHT_SEED), dev)
from codlad_amd.diffusion_and_flow.schedule import Tables, named_betas, space_timesteps  # noqa: E402
tables = Tables(named_betas("linear", 1000), space_timesteps(1000, str(bench.T_STEPS)))
report = {"tool": "ode_loop_latency", "device": torch.cuda.get_device_name(dev), "sizes": {}}
METHODS = (("euler", torch.linspace(0, 1, 101).tolist(), {}), ("dopri5", [0.0, 1.0], dict(rtol=1e-5, atol=1e-5)))

for make in (size_single, size_cfg2):
    label, xyz, z, members = make()
    job = flow.make_job(flow.prepare_structures(xyz, z), members)
    n = job.n_nodes
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    y0 = torch.randn(n, 3, generator=g, device=dev)
    say(f"== {label}: {len(members)} structures, {n} nodes")
    entry = report["sizes"][label] = {"n_nodes": n, "n_structures": len(members)}
    f = lambda t, y: flow.forward(job, y, float(t))  # noqa: E731  (t arrives as a device scalar, as from torchdiffeq)
    for method, ts, tol in METHODS:
        fused = lambda: flow.sample_ode(job, y0, ts, method=method, **tol)  # noqa: E731
        stepwise = lambda: ode.odeint(f, y0, ts, method=method, return_stats=True, **tol)  # noqa: E731
        (_tf, (yf, sf)), (_ts, (ys, ss)) = timed(fused), timed(stepwise)           # warm-up, and the results compared
        diff = float((yf[-1] - ys[-1]).abs().max())
        calls = calls_for(timed(stepwise)[0])
        t_step, t_fused = [], []
        for r in range(args.repeats):
            t_step.append(timed(stepwise, calls)[0])
            if r + 1 < args.repeats:
                t_fused.append(timed(fused, calls)[0])
        us_step = [1e6 * t / ss["n_eval"] for t in t_step]
        us_fused = [1e6 * t / sf["n_eval"] for t in t_fused]
        spread = max(us_step) - min(us_step)
        gain = min(us_step) - max(us_fused)
        say(f"{method:6s}: evaluations fused {sf['n_eval']} / step-wise {ss['n_eval']} "
            f"(accepted {sf['n_accept']}, rejected {sf['n_reject']}); max |fused - step-wise| of the result {diff:.3e}")
        say(f"        ({calls} calls per sample) step-wise {['%.1f' % v for v in us_step]} us per evaluation (spread {spread:.1f}), "
            f"fused {['%.1f' % v for v in us_fused]} us per evaluation; "
            f"fused below step-wise by {gain:.1f} us ({'more' if gain > spread else 'NOT more'} than the spread)")
        entry[method] = {"n_eval_fused": sf["n_eval"], "n_eval_stepwise": ss["n_eval"], "us_per_eval_stepwise": us_step,
                         "us_per_eval_fused": us_fused, "spread_us": spread, "max_abs_diff": diff}
    # context: the DDPM loop at the same size (its own weights: 6 outputs)
    djob = ddpm.make_job(ddpm.prepare_structures(xyz, z), members)
    x_T = torch.randn(n, 3, generator=g, device=dev)
    noise = torch.randn(bench.T_STEPS, n, 3, generator=g, device=dev)
    loop = lambda: ddpm.sample(djob, x_T, noise, tables)  # noqa: E731
    calls = calls_for(timed(loop)[0])
    us = [1e6 * timed(loop, calls)[0] / bench.T_STEPS for _ in range(args.repeats)]
    say(f"DDPM  : {['%.1f' % v for v in us]} us per step ({bench.T_STEPS} steps, the fused loop)")
    entry["ddpm_us_per_step"] = us

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n" + json.dumps(report) + "\n")
print(json.dumps(report))
