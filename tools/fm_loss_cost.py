"""What a time of the flow-matching loss sweep costs: the fused sweep (Denoiser.fm_loss_sweep: one codlad_fm_loss_loop call,
per time the path kernel, the forward and the loss kernel) against the step-wise path (Denoiser.fm_loss_terms per time: the
same three pieces, each time with its own allocations, launches from Python and a status check that synchronises) and against
the euler ODE loop's cost per model evaluation (one forward and its stage kernel: the yardstick of
profiles/ode_fused_latency.txt, measured again here), the three alternated in one call on the same seeded inputs.  Sizes:
one 87-residue protein, and the job of BASELINE configuration 2 (400 PED-shaped structures).  K = 20 times, the midpoints
(k + 0.5) / K.  Host clock around calls that end in a device synchronise, warm-up first; a timed sample repeats its call
until the window is at least --window seconds long.  Writes the report (default profiles/fm_loss_cost.txt) and prints one
JSON line.

    python tools/fm_loss_cost.py [--out FILE]
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
from codlad_amd.engine import Denoiser  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fm_loss_cost.txt"))
ap.add_argument("--repeats", type=int, default=4, help="samples per path")
ap.add_argument("--window", type=float, default=0.5, help="least length of a timed sample, seconds")
ap.add_argument("--times", type=int, default=20, help="K")
args = ap.parse_args()

torch.set_grad_enabled(False)
if not torch.cuda.is_available():
    raise SystemExit("fm_loss_cost.py needs an MI355X: a time taken anywhere else says nothing")
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
    return "one 87-residue protein", [torch.from_numpy(prot["xyz_full"])[0, 1:-1]], [torch.from_numpy(prot["z_full"])[1:-1]], [0]


def size_cfg2():
    wl = bench.Workload(dev, "cfg2")
    s_key = sorted({u[:2] for u in wl.units})
    s_of = {k: i for i, k in enumerate(s_key)}
    xyz = [torch.from_numpy(wl.proteins[p]["xyz_full"])[f, 1:-1] for p, f in s_key]
    z = [torch.from_numpy(wl.proteins[p]["z_full"])[1:-1] for p, _f in s_key]
    return "BASELINE configuration 2", xyz, z, [s_of[u[:2]] for u in wl.units]


den = Denoiser(synth.denoiser_state_dict(bench.WEIGHT_SEED, flow=True), dev)
K = args.times
ts = [(k + 0.5) / K for k in range(K)]
report = {"tool": "fm_loss_cost", "device": torch.cuda.get_device_name(dev), "K": K, "sizes": {}}

for make in (size_single, size_cfg2):
    label, xyz, z, members = make()
    job = den.make_job(den.prepare_structures(xyz, z), members)
    n = job.n_nodes
    g = torch.Generator(device=dev)
    g.manual_seed(42)
    x0, x1 = torch.randn(n, 3, generator=g, device=dev), torch.randn(n, 3, generator=g, device=dev)
    eps = torch.randn(K, n, 3, generator=g, device=dev)
    say(f"== {label}: {len(members)} structures, {n} nodes, K = {K}")
    kw = dict(kind="icfm", sigma=0.1, x0=x0)
    paths = {
        "fused sweep": lambda: den.fm_loss_sweep(job, x1, ts, eps=eps, **kw)["l2"],
        "step-wise": lambda: torch.stack([den.fm_loss_terms(job, x1, tv, eps=eps[k], **kw)["l2"] for k, tv in enumerate(ts)]),
        "euler ODE loop": lambda: den.sample_ode(job, x0, torch.linspace(0, 1, K + 1).tolist(), method="euler")[0],
    }
    first = {name: timed(fn) for name, fn in paths.items()}                      # warm-up, and the results compared
    equal = bool(torch.equal(first["fused sweep"][1], first["step-wise"][1]))
    calls = {name: calls_for(timed(fn)[0]) for name, fn in paths.items()}
    us = {name: [] for name in paths}
    for _r in range(args.repeats):                                               # alternated: drift hits all three alike
        for name, fn in paths.items():
            us[name].append(1e6 * timed(fn, calls[name])[0] / K)
    say(f"fused sweep = step-wise, bit for bit: {equal}")
    for name in paths:
        say(f"{name:15s}: ({calls[name]} calls per sample) {['%.1f' % v for v in us[name]]} us per time "
            f"(spread {max(us[name]) - min(us[name]):.1f})")
    extra = min(us["fused sweep"]) - max(us["euler ODE loop"])
    say(f"a sweep time above an euler evaluation (one forward and its stage kernel) by {extra:.1f} us at least; "
        f"fused below step-wise by {min(us['step-wise']) - max(us['fused sweep']):.1f} us at least")
    report["sizes"][label] = {"n_nodes": n, "n_structures": len(members), "bit_equal": equal,
                              "us_per_time": us, "calls_per_sample": calls}

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n" + json.dumps(report) + "\n")
print(json.dumps(report))
