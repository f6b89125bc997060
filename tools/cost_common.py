"""What the cost tools (tools/*_cost.py) share: the three timers, the decoded input of the per-structure tools and the
skeleton of a tool - argument parser, the "needs a GPU" exit, the two header lines, print and --out.  A tool keeps its
`measure` and hands `main` a body(args, dev, lines) that appends what it measured."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codlad_amd import metrics, synth  # noqa: E402
from codlad_amd.engine import Decoder  # noqa: E402
from codlad_amd.utils.cg_input import template_topology  # noqa: E402


def spread(xs):
    return f"min {min(xs) * 1e3:9.3f}  median {statistics.median(xs) * 1e3:9.3f}  max {max(xs) * 1e3:9.3f} ms"


def wall(fn, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def events(fn, repeats):
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def job(L, seed, n_frames, n_members, vae_type, dataname, dev):
    """One protein's decode tail and the check of its output -> (decode(), check(xyz), topology, n_structures)."""
    prot = synth.make_protein(L, seed, n_frames=n_frames, phospho=vae_type != "N6")
    batch = synth.make_batch(prot)
    mean, std = synth.norm_stats(dataname, vae_type)
    dec = Decoder(synth.vqvae_state_dict(vae_type, dataname, 4321), dev, mean, std)
    S = n_frames * n_members
    rep = lambda t: t.repeat(n_members, *([1] * (t.dim() - 1)))                                   # noqa: E731
    lat = synth.gaussian((S, L, 3), 9000 + seed).to(dev)
    cg_z = rep(batch["CG_nxyz"][:, 0].long()).to(dev)
    cg_xyz = rep(batch["CG_nxyz"][:, 1:]).to(dev)
    nbr = batch["CG_nbr_list"]
    pairs = torch.cat([nbr + m * n_frames * L for m in range(n_members)]).to(dev)
    ca_full = rep(batch["OG_CG_nxyz"].reshape(-1, L + 2, 4)[:, :, 1:]).to(dev)
    names = [synth.IDX2THR[int(z)] for z in prot["z_full"]]
    top = template_topology(names[1:-1])

    def decode():
        _idx, zq, _lat = dec.vq(lat)
        ic = dec.ic_decode(zq.reshape(-1, 3), cg_z, cg_xyz, pairs)
        return dec.ic_to_xyz(ca_full, ic.view(S, L, 13, 3), prot["info"])

    return decode, (lambda xyz: metrics.geometry_check(xyz, top)), top, S


def decoded_sections(dev):
    """The two inputs of the per-structure tools, one at a time -> (title, [(L, job)]): the cfg2 decode output, then the
    largest cfg4 protein (built when it is asked for, after the first has been measured)."""
    yield ("(i) cfg2 decode output: 4 PED-shaped proteins x (10 frames x 10 members), N6 decoder",
           [(L, job(L, 1000 + i, 10, 10, "N6", "PED", dev)) for i, L in enumerate(synth.PED_LENGTHS)])
    L = max(synth.atlas_test_lengths())
    yield f"(ii) largest cfg4 protein: L={L}, 1 frame x 32 members, K4 decoder", [(L, job(L, 1, 1, 32, "K4", "Atlas", dev))]


def main(tool, body, repeats=20, options=(), header=None):
    """The skeleton of tools/<tool>.py.  options: (flag, default) integer arguments beside --out and --repeats; header(args)
    -> (what follows the device line, the repeats line) where a tool's differ from the usual ones."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=repeats)
    for flag, default in options:
        ap.add_argument(flag, type=int, default=default)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs an MI355X: a CPU run measures nothing")
    torch.set_grad_enabled(False)
    device_more, repeats_line = header(args) if header else \
        ("", f"repeats: {args.repeats} (3 warm-up); times in ms per call; one call = one protein's structures")
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}{device_more}", repeats_line, ""]
    body(args, "cuda:0", lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
