#!/usr/bin/env python3
"""What the reference-free geometry check (metrics.geometry_check, codlad_geometry_check) costs beside the decode tail
that produces its input.

    python tools/geometry_check_cost.py [--out profiles/geometry_check_cost.txt] [--repeats 20]

(i)  the cfg2 decode output: the four synthetic PED proteins, 10 frames x 10 members = 100 structures each (400 in all);
     per protein one decode tail (VQ lookup + IC decoder + ic_to_xyz on 100 structures) and one check of its output.
(ii) the largest cfg4 protein (505 residues, K4 decoder) x 32 members of one frame.

Latents are drawn N(mean, std) as bench.py's decode-only configuration draws them (seeded random weights: the geometry is
what such a decoder makes, which is what the check then counts).  Wall clock is taken around the whole call including its
one synchronisation, the device side also by HIP events; every shape is warmed up; min / median / max over the repeats.
The exclusion list and bond tables of a topology are built once on the host and cached on it: the first call's wall
clock is reported apart.  Needs a GPU: there is nothing to measure without one."""
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


def measure(title, jobs, repeats, lines):
    lines.append(title)
    tot = {"decode": 0.0, "check": 0.0}
    for L, (decode, check, top, S) in jobs:
        xyz = decode()
        t0 = time.perf_counter()
        geo = check(xyz)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0                     # includes the host-side tables of the topology
        wd, ed = wall(decode, repeats, 3), events(decode, repeats)
        wc, ec = wall(lambda: check(xyz), repeats, 3), events(lambda: check(xyz), repeats)
        again = check(xyz)
        same = torch.equal(geo["counts"], again["counts"]) and torch.equal(geo["min_dist"], again["min_dist"])
        c = geo["counts"].double().mean(0).tolist()
        pairs = S * top.n_atoms * (top.n_atoms - 1) // 2
        tot["decode"] += statistics.median(ed)
        tot["check"] += statistics.median(ec)
        lines += [f"  L={L:3d} n_atoms={top.n_atoms:4d} structures={S:3d} ({pairs / 1e6:.1f} M atom pairs)  mean per structure: "
                  f"broken {c[0]:.1f} spurious {c[1]:.1f} bonded {c[2]:.1f} near {c[3]:.0f} clash {c[4]:.1f}; "
                  f"valid {float(geo['valid'].double().mean()):.2f}; repeat call bit-identical: {same}",
                  f"    decode tail   wall (incl. its one sync)  {spread(wd)}",
                  f"    decode tail   HIP events                 {spread(ed)}",
                  f"    geometry check wall (incl. its one sync) {spread(wc)}",
                  f"    geometry check HIP events                {spread(ec)}  ({pairs / statistics.median(ec) / 1e9:.1f} G pairs/s)",
                  f"    geometry check first call (host tables)  {first * 1e3:9.3f} ms",
                  f"    check / decode tail (median HIP events): {statistics.median(ec) / statistics.median(ed):.2f}"]
    lines += [f"  sum of medians (HIP events): decode tail {tot['decode'] * 1e3:.3f} ms, geometry check {tot['check'] * 1e3:.3f} ms", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geometry_check_cost needs an MI355X: a CPU run measures nothing")
    torch.set_grad_enabled(False)
    dev = "cuda:0"
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}",
             f"repeats: {args.repeats} (3 warm-up); times in ms per call; one call = one protein's structures", ""]
    measure("(i) cfg2 decode output: 4 PED-shaped proteins x (10 frames x 10 members), N6 decoder",
            [(L, job(L, 1000 + i, 10, 10, "N6", "PED", dev)) for i, L in enumerate(synth.PED_LENGTHS)], args.repeats, lines)
    L = max(synth.atlas_test_lengths())
    measure(f"(ii) largest cfg4 protein: L={L}, 1 frame x 32 members, K4 decoder",
            [(L, job(L, 1, 1, 32, "K4", "Atlas", dev))], args.repeats, lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
