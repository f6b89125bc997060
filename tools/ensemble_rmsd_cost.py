#!/usr/bin/env python3
"""What the superposed-RMSD arithmetic after the sampling path costs on the host and on the device.

    python tools/ensemble_rmsd_cost.py [--out profiles/ensemble_rmsd_cost.txt] [--repeats 20] [--host_repeats 5]

(i)  compute_div per data file at the cfg2 shapes (G = 10 members, F = 10 frames, the atom counts of the four synthetic
     PED proteins).  Host path = what the evaluation block did before the device path existed: every member's
     coordinates and the true ones copied device -> host per member (Evaluation.add), then the float64 SVD loop
     (metrics.compute_div on CPU tensors, 2 G F calls of superposed_rmsd).  Device path = metrics.compute_div on the
     device tensors: stack, member mean, moments + pair kernels, one transfer of the scalar.
(ii) pairwise_rmsd at G = 32, F = 4 for the largest cfg4 protein (505 residues) against the superposed_rmsd loop over the
     upper triangle on host copies.

Both paths start from the same device tensors.  Wall clock is taken around the whole call including its one
synchronisation; the device side of the device path also by HIP events.  Every shape is warmed up; min / median / max
over the repeats are reported.  Needs a GPU: there is nothing to measure without one."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread, synth, wall  # noqa: E402


def atom_count(L, seed):
    z = synth.sequence(L + 2, 2000 + seed)
    return sum(len(synth.PDB_ATOM_ORDER[synth.IDX2THR[int(r)]]) for r in z[1:-1])


def ensemble(G, F, n, seed, dev):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((1, F, n, 3)) * 12.0
    gen = (base + rng.standard_normal((G, F, n, 3)) * 1.5).astype(np.float32)
    ref = (base[0] + rng.standard_normal((F, n, 3)) * 0.5).astype(np.float32)
    return torch.from_numpy(gen).to(dev), torch.from_numpy(ref).to(dev)


def body(args, dev, lines):
    lines.append("(i) compute_div per data file, cfg2 shapes: G = 10 members x F = 10 frames (200 superpositions x 2 tables)")
    tot_host, tot_dev = 0.0, 0.0
    for i, L in enumerate(synth.PED_LENGTHS):
        n = atom_count(L, 1000 + i)
        gen, ref = ensemble(10, 10, n, i, dev)
        members = [g.contiguous() for g in gen]

        def host_path():
            recon, true = [], None
            for g in members:                  # Evaluation.add, once per member
                recon.append(g.cpu())
                true = ref.cpu()
            return metrics.compute_div(recon, true)

        def device_path():
            return metrics.compute_div(members, ref)

        h, d = host_path(), device_path()
        th = wall(host_path, args.host_repeats, 1)
        td = wall(device_path, args.repeats, 3)
        te = events(lambda: metrics.diversity_terms(members, ref), args.repeats)
        tot_host += statistics.median(th)
        tot_dev += statistics.median(td)
        lines += [f"  L={L:3d} n_atoms={n:4d}  diversity host {h:.15f} device {d:.15f} (|diff| {abs(h - d):.1e})",
                  f"    host path   wall (copies + SVD loop)      {spread(th)}",
                  f"    device path wall (incl. its one sync)     {spread(td)}",
                  f"    device path HIP events (diversity_terms)  {spread(te)}",
                  f"    median wall ratio host / device: {statistics.median(th) / statistics.median(td):.1f}x"]
    lines += [f"  four data files, sum of medians: host {tot_host * 1e3:.3f} ms, device {tot_dev * 1e3:.3f} ms "
              f"({tot_host / tot_dev:.1f}x)", ""]

    L = max(synth.atlas_test_lengths())
    n = atom_count(L, 1)
    G, F = 32, 4
    gen, _ref = ensemble(G, F, n, 99, dev)
    lines.append(f"(ii) pairwise_rmsd, largest cfg4 protein: L={L}, n_atoms={n}, G={G} members x F={F} frames "
                 f"({F * G * (G - 1) // 2} superpositions)")

    def host_pairwise():
        x = gen.cpu()
        out = torch.zeros(F, G, G, dtype=torch.float64)
        for f in range(F):
            for a in range(G):
                for b in range(a + 1, G):
                    out[f, a, b] = out[f, b, a] = metrics.superposed_rmsd(x[a, f], x[b, f])
        return out

    hm, dm = host_pairwise(), metrics.pairwise_rmsd(gen).cpu()
    th = wall(host_pairwise, args.host_repeats, 1)
    td = wall(lambda: metrics.pairwise_rmsd(gen), args.repeats, 3)
    te = events(lambda: metrics.pairwise_rmsd(gen), args.repeats)
    lines += [f"    largest |host - device| over the matrix: {float((hm - dm).abs().max()):.1e} A",
              f"    host loop   wall (copy + SVD loop)        {spread(th)}",
              f"    device path wall (incl. one sync)         {spread(td)}",
              f"    device path HIP events                    {spread(te)}",
              f"    median wall ratio host / device: {statistics.median(th) / statistics.median(td):.1f}x"]


if __name__ == "__main__":
    main("ensemble_rmsd_cost", body, options=[("--host_repeats", 5)], header=lambda args: (
        f"; host threads {torch.get_num_threads()}",
        f"repeats: device {args.repeats} (3 warm-up), host {args.host_repeats} (1 warm-up); times in ms per call"))
