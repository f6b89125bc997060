#!/usr/bin/env python3
"""What lDDT against the true frames (metrics.lddt, codlad_lddt) costs beside the geometry check of the same structures
and beside the same counts made with torch on the device.

    python tools/lddt_cost.py [--out profiles/lddt_cost.txt] [--repeats 5]

(i)  one cfg2 shape at a time: the four synthetic PED proteins, 10 true frames x 10 members = 100 structures each.
(ii) the largest cfg4 protein (505 residues, 4 325 atoms) x 32 members of one true frame.

The true frames are synth.make_atoms' (what test.py --lddt scores against on the synthetic route); a member is its frame plus
seeded Gaussian noise of 1 A, so the share of included pairs is that of the frames.  Timed by HIP events around one call,
tables cached (the first call, which builds them on the host, is reported apart); median of the repeats after 3 warm-up
calls, in one process: lddt without and with symmetry, geometry_check, and the torch baseline - two cdist, a mask, a sum
per threshold - which allocates [S, n, n] matrices and is chunked over the structures where those would pass 2 GiB.
Needs a GPU: there is nothing to measure without one."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, spread  # noqa: E402
from codlad_amd import metrics, synth  # noqa: E402
from codlad_amd.utils.cg_input import template_topology  # noqa: E402

THRESHOLDS = (0.5, 1.0, 2.0, 4.0)


def inputs(L, seed, n_frames, n_members, phospho, dev):
    prot = synth.make_protein(L, seed, n_frames=n_frames, phospho=phospho)
    top = template_topology([synth.IDX2THR[int(z)] for z in prot["z_full"]][1:-1])
    truth = synth.make_atoms(prot, range(n_frames), seed=seed)["nxyz"][:, 1:].reshape(n_frames, top.n_atoms, 3).float().to(dev)
    index = torch.arange(n_frames).repeat(n_members)
    gen = torch.Generator().manual_seed(7000 + seed)
    models = truth[index.to(dev)] + torch.randn(n_frames * n_members, top.n_atoms, 3, generator=gen).to(dev)
    return top, models.contiguous(), truth.contiguous(), index


def torch_counts(models, truth, index, res, chunk):
    """The same counts with torch: per chunk of structures two cdist, the inclusion mask, a sum per threshold."""
    sep = (res[:, None] - res[None, :]).abs() >= 1
    total, kept = [], []
    for a in range(0, models.shape[0], chunk):
        d_ref = torch.cdist(truth[index[a:a + chunk]], truth[index[a:a + chunk]])
        d_mod = torch.cdist(models[a:a + chunk], models[a:a + chunk])
        inc = (d_ref < 15.0) & sep
        diff = (d_mod - d_ref).abs()
        total.append(inc.sum(-1))
        kept.append(torch.stack([(inc & (diff < t)).sum(-1) for t in THRESHOLDS], -1))
    return torch.cat(total), torch.cat(kept)


def measure(title, cases, repeats, lines, dev):
    lines.append(title)
    for L, seed, n_frames, n_members, phospho in cases:
        top, models, truth, index = inputs(L, seed, n_frames, n_members, phospho, dev)
        S, n = models.shape[0], top.n_atoms
        idx_dev = index.to(dev)
        res = torch.from_numpy(top.residue_of_atom).to(dev)
        chunk = max(1, min(S, (1 << 31) // (4 * n * n)))
        calls = {"lddt, symmetry off": lambda: metrics.lddt(models, truth, top, ref_index=index, symmetry=False),
                 "lddt, symmetry on": lambda: metrics.lddt(models, truth, top, ref_index=index),
                 "geometry_check": lambda: metrics.geometry_check(models, top),
                 "torch (2 cdist, mask, sums)": lambda: torch_counts(models, truth, idx_dev, res, chunk)}
        t0 = time.perf_counter()
        out = calls["lddt, symmetry on"]()
        torch.cuda.synchronize()
        first = time.perf_counter() - t0
        plain = calls["lddt, symmetry off"]()
        again = calls["lddt, symmetry on"]()
        same = all(torch.equal(out[k], again[k]) for k in ("atom_total", "atom_preserved", "swapped"))
        t_total, _t_kept = calls["torch (2 cdist, mask, sums)"]()
        included = int(plain["counts"][:, 0].sum())
        lines.append(f"  L={L:3d} n_atoms={n:4d} structures={S:3d} ({S * n * (n - 1) / 1e6:.1f} M ordered atom pairs, "
                     f"{100.0 * included / (S * n * (n - 1)):.1f} % included)  mean lDDT {float(plain['global'].mean()):.4f}, with symmetry "
                     f"{float(out['global'].mean()):.4f} ({int(out['swapped'].sum())} residues swapped); repeat call bit-identical: {same}; "
                     f"totals that differ from torch's (cdist rounds otherwise): {int((t_total != plain['atom_total']).sum())} of {S * n}")
        med = {}
        for name, fn in calls.items():
            for _ in range(3):
                fn()
            ts = events(fn, repeats)
            med[name] = statistics.median(ts)
            lines.append(f"    {name:28s} HIP events  {spread(ts)}")
        lines += [f"    lddt first call (host tables)  {first * 1e3:9.3f} ms",
                  f"    medians: lddt / geometry_check {med['lddt, symmetry off'] / med['geometry_check']:.2f}, symmetry on / off "
                  f"{med['lddt, symmetry on'] / med['lddt, symmetry off']:.2f}, torch / lddt "
                  f"{med['torch (2 cdist, mask, sums)'] / med['lddt, symmetry off']:.1f}  "
                  f"({S * n * (n - 1) / med['lddt, symmetry off'] / 1e9:.1f} G ordered pairs/s)"]
    lines.append("")


def body(args, dev, lines):
    measure("(i) cfg2 shapes: 4 PED-shaped proteins x (10 true frames x 10 members)",
            [(L, 1000 + i, 10, 10, False) for i, L in enumerate(synth.PED_LENGTHS)], args.repeats, lines, dev)
    L = max(synth.atlas_test_lengths())
    measure(f"(ii) largest cfg4 protein: L={L}, 1 true frame x 32 members", [(L, 1, 1, 32, True)], args.repeats, lines, dev)


if __name__ == "__main__":
    main("lddt_cost", body, repeats=5,
         header=lambda a: ("", f"repeats: {a.repeats} (3 warm-up); times in ms per call; one call = one protein's structures"))
