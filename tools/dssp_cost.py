#!/usr/bin/env python3
"""What the secondary-structure assignment costs (metrics.hbonds, dssp_assign, dssp) beside the stereochemistry check and the
geometry check of the same structures.

    python tools/dssp_cost.py [--out profiles/dssp_cost.txt] [--repeats 20]

Inputs, as tools/geometry_check_cost.py builds them (the decode tail of seeded random weights):
(i)  the cfg2 decode output: the four synthetic PED proteins (46-129 residues), 10 frames x 10 members = 100 structures each;
(ii) the largest cfg4 protein (505 residues) x 32 members of one frame.
Per input: stage 1 (codlad_dssp_hbonds), stage 2 (codlad_dssp_assign on stage 1's bitmaps), both together (metrics.dssp),
the stereochemistry check and the geometry check.  The device side by HIP events, the wall clock around the whole call
including its one synchronisation; every shape is warmed up; min / median / max over the repeats.  The float64 numpy
reference of the tests (tests/dssp_ref.reference: both stages) is timed on ONE structure of the smallest protein: what the
same assignment costs on the host.  Needs a GPU: there is nothing to measure without one."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread, wall  # noqa: E402


def measure(title, jobs, repeats, lines):
    lines.append(title)
    for L, (decode, check, top, S) in jobs:
        xyz = decode()
        hb = metrics.hbonds(xyz, top)
        calls = [("dssp stage 1", lambda: metrics.hbonds(xyz, top)),
                 ("dssp stage 2", lambda: metrics.dssp_assign(hb["acc"], hb["don"], hb["geom"], hb["finite"])),
                 ("dssp both", lambda: metrics.dssp(xyz, top)),
                 ("stereo check", lambda: metrics.stereo_check(xyz, top)),
                 ("geometry check", lambda: check(xyz))]
        a, b = metrics.dssp(xyz, top), metrics.dssp(xyz, top)
        same = all(torch.equal(a[k], b[k]) for k in ("acc", "don", "geom", "ss", "bridge", "counts", "partner")) and \
            torch.equal(a["e_best"].view(torch.int32), b["e_best"].view(torch.int32))
        prop = metrics.ss_propensity(a["ss"]).mean(dim=0).tolist()
        bonds = float(sum(bin(w & (2 ** 64 - 1)).count("1") for w in a["acc"].flatten().tolist())) / S
        lines.append(f"  L={L:3d} n_atoms={top.n_atoms:4d} structures={S:3d}: {bonds:.1f} hydrogen bonds per structure; mean share "
                     + " ".join(f"{c if c != ' ' else 'loop'} {p:.3f}" for c, p in zip(metrics.DSSP_CODES, prop))
                     + f"; repeat call bit-identical: {same}")
        for name, fn in calls:
            w, e = wall(fn, repeats, 3), events(fn, repeats)
            lines += [f"    {name:16s} wall (incl. its one sync) {spread(w)}",
                      f"    {name:16s} HIP events                {spread(e)}"]
        lines.append("")


def host_reference(jobs, lines):
    from tests import dssp_ref as dr
    L, (decode, _check, top, _S) = jobs[0]
    x = decode()[:1]
    xh = x.cpu().numpy()
    t0 = time.perf_counter()
    ref = dr.reference(xh, top)
    dt = time.perf_counter() - t0
    got = metrics.dssp(x, top)["ss"][0].cpu().numpy()
    lines += [f"float64 numpy reference (tests/dssp_ref.reference, both stages), ONE structure of L={L}: {dt * 1e3:.1f} ms wall; "
              f"residues whose label differs from the device's: {int((np.asarray(ref['ss'][0]) != got).sum())}", ""]


def body(args, dev, lines):
    sections = []
    for title, jobs in decoded_sections(dev):
        measure(title, jobs, args.repeats, lines)
        sections.append(jobs)
    host_reference(sections[0], lines)


if __name__ == "__main__":
    main("dssp_cost", body)
