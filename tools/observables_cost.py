#!/usr/bin/env python3
"""What the ensemble observables cost (metrics.sasa, contact_map, radius_of_gyration) beside the geometry check of the same
structures.

    python tools/observables_cost.py [--out profiles/observables_cost.txt] [--repeats 20]

Inputs, as tools/geometry_check_cost.py builds them (the decode tail of seeded random weights):
(i)  the cfg2 decode output: the four synthetic PED proteins, 10 frames x 10 members = 100 structures each;
(ii) the largest cfg4 protein (505 residues) x 32 members of one frame.
Per input: SASA at 96 and at 960 points per atom, the geometry check, the CA contact map at 8 A, the all-atom contact map
and the radius of gyration.  Wall clock is taken around the whole call including its one synchronisation, the device side
also by HIP events; every shape is warmed up; min / median / max over the repeats.  The float64 numpy reference of the tests
(tests/observables_ref.margins) is timed on ONE structure of the smallest protein at 96 points: what the same decision
costs on the host.  Needs a GPU: there is nothing to measure without one."""
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
        ca = top.select("CA")
        calls = [("geometry check", lambda: check(xyz)),
                 ("sasa  96 points", lambda: metrics.sasa(xyz, top, n_points=96)),
                 ("sasa 960 points", lambda: metrics.sasa(xyz, top, n_points=960)),
                 ("contact map CA", lambda: metrics.contact_map(xyz, sel=ca, cutoff=8.0)),
                 ("contact map all", lambda: metrics.contact_map(xyz, cutoff=8.0)),
                 ("radius of gyr.", lambda: metrics.radius_of_gyration(xyz))]
        a, b = metrics.sasa(xyz, top, n_points=960), metrics.sasa(xyz, top, n_points=960)
        same = all(torch.equal(a[k], b[k]) for k in ("exposed", "atom", "residue", "total"))
        rg = metrics.radius_of_gyration(xyz)
        lines.append(f"  L={L:3d} n_atoms={top.n_atoms:4d} structures={S:3d}: total SASA {float(a['total'].mean()):.0f} +- "
                     f"{float(a['total'].std()):.0f} A^2, exposed {float(a['exposed'].double().mean()):.1f} of 960 points per atom, "
                     f"Rg {float(rg.mean()):.2f} +- {float(rg.std()):.2f} A; repeat call bit-identical: {same}")
        for name, fn in calls:
            w, e = wall(fn, repeats, 3), events(fn, repeats)
            lines += [f"    {name:16s} wall (incl. its one sync) {spread(w)}",
                      f"    {name:16s} HIP events                {spread(e)}"]
        lines.append("")


def host_reference(jobs, lines):
    from tests import observables_ref as obr
    L, (decode, _check, top, _S) = jobs[0]
    x = decode()[0].cpu().numpy()
    radius = (metrics.vdw_radii(top.element) + 1.4).astype(np.float32)
    dirs = metrics.sphere_points(96).numpy()
    t0 = time.perf_counter()
    m = obr.margins(x, radius, dirs, np.float64)
    dt = time.perf_counter() - t0
    got = metrics.sasa(torch.from_numpy(x[None]).cuda(), top, n_points=96)["exposed"][0].cpu().numpy()
    lines += [f"float64 numpy reference (tests/observables_ref.margins), ONE structure of L={L} ({top.n_atoms} atoms) at 96 points: "
              f"{dt * 1e3:.1f} ms wall; atoms whose count differs from the device's: {int(((m >= 0).sum(1) != got).sum())}", ""]


def body(args, dev, lines):
    sections = []
    for title, jobs in decoded_sections(dev):
        measure(title, jobs, args.repeats, lines)
        sections.append(jobs)
    host_reference(sections[0], lines)


if __name__ == "__main__":
    main("observables_cost", body)
