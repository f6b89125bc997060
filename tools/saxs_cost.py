#!/usr/bin/env python3
"""What the SAXS profile of an ensemble costs (metrics.saxs_profile: the Debye sum over all atom pairs) beside the SASA of the
same structures.

    python tools/saxs_cost.py [--out profiles/saxs_cost.txt] [--repeats 10]

Inputs, as tools/observables_cost.py builds them (the decode tail of seeded random weights):
(i)  the cfg2 decode output: the four synthetic PED proteins, 10 frames x 10 members = 100 structures each, at Q = 51;
(ii) the largest cfg4 protein (505 residues) x 32 members of one frame, at Q = 51 and at Q = 256.
Wall clock is taken around the whole call including its one synchronisation, the device side also by HIP events; every shape
is warmed up; min / median / max over the repeats.  The float64 numpy reference of the tests (tests/saxs_ref.debye64) is
timed on ONE structure of the smallest protein at Q = 51, and the device's distance from it is printed in units of the
float32 restatement's (tests/saxs_ref.debye32): the ratio the tests hold below 4.  Needs a GPU: there is nothing to measure
without one."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread, wall  # noqa: E402


def measure(title, jobs, q_sizes, repeats, lines):
    lines.append(title)
    for L, (decode, _check, top, S) in jobs:
        xyz = decode()
        grids = {Q: np.linspace(0.0, 0.5, Q) for Q in q_sizes}
        calls = [(f"saxs Q = {Q:3d}", lambda Q=Q: metrics.saxs_profile(xyz, top, q=grids[Q])) for Q in q_sizes]
        calls.append(("sasa 960 points", lambda: metrics.sasa(xyz, top, n_points=960)))
        a, b = metrics.saxs_profile(xyz, top), metrics.saxs_profile(xyz, top)
        same = torch.equal(a["I"], b["I"]) and torch.equal(a["mean"], b["mean"])
        mean = a["mean"].cpu().numpy()
        n = top.n_atoms
        lines.append(f"  L={L:3d} n_atoms={n:4d} structures={S:3d} ({S * n * (n - 1) // 2 * 51:.3e} sinc evaluations at Q = 51): "
                     f"finite {int(a['n_finite'])}, mean I(0) {mean[0]:.5g}, I(0.1) {mean[10]:.5g}, I(0.5) {mean[50]:.5g}; "
                     f"repeat call bit-identical: {same}")
        for name, fn in calls:
            w, e = wall(fn, repeats, 3), events(fn, repeats)
            lines += [f"    {name:16s} wall (incl. its one sync) {spread(w)}",
                      f"    {name:16s} HIP events                {spread(e)}"]
        lines.append("")


def host_reference(jobs, lines):
    from tests import saxs_ref as sr
    L, (decode, _check, top, _S) = jobs[0]
    x = decode()[:1].cpu().numpy()
    groups, types = metrics.saxs_groups(top)
    q = np.linspace(0.0, 0.5, 51).astype(np.float32)
    table = metrics.form_factors(q.astype(np.float64), groups).astype(np.float32)
    t0 = time.perf_counter()
    ref, A = sr.debye64(x, types, table, q)
    dt = time.perf_counter() - t0
    dev32 = (np.abs(sr.debye32(x[0], types, table, q) - ref[0]) / A[0]).max()
    got = metrics.saxs_profile(torch.from_numpy(x).cuda(), top, q=q)["I"][0].cpu().numpy()
    lines += [f"float64 numpy reference (tests/saxs_ref.debye64), ONE structure of L={L} ({top.n_atoms} atoms) at Q = 51: "
              f"{dt * 1e3:.1f} ms wall; dev32 of the float32 restatement {dev32:.3e}; the device's largest "
              f"|I_dev - I_ref| / (dev32 A) = {(np.abs(got - ref[0]) / (dev32 * A[0])).max():.3f} (the tests hold it below 4)", ""]


def body(args, dev, lines):
    first = None
    for k, (title, jobs) in enumerate(decoded_sections(dev)):
        measure(title, jobs, (51,) if k == 0 else (51, 256), args.repeats, lines)
        first = first or jobs
    host_reference(first, lines)


if __name__ == "__main__":
    main("saxs_cost", body, repeats=10)
