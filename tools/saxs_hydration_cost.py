#!/usr/bin/env python3
"""What the SAXS hydration model costs (metrics.saxs_partials: six partial Debye sums from one pass over the pairs, three
fp32 accumulators per sine) beside the plain profile (metrics.saxs_profile, one accumulator) and the SASA call that gives
the exposure, and what the fit of (c1, c2) on the default grid costs.

    python tools/saxs_hydration_cost.py [--out profiles/saxs_hydration_cost.txt] [--repeats 10]

Inputs as tools/saxs_cost.py: (i) the four synthetic PED proteins x 100 structures at Q = 51; (ii) the largest cfg4 protein
x 32 members at Q = 51 and Q = 256.  "partials launch" is codlad_saxs_partials alone, on an exposure computed before the
clock starts - the figure to set beside the plain launch; "saxs_partials" is the public call, SASA included.  HIP events and
wall clock as in tools/cost_common.py.  The q-chunk of the kernel is a compile-time constant: to compare two values build a
second library (CODLAD_CXXFLAGS=-DCODLAD_SAXS_HYD_Q_CHUNK=4, kept under another name) and run this tool once per library
with CODLAD_HIP_LIB set.  Needs a GPU: there is nothing to measure without one."""
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread, wall  # noqa: E402
from codlad_amd.metrics import saxs as saxs_mod  # noqa: E402


def measure(title, jobs, q_sizes, repeats, lines):
    lines.append(title)
    for L, (decode, _check, top, S) in jobs:
        xyz = decode()
        n = top.n_atoms
        for Q in q_sizes:
            grid = np.linspace(0.0, 0.5, Q)
            hp = metrics.saxs_partials(xyz, top, q=grid)
            again = metrics.saxs_partials(xyz, top, q=grid)
            plain = metrics.saxs_profile(xyz, top, q=grid)
            same = torch.equal(hp["P"], again["P"]) and torch.equal(hp["mean"], again["mean"])
            tables = next(iter(v for k, v in top._saxs_hydration_tables.items() if k[0] == grid.tobytes()))
            typ, ff_t, ff_d, qd, water = tables
            exposure = hp["exposure"]
            wet = metrics.saxs_combine(hp["mean"], hp["q"], water, 1.02, 1.5)
            sigma = 0.01 * wet + 1e-3 * wet[0]
            calls = [("plain launch", lambda: metrics.saxs_profile(xyz, top, q=grid)),
                     ("partials launch", lambda: saxs_mod._partials_launch(xyz, typ, ff_t, ff_d, exposure, qd, with_mean=True)),
                     ("sasa 960 points", lambda: metrics.sasa(xyz, top, n_points=960)),
                     ("saxs_partials", lambda: metrics.saxs_partials(xyz, top, q=grid)),
                     ("fit, 21 x 61 grid", lambda: metrics.saxs_hydration_fit(hp["mean"], hp["q"], water, 3.7 * wet, sigma))]
            lines.append(f"  L={L:3d} n_atoms={n:4d} structures={S:3d} Q={Q:3d} ({S * n * (n - 1) // 2 * Q:.3e} sinc evaluations): finite "
                         f"{int(hp['n_finite'])}, mean exposure {float(exposure.mean()):.3f}, tt == plain I: "
                         f"{torch.equal(hp['P'][:, 0], plain['I'])}, repeat call bit-identical: {same}")
            med = {}
            for name, fn in calls:
                w, e = wall(fn, repeats, 3), events(fn, repeats)
                med[name] = statistics.median(e)
                lines += [f"    {name:17s} wall (incl. its one sync) {spread(w)}",
                          f"    {name:17s} HIP events                {spread(e)}"]
            lines.append(f"    partials launch / plain launch (median HIP events) = {med['partials launch'] / med['plain launch']:.2f}; "
                         f"saxs_partials / plain launch = {med['saxs_partials'] / med['plain launch']:.2f}")
            lines.append("")


def body(args, dev, lines):
    lines.insert(2, f"q-chunk of codlad_saxs_partials: see the build (header default {saxs_mod.SAXS_HYD_Q_CHUNK}); library "
                    f"{os.path.basename(os.environ.get('CODLAD_HIP_LIB') or 'libcodlad_hip.so')}")
    for k, (title, jobs) in enumerate(decoded_sections(dev)):
        measure(title, jobs, (51,) if k == 0 else (51, 256), args.repeats, lines)


if __name__ == "__main__":
    main("saxs_hydration_cost", body, repeats=10)
