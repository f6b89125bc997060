#!/usr/bin/env python3
"""What the restrained clash relaxation (metrics.relax, codlad_relax) costs beside the decode tail that produces its input
and the geometry check that judges it.

    python tools/relax_cost.py [--out profiles/relax_cost.txt] [--repeats 10] [--n_iter 200]

The two job shapes of tools/geometry_check_cost.py, built by cost_common's `job`: (i) the four synthetic PED proteins of cfg2, 10
frames x 10 members = 100 structures each; (ii) the largest cfg4 protein (505 residues) x 32 members.  Per shape: the decode
tail, one geometry check, and relax with --n_iter iterations (two launches each, no host synchronisation), by HIP events
around the whole call; every shape is warmed up; min / median / max over the repeats.  The cost per iteration is the
difference of a run with --n_iter and one with 0 iterations (start constants, the first evaluation and the trace's first
column), divided by --n_iter.  Decode and check are the parent commit's code, measured here in the same process.  Needs a
GPU: there is nothing to measure without one."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread  # noqa: E402


def measure(title, jobs, repeats, n_iter, lines):
    lines.append(title)
    for L, (decode, check, top, S) in jobs:
        xyz = decode()
        relax = lambda k=n_iter: metrics.relax(xyz, top, n_iter=k)                                         # noqa: E731
        out = relax()                                           # first call: host tables, warm-up
        for fn in (decode, lambda: check(xyz), relax, lambda: relax(0)):
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        ed, ec = events(decode, repeats), events(lambda: check(xyz), repeats)
        er, e0 = events(relax, repeats), events(lambda: relax(0), repeats)
        again = relax()
        same = all(torch.equal(out[k], again[k]) for k in ("xyz", "trace_energy", "accepted"))
        g0, g1 = check(xyz), check(out["xyz"])
        med = statistics.median
        per_iter = (med(er) - med(e0)) / max(n_iter, 1)
        pairs = S * top.n_atoms * top.n_atoms                  # the full matrix, per evaluation
        lines += [f"  L={L:3d} n_atoms={top.n_atoms:4d} structures={S:3d}: clashes per structure {float(g0['clash'].double().mean()):.1f} -> "
                  f"{float(g1['clash'].double().mean()):.1f}, min_dist {float(g0['min_dist'].min()):.3f} -> {float(g1['min_dist'].min()):.3f} A, "
                  f"accepted {float(out['n_accepted'].double().mean()):.1f} of {n_iter}, energy {float(out['energy0'].mean()):.2f} -> "
                  f"{float(out['energy'].mean()):.2f}; repeat call bit-identical: {same}",
                  f"    decode tail          HIP events  {spread(ed)}",
                  f"    geometry check       HIP events  {spread(ec)}",
                  f"    relax, {n_iter:3d} iterations HIP events  {spread(er)}",
                  f"    relax,   0 iterations HIP events  {spread(e0)}",
                  f"    per iteration (evaluation + step): {per_iter * 1e3:.4f} ms  ({pairs / per_iter / 1e9:.1f} G ordered pairs/s)",
                  f"    relax / (decode tail + check), medians: {med(er) / (med(ed) + med(ec)):.2f}"]
    lines.append("")


def body(args, dev, lines):
    for title, jobs in decoded_sections(dev):
        measure(title, jobs, args.repeats, args.n_iter, lines)


if __name__ == "__main__":
    main("relax_cost", body, repeats=10, options=[("--n_iter", 200)], header=lambda args: (
        "", f"repeats: {args.repeats} (2 warm-up); times in ms per call; one call = one protein's structures; defaults "
            f"{metrics.RELAX_DEFAULTS}"))
