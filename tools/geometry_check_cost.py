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
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, spread, wall  # noqa: E402


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


def body(args, dev, lines):
    for title, jobs in decoded_sections(dev):
        measure(title, jobs, args.repeats, lines)


if __name__ == "__main__":
    main("geometry_check_cost", body)
