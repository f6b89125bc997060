#!/usr/bin/env python3
"""What the stereochemistry check (metrics.stereo_check, codlad_stereo_check) costs beside the geometry check
(metrics.geometry_check) on the same decoded structures.

    python tools/stereo_check_cost.py [--out profiles/stereo_check_cost.txt] [--repeats 20]

The shapes and the decoded input are those of tools/geometry_check_cost.py (cost_common's `job`):
(i)  the cfg2 decode output: the four synthetic PED proteins, 10 frames x 10 members = 100 structures each;
(ii) the largest cfg4 protein (505 residues, K4 decoder) x 32 members of one frame.
Both checks run on the SAME xyz tensor, alternating within a repeat.  Device time by HIP events around one call (the
launch and its memset), wall clock around the call and its one synchronisation; every shape is warmed up; min / median /
max over the repeats.  The site table of a topology is built once on the host and cached on it: the first call's wall
clock is reported apart.  There is no threshold: this tool reports, it does not judge.  Needs a GPU."""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread, wall  # noqa: E402


def measure(title, jobs, repeats, lines):
    lines.append(title)
    tot = {"stereo": 0.0, "geometry": 0.0}
    for L, (decode, geometry, top, S) in jobs:
        xyz = decode()
        geometry(xyz)                                             # its host tables are not this tool's subject
        t0 = time.perf_counter()
        ste = metrics.stereo_check(xyz, top)
        torch.cuda.synchronize()
        first = time.perf_counter() - t0                          # includes the host-side site table of the topology
        stereo = lambda: metrics.stereo_check(xyz, top)           # noqa: E731
        for _ in range(3):
            stereo(), geometry(xyz)
        torch.cuda.synchronize()
        es, eg = [], []
        for _ in range(repeats):                                  # alternating: both see the same machine state
            es += events(stereo, 1)
            eg += events(lambda: geometry(xyz), 1)
        ws, wg = wall(stereo, repeats, 3), wall(lambda: geometry(xyz), repeats, 3)
        again = stereo()
        same = all(torch.equal(ste[k].view(torch.int32) if ste[k].dtype == torch.float32 else ste[k],
                               again[k].view(torch.int32) if again[k].dtype == torch.float32 else again[k])
                   for k in ("values", "flags", "counts"))
        c = ste["counts"].double().mean(0).tolist()
        R = top.n_residues
        n_q = int((metrics.stereo_tables(top)[0] >= 0).all(-1).sum())
        gathered = S * n_q * 4 * 12 + S * R * (9 * 4 + 1)         # coordinate bytes asked for + values and flags written
        tot["stereo"] += statistics.median(es)
        tot["geometry"] += statistics.median(eg)
        lines += [f"  L={L:3d} residues={R:3d} n_atoms={top.n_atoms:4d} structures={S:3d} ({S * R} threads, {S * n_q} quantities)  "
                  f"mean per structure: " + " ".join(f"{k} {v:.1f}" for k, v in zip(metrics.STEREO_COUNTS, c)) +
                  f"; stereo_ok {float(ste['stereo_ok'].double().mean()):.2f}; repeat call bit-identical: {same}",
                  f"    stereo check   wall (incl. its one sync) {spread(ws)}",
                  f"    stereo check   HIP events                {spread(es)}  ({gathered / statistics.median(es) / 1e9:.1f} GB/s gathered + written)",
                  f"    geometry check wall (incl. its one sync) {spread(wg)}",
                  f"    geometry check HIP events                {spread(eg)}",
                  f"    stereo check first call (host table)     {first * 1e3:9.3f} ms",
                  f"    stereo / geometry (median HIP events): {statistics.median(es) / statistics.median(eg):.2f}"]
    lines += [f"  sum of medians (HIP events): stereo check {tot['stereo'] * 1e3:.3f} ms, geometry check {tot['geometry'] * 1e3:.3f} ms", ""]


def body(args, dev, lines):
    for title, jobs in decoded_sections(dev):
        measure(title, jobs, args.repeats, lines)


if __name__ == "__main__":
    main("stereo_check_cost", body)
