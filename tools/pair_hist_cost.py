#!/usr/bin/env python3
"""What the typed pair-distance histogram of an ensemble costs (metrics.pair_histogram: one sqrt and one integer add per
pair), what a profile costs once the histogram is there (metrics.saxs_profile_hist(hist=...)), and the exact Debye sum
(metrics.saxs_profile) on the same structures; and how far the histogram profile lies from the exact one.

    python tools/pair_hist_cost.py [--out profiles/pair_hist_cost.txt] [--repeats 10]

Inputs, as tools/saxs_cost.py builds them (the decode tail of seeded random weights):
(i)  the cfg2 decode output: the four synthetic PED proteins, 10 frames x 10 members = 100 structures each, at Q = 51;
(ii) the largest cfg4 protein (505 residues) x 32 members of one frame, at Q = 51 and at Q = 256.
r_max is the diagonal of the ensemble's bounding box rounded up (so no pair lies beyond it, at both bin widths); the device
side is timed by HIP events around the launches of one call, every shape warmed up; min / median / max over the repeats.
The deviation is the largest |I_hist - I_exact| / |I_exact| over the finite structures and all q, I_exact the Debye sum of
metrics.saxs_profile (float32 sinc, float64 sums), at dr = 0.5 and 0.25 A.  Needs a GPU."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import decoded_sections, events, main, metrics, spread  # noqa: E402


def measure(title, jobs, q_sizes, repeats, lines):
    lines.append(title)
    for L, (decode, _check, top, S) in jobs:
        xyz = decode()
        n = top.n_atoms
        ok = torch.isfinite(xyz).all(dim=2).all(dim=1)
        box = xyz[ok].reshape(-1, 3)
        r_max = float(math.ceil(float((box.max(0).values - box.min(0).values).norm()))) + 1.0
        lines.append(f"  L={L:3d} n_atoms={n:4d} structures={S:3d} ({S * n * (n - 1) // 2:.3e} pairs, "
                     f"{len(metrics.saxs_groups(top)[0])} types), r_max {r_max:.0f} A")
        hists = {}
        for dr in (0.5, 0.25):
            fn = lambda dr=dr: metrics.pair_histogram(xyz, top, dr=dr, r_max=r_max)                  # noqa: E731
            a, b = fn(), fn()
            hists[dr] = a
            same = all(torch.equal(a[k], b[k]) for k in ("H", "over", "d_bin"))
            for _ in range(3):
                fn()
            lines.append(f"    histogram dr = {dr:4.2f} ({a['H'].shape[2]:4d} bins)   HIP events {spread(events(fn, repeats))}; "
                         f"pairs beyond r_max {int(a['over'].clamp(min=0).sum())}, repeat call bit-identical: {same}")
        fn = lambda: metrics.pair_distribution(None, top, hist=hists[0.5])                             # noqa: E731
        for _ in range(3):
            fn()
        lines.append(f"    P(r) from the histogram, dr = 0.50       HIP events {spread(events(fn, repeats))}")
        for Q in q_sizes:
            q = np.linspace(0.0, 0.5, Q)
            exact_fn = lambda: metrics.saxs_profile(xyz, top, q=q)                                  # noqa: E731
            exact = exact_fn()
            for _ in range(2):
                exact_fn()
            lines.append(f"    Debye sum Q = {Q:3d} (saxs_profile)        HIP events {spread(events(exact_fn, repeats))}")
            for dr in (0.5, 0.25):
                fn = lambda dr=dr: metrics.saxs_profile_hist(None, top, q=q, hist=hists[dr])         # noqa: E731
                got = fn()
                for _ in range(3):
                    fn()
                keep = got["complete"] & exact["finite"]
                dev = ((got["I"][keep] - exact["I"][keep]).abs() / exact["I"][keep].abs()).max()
                lines.append(f"    profile from the histogram Q = {Q:3d}, dr = {dr:4.2f}  HIP events {spread(events(fn, repeats))}; "
                             f"complete {int(keep.sum())} of {S}, max |I_hist - I_exact| / I_exact {float(dev):.3e}")
        lines.append("")


def body(args, dev, lines):
    for k, (title, jobs) in enumerate(decoded_sections(dev)):
        measure(title, jobs, (51,) if k == 0 else (51, 256), args.repeats, lines)


if __name__ == "__main__":
    main("pair_hist_cost", body, repeats=10)
