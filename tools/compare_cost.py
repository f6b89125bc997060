#!/usr/bin/env python3
"""What comparing two ensembles costs on the device (metrics.distance_histogram, column_histogram, histogram_divergence;
csrc/compare_kernels.hip), beside a torch route to the same distance histograms.

    python tools/compare_cost.py [--out profiles/compare_cost.txt] [--repeats 5]

Inputs: pools of (N, m) = (400, 87), (4 096, 129), (65 536, 129) and (4 096, 505): one blob of m atoms of spread 8 A with
1 A of noise per coordinate, fp32, fixed seeds; 50 bins up to the default r_max.
  distance histogram   HIP events around the three launches of codlad_dist_hist (fill, finite, the pair tiles), and the rate
                       in distances binned per second: N m (m - 1) / 2 of them
  column histogram     HIP events around codlad_column_hist on a table [N, 7 m] of angles (what the torsions of an m-residue
                       protein are), 36 periodic bins
  divergence           HIP events around codlad_hist_divergence on two distance tables [P, 52]
  torch                at the first two shapes: cdist per structure batch, the bin of every distance by the same float32
                       multiply and truncation, and one scatter_add into the [P, 52] table - the whole [N, P] index
                       tensor is materialised, which is why the larger shapes are not run
Needs a GPU."""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

C = importlib.import_module("codlad_amd.metrics.compare")

SHAPES = ((400, 87), (4096, 129), (65536, 129), (4096, 505))
TORCH_SHAPES = SHAPES[:2]
N_BINS = 50


def pool(N, m, seed=31):
    rng = np.random.default_rng(seed + N + m)
    return (rng.standard_normal((1, m, 3)) * 8.0 + rng.standard_normal((N, m, 3))).astype(np.float32)


def torch_route(x, inv_dr, n_bins):
    """H int32 [P, n_bins + 2] by plain torch ops."""
    N, m = x.shape[:2]
    i, j = torch.triu_indices(m, m, 1, device=x.device)
    t = torch.cdist(x, x)[:, i, j] * inv_dr                                  # [N, P] float32
    col = torch.where(t < n_bins, 1 + t.to(torch.int64), torch.full_like(t, n_bins + 1, dtype=torch.int64))
    H = torch.zeros(i.numel(), n_bins + 2, dtype=torch.int32, device=x.device)
    H.scatter_add_(1, col.t().contiguous(), torch.ones(i.numel(), N, dtype=torch.int32, device=x.device))
    return H


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    for N, m in SHAPES:
        x = torch.from_numpy(pool(N, m)).to(dev)
        x_, sel, n_sel, _m = C._pool(x, None, "compare_cost")
        r_max = C._default_r_max(float(C._box_diagonal(x_, None)), "compare_cost")
        n_bins, r_max, inv_dr = C._grid(None, r_max, N_BINS, "compare_cost")
        dist = lambda: C._dist_launch(x_, sel, n_sel, m, inv_dr, n_bins, "compare_cost")      # noqa: E731
        H, _fin, n_counted = dist()
        again = dist()[0]
        same = torch.equal(H, again) and bool((H.sum(1) == n_counted).all())
        dist()
        t_d = events(dist, args.repeats)
        n_dist = float(N) * m * (m - 1) / 2
        lines.append(f"N = {N}, m = {m}: P = {m * (m - 1) // 2} pairs, {n_bins} bins up to {r_max:.0f} A")
        lines.append(f"  distance histogram   HIP events {spread(t_d)}   {n_dist:.3e} distances -> {n_dist / med(t_d) / 1e9:.1f} G/s "
                     f"(repeat bit-identical, rows sum to n_counted: {same})")
        ang = torch.rand(N, 7 * m, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(N + m)) * 360 - 180
        colh = lambda: metrics.column_histogram(ang, -180.0, 180.0, 36, periodic=True)         # noqa: E731
        colh()
        colh()
        t_c = events(colh, args.repeats)
        lines.append(f"  column histogram     HIP events {spread(t_c)}   [{N}, {7 * m}] float64, 36 periodic bins")
        H2 = torch.roll(H, 1, 0).contiguous()
        div = lambda: metrics.histogram_divergence(H, H2)                                      # noqa: E731
        div()
        div()
        t_v = events(div, args.repeats)
        lines.append(f"  divergence           HIP events {spread(t_v)}   two tables [{H.shape[0]}, {H.shape[1]}]")
        if (N, m) in TORCH_SHAPES:
            ref = lambda: torch_route(x_, inv_dr, n_bins)                                      # noqa: E731
            Ht = ref()
            ref()
            t_t = events(ref, args.repeats)
            lines.append(f"  torch                HIP events {spread(t_t)}   cdist + truncation + scatter_add; differs from the "
                         f"kernel in {int((Ht != H).sum())} of {H.numel()} counts (cdist rounds its own way)")
        else:
            lines.append("  torch                not run at this shape (an [N, P] int64 index tensor)")
        lines.append("")
        del x, x_, H, H2, ang
        torch.cuda.empty_cache()
    lines.append("not measured: hardware counters, LDS bank conflicts, the three launches of a call one by one")


def header(args):
    return "", f"repeats: {args.repeats} (2 warm-up); times in ms per call"


if __name__ == "__main__":
    main("compare_cost", body, repeats=5, header=header)
