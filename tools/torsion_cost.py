#!/usr/bin/env python3
"""What the torsion-space analysis costs on the device (metrics.torsion_features, torsion_neighbours, torsion_matrix,
dihedral_pca, cluster_torsion; csrc/torsion_kernels.hip), beside a torch float64 route on the same pool.

    python tools/torsion_cost.py [--out profiles/torsion_cost.txt] [--repeats 5]

Inputs: random-walk chains of T + 3 beads with the quads (k, k + 1, k + 2, k + 3), (N, T) = (400, 172), (4 096, 256),
(16 384, 256) and (65 536, 256), fixed seeds.  At (65 536, 256) the bitmap alone is made: the table would be 34 GB.
  features       HIP events around one whole call of torsion_features, 2 warm-up calls and the median of `repeats`
  matrix         torsion_neighbours (features + norms + product, the bitmap alone: no N x N table exists) and
                 torsion_matrix (the float64 table); the product's rate from the time of the bitmap call less the
                 features call: useful 2 flop per (structure pair of the upper triangle with its diagonal, feature),
                 executed 2 * 256 * 4 flop per MFMA, 8 per chunk of 32 features, 16 wave tiles per block of 64 x 64 (10 on
                 the diagonal) plus the 4 diagonal wave tiles of the norm launch; against the MI355X's 78.6 TFLOP/s of
                 float64 and rmsd_matrix's 38 (profiles/cluster_cost.txt)
  torch          float64 on the device's own feature table: F @ F.T and the Gram combination (clamped, / T), where the
                 N x N table fits 8 GiB; median of 3 after one warm-up, and its largest difference from the kernel
  dihedral_pca   the whole call (10 components), and its stages one by one: features, mean + deviations, covariance,
                 eigen-solve, projection; beside torch.linalg.eigh of the same covariance
  cluster        cluster_torsion at a cut-off of 1.41 rad (random chains sit near sqrt(2): about half of the pairs are
                 neighbours), up to 16 384 structures
Needs a GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

PEAK_FP64 = 78.6e12
RMSD_MATRIX_TFLOPS = 38.0                               # profiles/cluster_cost.txt, N = 4096
SHAPES = ((400, 172), (4096, 256), (16384, 256), (65536, 256))
TABLE_LIMIT, CLUSTER_LIMIT = 8 << 30, 16384
KC = 32                                                 # features of a staged chunk (torsion_kernels.hip)


def pool(N, T, seed=29):
    rng = np.random.default_rng(seed + N + T)
    step = rng.normal(size=(N, T + 3, 3))
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    return (np.cumsum(step, axis=1) + rng.normal(0.0, 0.05, (N, T + 3, 3))).astype(np.float32)


def flops(N, T):
    nb = (N + 63) // 64
    useful = 2.0 * 2 * T * (N * (N + 1) // 2)
    executed = 2.0 * 256 * 4 * 8 * ((2 * T + KC - 1) // KC) * (16 * nb * (nb - 1) // 2 + 10 * nb + 4 * nb)
    return useful, executed


def torch_route(F, T):
    G = (F * F).sum(1)
    return (G[:, None] + G[None, :] - 2.0 * (F @ F.T)).clamp_(min=0.0) / T


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    tor = metrics.torsion
    for N, T in SHAPES:
        x = torch.from_numpy(pool(N, T)).to(dev)
        k = np.arange(T, dtype=np.int32)
        q = torch.from_numpy(np.stack([k, k + 1, k + 2, k + 3], 1)).to(dev)
        useful, executed = flops(N, T)
        lines.append(f"N = {N}, T = {T}: {N * (N - 1) // 2} pairs of structures, {useful:.3e} useful flop, {executed:.3e} executed")
        feats = lambda: metrics.torsion_features(x, q)                                                # noqa: E731
        bits_only = lambda: metrics.torsion_neighbours(x, q, 1.35)                                    # noqa: E731
        a, b = bits_only(), bits_only()
        same = torch.equal(a["bits"], b["bits"])
        del a, b
        feats(), feats()
        t_f, t_bits = events(feats, args.repeats), events(bits_only, args.repeats)
        lines.append(f"  torsion_features                HIP events {spread(t_f)}")
        lines.append(f"  torsion distance, bitmap alone  HIP events {spread(t_bits)}   (a repeat is bit-identical: {same})")
        prod = max(med(t_bits) - med(t_f), 1e-9)
        rate_u, rate_e = useful / prod / 1e12, executed / prod / 1e12
        lines.append(f"  product (bitmap - features)     {prod * 1e3:9.3f} ms: {rate_u:.2f} TFLOP/s useful, {rate_e:.2f} executed = "
                     f"{100 * rate_e * 1e12 / PEAK_FP64:.1f} % of the float64 peak, {rate_e / RMSD_MATRIX_TFLOPS:.2f} of rmsd_matrix's "
                     f"{RMSD_MATRIX_TFLOPS:.0f} TFLOP/s")
        if 8 * N * N <= TABLE_LIMIT:
            table = lambda: metrics.torsion_matrix(x, q, squared=True)                                # noqa: E731
            table(), table()
            t_table = events(table, args.repeats)
            lines.append(f"  torsion distance, N x N table   HIP events {spread(t_table)}   ({8.0 * N * N / 2 ** 20:.0f} MiB)")
            F = tor._features(x, q)[0]
            ref = torch_route(F, T)
            diff = float((ref - table()).abs().max())
            del ref
            t_torch = events(lambda: torch_route(F, T), 3)
            ratio = med(t_torch) / max(med(t_table) - med(t_f), 1e-9)
            lines.append(f"  torch float64 (F @ F.T + Gram)  HIP events {spread(t_torch)}   (largest |tmsd - kernel| {diff:.2e}) -> the "
                         f"kernel's table (less the features) takes {1 / ratio:.2f} x its time: {'faster' if ratio > 1 else 'SLOWER'}")
            del F
        else:
            lines.append(f"  torsion distance, N x N table   not made: {8.0 * N * N / 2 ** 30:.0f} GiB; torch float64 not run")
        whole = lambda: metrics.dihedral_pca(x, q, n_components=10)                                   # noqa: E731
        o = whole()
        whole()
        lines.append(f"  dihedral_pca, 10 components     HIP events {spread(events(whole, args.repeats))}   ({o['eig_iter']} iterations, "
                     f"{o['eig_status']})")
        F, fin = tor._features(x, q)
        mean, scal, D = tor._mean(F, fin, None, True)
        cov, total = tor._feature_covariance(D, None, fin, scal)
        comps = o["components"].reshape(10, -1).contiguous()
        for name, fn in (("mean + deviations", lambda: tor._mean(F, fin, None, True)),
                         ("covariance", lambda: tor._feature_covariance(D, None, fin, scal)),
                         ("eigen-solve", lambda: tor._eigen(cov, 10, 1e-10, 1000)),
                         ("projection", lambda: tor._project(D, comps)),
                         ("torch.linalg.eigh", lambda: torch.linalg.eigh(cov))):
            fn()
            lines.append(f"  ... {name:27s} HIP events {spread(events(fn, args.repeats))}")
        del F, D, cov, o
        if N <= CLUSTER_LIMIT:
            clus = lambda: metrics.cluster_torsion(x, q, 1.41)                                        # noqa: E731
            c = clus()
            lines.append(f"  cluster_torsion at 1.41 rad     HIP events {spread(events(clus, args.repeats))}   ({c['n_clusters']} clusters, "
                         f"{c['rounds']} rounds)")
            del c
        else:
            lines.append("  cluster_torsion                 not run: a random pool of this size has no clusters to find, only rounds")
        lines.append("")
        del x
        torch.cuda.empty_cache()
    lines.append("torsion_gram_kernel as built: float64 panels of 32 features with a row stride of 34 doubles, 8 waves, two 16 x 16 tiles "
                 "a wave, 35 KiB of LDS; 64 / 81 / 74 VGPRs (norm, one pool, two pools)")
    lines.append("not measured: kernel times apart from the call (no profiler run), LDS bank conflicts by counter, other chunk sizes")


def header(args):
    return "", f"repeats: {args.repeats} (2 warm-up); times in ms per call"


if __name__ == "__main__":
    main("torsion_cost", body, repeats=5, header=header)
