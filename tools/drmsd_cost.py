#!/usr/bin/env python3
"""What the superposition-free dRMSD costs on the device (metrics.drmsd_neighbours, drmsd_matrix, drmsd_pairs;
csrc/drmsd_kernels.hip), beside the superposed route on the same pool and a torch float64 route.

    python tools/drmsd_cost.py [--out profiles/drmsd_cost.txt] [--repeats 5]

Inputs: random-walk chains of (N, m) = (400, 87), (4 096, 129), (16 384, 129), (4 096, 1 075) and (32, 4 325) with a 3.8 A
step, fixed seeds; min_sep = 1, every atom selected.
  dRMSD          HIP events around one whole call (the finite, norm, product and, with the split, finishing launches and
                 the allocations), 2 warm-up calls and the median of `repeats`: the bitmap alone (no N x N table exists)
                 and the float64 table
  product        useful: 2 flop per (structure pair of the upper triangle with its diagonal, pair of positions); executed:
                 2 * 256 * 4 flop per MFMA over the slots the kernel runs (windows on the diagonal are half empty, the last
                 window of a row is ragged), 16 wave tiles per block of 64 x 64 (10 on the diagonal) plus the 4 diagonal
                 wave tiles of the norm launch; both against the whole call's time (bitmap alone) - lower bounds of the
                 kernel's own rate - and against the MI355X's 78.6 TFLOP/s of float64.  The operand generation is inside
                 that time: the ratio to rmsd_matrix's rate on the same pool, same run, is what it costs
  rmsd_matrix    metrics.rmsd_neighbours on the same pool, bitmap alone and with the table, and its product rate by
                 tools/cluster_cost.py's count
  torch          float64, where the [N, P] table fits 4 GiB: the fp32 distances of every structure by indexed differences
                 (torch.cdist, batched or at 4 325 atoms, returned wrong and non-finite distances on the ROCm build this was
                 written on and is not used) into the table, then G + G^T - 2 D D^T by one matmul; median of 3 after one
                 warm-up, and its largest difference from the kernel
  check          the table against drmsd_pairs (the direct sum) on 3 000 random pairs: the largest relative difference
  pairs          drmsd_pairs of N pairs (structure i against structure 0), with and without the per-position rows
Needs a GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

PEAK_FP64 = 78.6e12
RMSD_MATRIX_TFLOPS = 38.0                               # profiles/cluster_cost.txt, N = 4096
SHAPES = ((400, 87), (4096, 129), (16384, 129), (4096, 1075), (32, 4325))
WINDOW, TABLE_LIMIT = 16, 4 << 30


def pool(N, m, seed=23):
    rng = np.random.default_rng(seed + N + m)
    step = rng.normal(size=(N, m, 3))
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    return (np.cumsum(step, axis=1) + rng.normal(0.0, 0.05, (N, m, 3))).astype(np.float32)


def slots_run(m, min_sep=1):
    """The pair slots the kernel multiplies: 32 per pair of window rows that holds a pair."""
    T, n = (m + WINDOW - 1) // WINDOW, 0
    for tr in range(T):
        for tc in range(tr, T):
            lmax = min((tc + 1) * WINDOW, m) - 1
            for k0 in range(tr * WINDOW, (tr + 1) * WINDOW, 2):
                if lmax - k0 < min_sep:
                    break
                n += 2 * WINDOW
    return n


def flops(N, m):
    P = m * (m - 1) // 2
    nb = (N + 63) // 64
    useful = 2.0 * P * (N * (N + 1) // 2)
    executed = 2.0 * 256 * slots_run(m) * (16 * nb * (nb - 1) // 2 + 10 * nb + 4 * nb)
    return P, useful, executed


def rmsd_flop(N, n):                                    # tools/cluster_cost.py product_flop
    nb = (N + 63) // 64
    return (16 * nb * (nb - 1) // 2 + 10 * nb) * 9 * 2.0 * 16 * 16 * 4 * ((n + 3) // 4)


def torch_route(x):
    N, m = x.shape[:2]
    iu = torch.triu_indices(m, m, 1, device=x.device)
    P = iu.shape[1]
    D = torch.empty(N, P, dtype=torch.float64, device=x.device)
    step = max(1, min(N, (256 << 20) // (12 * P)))
    for i0 in range(0, N, step):
        d = x[i0:i0 + step][:, iu[1]] - x[i0:i0 + step][:, iu[0]]
        D[i0:i0 + step] = (d * d).sum(-1).sqrt().double()
    G = (D * D).sum(1)
    return ((G[:, None] + G[None, :] - 2.0 * (D @ D.T)).clamp_(min=0.0) / P)


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    for N, m in SHAPES:
        x = torch.from_numpy(pool(N, m)).to(dev)
        P, useful, executed = flops(N, m)
        groups = metrics.drmsd._lib.lib().codlad_drmsd_groups(N, 0, m, 1)
        lines.append(f"N = {N}, m = {m}: P = {P} pairs of positions, {N * (N - 1) // 2} pairs of structures, {useful:.3e} useful flop, "
                     f"{executed:.3e} executed; {groups} workgroup(s) per block")
        cutoff = float(metrics.drmsd_pairs(x[:1], x[1:2], torch.tensor([[0, 0]])))
        bits_only = lambda: metrics.drmsd_neighbours(x, cutoff)                                        # noqa: E731
        table = lambda: metrics.drmsd_matrix(x, squared=True)                                         # noqa: E731
        a, b = bits_only(), bits_only()
        same = torch.equal(a["bits"], b["bits"])
        del a, b
        bits_only(), table()
        t_bits, t_table = events(bits_only, args.repeats), events(table, args.repeats)
        lines.append(f"  dRMSD, bitmap alone             HIP events {spread(t_bits)}   (a repeat is bit-identical: {same})")
        lines.append(f"  dRMSD, the N x N table          HIP events {spread(t_table)}   ({8.0 * N * N / 2 ** 20:.0f} MiB)")
        rate_u, rate_e = useful / med(t_bits) / 1e12, executed / med(t_bits) / 1e12
        lines.append(f"  product                         >= {rate_u:.2f} TFLOP/s useful, {rate_e:.2f} executed = {100 * rate_e * 1e12 / PEAK_FP64:.1f} % of "
                     f"the float64 peak (whole call, operand generation inside)")
        old_bits = lambda: metrics.rmsd_neighbours(x, cutoff)                                          # noqa: E731
        old_table = lambda: metrics.rmsd_neighbours(x, cutoff, return_matrix=True)                     # noqa: E731
        old_bits(), old_bits(), old_table()
        t_ob, t_ot = events(old_bits, args.repeats), events(old_table, args.repeats)
        rate_old = rmsd_flop(N, m) / med(t_ob) / 1e12
        lines.append(f"  rmsd_matrix, bitmap alone       HIP events {spread(t_ob)}   ({rate_old:.2f} TFLOP/s executed, whole call)")
        lines.append(f"  rmsd_matrix, with the table     HIP events {spread(t_ot)}")
        lines.append(f"  dRMSD / rmsd_matrix             {med(t_bits) / med(t_ob):.1f} x the time for {executed / rmsd_flop(N, m):.1f} x the flop; "
                     f"the dRMSD product runs at {rate_e / rate_old:.2f} of rmsd_matrix's rate here and {rate_e / RMSD_MATRIX_TFLOPS:.2f} of its "
                     f"{RMSD_MATRIX_TFLOPS:.0f} TFLOP/s")
        rnd = torch.randint(0, N, (3000, 2), generator=torch.Generator().manual_seed(N + m))
        rnd = rnd[rnd[:, 0] != rnd[:, 1]]
        direct, sq = metrics.drmsd_pairs(x, x, rnd, squared=True), table()
        rel = float(((sq[rnd[:, 0].to(dev), rnd[:, 1].to(dev)] - direct).abs() / direct).max())
        del sq
        lines.append(f"  check                           table against the pair route on {rnd.shape[0]} random pairs: largest relative difference {rel:.1e}")
        if 8 * N * P <= TABLE_LIMIT:
            ref = torch_route(x)
            diff = float((ref - table()).abs().max())
            del ref
            t_torch = events(lambda: torch_route(x), 3)
            ratio = med(t_torch) / med(t_table)
            lines.append(f"  torch float64 (table + matmul)  HIP events {spread(t_torch)}   ({8.0 * N * P / 2 ** 20:.0f} MiB table; largest |msd - kernel| "
                         f"{diff:.2e} A^2) -> the kernel's table takes {1 / ratio:.2f} x its time: {'faster' if ratio > 1 else 'SLOWER'}")
        else:
            lines.append(f"  torch float64 (table + matmul)  not run: the [N, P] table is {8.0 * N * P / 2 ** 30:.1f} GiB")
        idx = torch.arange(N)
        pairs = torch.stack((idx, torch.zeros_like(idx)), 1)
        plain = lambda: metrics.drmsd_pairs(x, x, pairs)                                               # noqa: E731
        per_pos = lambda: metrics.drmsd_pairs(x, x, pairs, per_position=True)                          # noqa: E731
        plain(), per_pos()
        lines.append(f"  drmsd_pairs, {N} pairs           HIP events {spread(events(plain, args.repeats))}")
        lines.append(f"  ... with per-position rows      HIP events {spread(events(per_pos, args.repeats))}")
        lines.append("")
        del x
        torch.cuda.empty_cache()
    lines.append("gram_kernel as built: fp32 panels of two window rows converted on the operand read, 16 x 16 windows with the row atoms "
                 "in LDS and the column atoms in registers, 74 VGPRs, 43.2 KiB of LDS, 8 waves")
    lines.append("not measured: float64 panels, other window sizes (not built); kernel times apart from the call (no profiler run); "
                 "pools above 16 384")


def header(args):
    return "", f"repeats: {args.repeats} (2 warm-up); times in ms per call"


if __name__ == "__main__":
    main("drmsd_cost", body, repeats=5, header=header)
