#!/usr/bin/env python3
"""What clustering an ensemble costs on the device (metrics.rmsd_neighbours, rmsd_matrix, cluster_neighbours;
csrc/cluster_kernels.hip), beside the same table through the per-pair kernel of metrics.pairwise_rmsd.

    python tools/cluster_cost.py [--out profiles/cluster_cost.txt] [--repeats 10]

Inputs: pools of (N, n) = (400, 87), (1 024, 129), (4 096, 129), (4 096, 1 075) and (16 384, 129): eight families of n
atoms of spread 5 A, N / 16 blobs each a family plus 1.0 A noise, every member its blob plus 0.15 A noise, moved by a random
translation, every odd member 1000 A away; fixed seeds.  At 0.6 A the blobs are the clusters, at 3.0 A the families.
  all pairs      HIP events around the moments, operand and matrix kernels of one call, 3 warm-up calls and the median of
                 `repeats`: the bitmap alone (no N x N table exists) and with the float64 N x N table
  kernels        the device time of operand_kernel and matrix_kernel in one call of each kind (torch.profiler)
  product        2 * 9 * 256 * 4 flop per MFMA, 9 MFMAs per wave tile and block of 4 atoms, 16 wave tiles per block of 64 x 64
                 pairs (10 on the diagonal), against the matrix kernel's time (bitmap alone) and the MI355X's 78.6 TFLOP/s of
                 float64; the kernel's time also holds the per-pair tail, so this is a lower bound of the product's own rate
  tail           the two shapes with N = 4 096 differ in n alone: t = tail + product * n_pad gives both
  pairwise_rmsd  the same table through the per-pair kernel (x[:, None]), same run, N <= 4 096
  clustering     cluster_neighbours of the bitmap at two cut-offs, one giving a handful of clusters and one hundreds: the
                 clusters, the picks, the launches enqueued (2 + 128 per batch of 64 rounds) and the time of the whole call,
                 host reads of the number still active included
Needs a GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

PEAK_FP64 = 78.6e12
SHAPES = ((400, 87), (1024, 129), (4096, 129), (4096, 1075), (16384, 129))
CUTOFFS = (3.0, 0.6)


def pool(N, n, seed=11):
    rng = np.random.default_rng(seed + N + n)
    families = rng.standard_normal((8, n, 3)) * 5.0
    n_blob = max(8, N // 16)
    blobs = families[rng.integers(0, 8, n_blob)] + 1.0 * rng.standard_normal((n_blob, n, 3))
    x = blobs[rng.integers(0, n_blob, N)] + 0.15 * rng.standard_normal((N, n, 3))
    x += 10.0 * rng.standard_normal((N, 1, 3))
    x[1::2] += np.array([1000.0, -500.0, 250.0])
    return x.astype(np.float32)


def product_flop(N, n):
    nb = (N + 63) // 64
    tiles = 16 * nb * (nb - 1) // 2 + 10 * nb
    return tiles * 9 * 2.0 * 16 * 16 * 4 * ((n + 3) // 4)


def kernel_times(fn):
    """Device seconds of operand_kernel and matrix_kernel in one fn(), or None without a profiler."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for name in ("operand_kernel", "matrix_kernel"):
            ts = [(e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) * 1e-6
                  for e in prof.events() if name in e.name]
            if not ts or max(ts) <= 0:
                return None
            out[name] = max(ts)
        return out
    except Exception as e:                                # noqa: BLE001 (a profiler that is not there leaves the other figures)
        print(f"torch.profiler: {e}", file=sys.stderr)
        return None


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    matrix_time = {}
    for N, n in SHAPES:
        x = torch.from_numpy(pool(N, n)).to(dev)
        flop = product_flop(N, n)
        lines.append(f"N = {N}, n = {n}: {N * (N - 1) // 2} pairs, {flop:.3e} flop in the product")
        bits_only = lambda: metrics.rmsd_neighbours(x, CUTOFFS[0])                                    # noqa: E731
        with_table = lambda: metrics.rmsd_neighbours(x, CUTOFFS[0], return_matrix=True)               # noqa: E731
        a, b = bits_only(), with_table()
        same = torch.equal(a["bits"], b["bits"]) and torch.equal(a["bits"], bits_only()["bits"])
        del a, b
        for fn in (bits_only, with_table):
            for _ in range(3):
                fn()
        t_bits, t_table = events(bits_only, args.repeats), events(with_table, args.repeats)
        lines.append(f"  all pairs, bitmap alone         HIP events {spread(t_bits)}   (repeat and table-or-not bit-identical: {same})")
        lines.append(f"  all pairs, with the N x N table HIP events {spread(t_table)}   ({8.0 * N * N / 2 ** 20:.0f} MiB)")
        kt, kt2 = kernel_times(bits_only), kernel_times(with_table)
        if kt is None or kt2 is None:
            lines.append("  kernels                         no kernel times from torch.profiler on this build: the whole call stands in")
            t_mat = med(t_bits)
        else:
            t_mat = kt["matrix_kernel"]
            lines.append(f"  kernels                         operand {kt['operand_kernel'] * 1e3:.3f} ms, matrix {t_mat * 1e3:.3f} ms "
                         f"(with the table {kt2['matrix_kernel'] * 1e3:.3f} ms)")
        matrix_time[(N, n)] = t_mat
        lines.append(f"  product                         >= {flop / t_mat / 1e12:.2f} TFLOP/s = {100 * flop / t_mat / PEAK_FP64:.1f} % of the "
                     f"float64 peak (the tail's time included)")
        if N <= 4096:
            old = lambda: metrics.pairwise_rmsd(x[:, None])                                           # noqa: E731
            for _ in range(2):
                old()
            t_old = events(old, max(3, args.repeats // 3))
            ratio = med(t_old) / med(t_table)
            lines.append(f"  pairwise_rmsd(x[:, None])       HIP events {spread(t_old)}   -> the new route with the table is "
                         f"{ratio:.1f} x {'faster' if ratio > 1 else 'SLOWER'}")
        for cutoff in CUTOFFS:
            nb = metrics.rmsd_neighbours(x, cutoff)
            run = lambda: metrics.cluster_neighbours(nb["bits"], N, finite=nb["finite"])              # noqa: E731
            out = run()
            for _ in range(2):
                run()
            t_cl = events(run, args.repeats)
            batches = -(-out["rounds"] // metrics.CLUSTER_BATCH)
            lines.append(f"  clustering at {cutoff} A           {out['n_clusters']} clusters (largest {int(out['sizes'].max())}), {out['rounds']} picks, "
                         f"{batches} batch(es) = {batches * (2 + 2 * metrics.CLUSTER_BATCH)} launches: HIP events {spread(t_cl)}")
        lines.append("")
        del x
        torch.cuda.empty_cache()
    if (4096, 129) in matrix_time and (4096, 1075) in matrix_time:
        t1, t2 = matrix_time[(4096, 129)], matrix_time[(4096, 1075)]
        per_block = (t2 - t1) / (1076 // 4 - 132 // 4)
        tail = t1 - per_block * (132 // 4)
        lines.append(f"N = 4096, product and tail from the two atom counts: {per_block * 1e6:.2f} us per block of 4 atoms "
                     f"({product_flop(4096, 4) / per_block / 1e12:.1f} TFLOP/s), tail and stores {tail * 1e3:.3f} ms: the tail is "
                     f"{100 * tail / t1:.0f} % of the matrix kernel at n = 129 and {100 * tail / t2:.0f} % at n = 1075")
    lines.append("not measured: the member-walk update (not built), pools above 16 384 (N = 65 536: 512 MB of bits)")


def header(args):
    return "", f"repeats: {args.repeats} (3 warm-up); times in ms per call"


if __name__ == "__main__":
    main("cluster_cost", body, repeats=10, header=header)
