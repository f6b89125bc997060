#!/usr/bin/env python3
"""What the chain statistics of an ensemble cost on the device (metrics.chain_sums, gyration_tensor;
csrc/polymer_kernels.hip), beside a torch route to the same numbers and beside the typed pair histogram of the same
structures (the all-pairs kernel the project already has), all in one run.

    python tools/polymer_cost.py [--out profiles/polymer_cost.txt] [--repeats 5]

Inputs: random-walk chains of m beads with a step of 3.8 A, fp32, fixed seeds, (N, m) = (400, 87), (4 096, 129),
(65 536, 129), (1, 4 325), (32, 4 325): many small structures (a workgroup each) and few large ones (split across
workgroups).
  chain_sums        HIP events around the two launches of codlad_chain_sums, and the rate in pairs per second: N m (m - 1) / 2
  gyration_tensor   HIP events around codlad_ens_moments, codlad_gyration and the torch arithmetic of the shape numbers
  torch             float64 cdist of every structure with itself, the reciprocal off the diagonal, and the sum of every
                    diagonal: torch.diagonal(..).sum per separation up to m = 129 (2 (m - 1) small launches), one
                    index_add_ per sum over the flattened matrix at m = 4 325 (float atomics: the bits do not repeat);
                    in batches of 8 192 structures.  Then the largest relative difference to the kernel's sums.
  torch gyration    the centred second moments by einsum and torch.linalg.eigvalsh, float64
  pair_histogram    HIP events around codlad_pair_hist on the same structures: one atom type, bins of 0.5 A
Needs a GPU."""
import importlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

PD = importlib.import_module("codlad_amd.metrics.pair_distribution")

SHAPES = ((400, 87), (4096, 129), (65536, 129), (1, 4325), (32, 4325))
TORCH_BATCH = 8192
DIAGONAL_LOOP_MAX = 129


def chains(N, m, seed=41):
    rng = np.random.default_rng(seed + N + m)
    step = rng.standard_normal((N, m, 3)).astype(np.float32)
    step *= 3.8 / np.linalg.norm(step, axis=-1, keepdims=True)
    return np.cumsum(step, axis=1, dtype=np.float32)


def torch_route(x):
    """(sep_r2, sep_inv [N, m - 1], inv_sum [N]) by plain torch ops in float64."""
    N, m = x.shape[:2]
    r2s, invs = [], []
    idx = torch.arange(m, device=x.device)
    sep = (idx[None] - idx[:, None]).reshape(-1)                               # j - i of the flattened matrix
    upper = sep > 0
    for b in range(0, N, TORCH_BATCH):
        xb = x[b:b + TORCH_BATCH].to(torch.float64)
        D = torch.cdist(xb, xb)
        if m <= DIAGONAL_LOOP_MAX:
            r2s.append(torch.stack([(torch.diagonal(D, s, 1, 2) ** 2).sum(-1) for s in range(1, m)], 1))
            invs.append(torch.stack([(1.0 / torch.diagonal(D, s, 1, 2)).sum(-1) for s in range(1, m)], 1))
        else:
            flat = D.reshape(D.shape[0], -1)[:, upper]
            col = sep[upper] - 1
            r2s.append(torch.zeros(D.shape[0], m - 1, dtype=torch.float64, device=x.device).index_add_(1, col, flat * flat))
            invs.append(torch.zeros(D.shape[0], m - 1, dtype=torch.float64, device=x.device).index_add_(1, col, 1.0 / flat))
    r2s, invs = torch.cat(r2s), torch.cat(invs)
    return r2s, invs, invs.sum(1)


def torch_gyration(x):
    d = x.to(torch.float64)
    d = d - d.mean(1, keepdim=True)
    return torch.linalg.eigvalsh(torch.einsum("nka,nkb->nab", d, d) / x.shape[1])


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    for N, m in SHAPES:
        x = torch.from_numpy(chains(N, m)).to(dev)
        n_pairs = float(N) * m * (m - 1) / 2
        groups = metrics._lib.lib().codlad_chain_sums_groups(N, m)
        cs = lambda: metrics.chain_sums(x)                                                     # noqa: E731
        out = cs()
        again = cs()
        same = all(torch.equal(out[k], again[k]) for k in ("sep_r2", "sep_inv", "inv_sum"))
        t_c = events(cs, args.repeats)
        lines.append(f"N = {N}, m = {m}: {n_pairs:.3e} pairs, {groups} workgroup(s) per structure")
        lines.append(f"  chain_sums        HIP events {spread(t_c)}   {n_pairs / med(t_c) / 1e9:.1f} G pairs/s "
                     f"(repeat bit-identical: {same})")
        gy = lambda: metrics.gyration_tensor(x)                                                # noqa: E731
        g = gy()
        gy()
        t_g = events(gy, args.repeats)
        lines.append(f"  gyration_tensor   HIP events {spread(t_g)}")
        ref = lambda: torch_route(x)                                                           # noqa: E731
        r2s, invs, inv_sum = ref()
        ref()
        t_t = events(ref, args.repeats)
        how = "a sum per diagonal" if m <= DIAGONAL_LOOP_MAX else "index_add_"
        diff = max(float(((a - b).abs() / b.abs()).max()) for a, b in ((r2s, out["sep_r2"]), (invs, out["sep_inv"]), (inv_sum, out["inv_sum"])))
        lines.append(f"  torch             HIP events {spread(t_t)}   cdist, reciprocal, {how}; largest relative difference to "
                     f"the kernel {diff:.1e}; {med(t_t) / med(t_c):.1f} x the kernel's time")
        tg = lambda: torch_gyration(x)                                                         # noqa: E731
        e = tg()
        tg()
        t_tg = events(tg, args.repeats)
        ediff = float(((e - g["eig"]).abs().max(1).values / g["rg2"]).max())
        lines.append(f"  torch gyration    HIP events {spread(t_tg)}   einsum, eigvalsh; largest difference of an eigenvalue "
                     f"{ediff:.1e} of the trace; {med(t_tg) / med(t_g):.1f} x the kernel route's time")
        span = float((x.amax(1) - x.amin(1)).norm(dim=-1).max())
        r_max = float(min(2000.0, np.ceil(span)))
        tab = PD._hist_tables(np.zeros(m, dtype=np.int64), 1, 0.5, r_max, dev)
        ph = lambda: PD._hist_launch(x, tab)                                                   # noqa: E731
        ph()
        ph()
        t_p = events(ph, args.repeats)
        lines.append(f"  pair_histogram    HIP events {spread(t_p)}   one type, {tab['n_bins']} bins of 0.5 A; "
                     f"{med(t_p) / med(t_c):.1f} x chain_sums' time")
        lines.append("")
        del x, out, again, r2s, invs, g
        torch.cuda.empty_cache()
    lines.append("not measured: hardware counters, LDS bank conflicts, the two launches of chain_sums one by one")


def header(args):
    return "", f"repeats: {args.repeats} (2 warm-up); times in ms per call"


if __name__ == "__main__":
    main("polymer_cost", body, repeats=5, header=header)
