#!/usr/bin/env python3
"""What the essential dynamics of an ensemble cost on the device (metrics.mean_structure, covariance, pca;
csrc/pca_kernels.hip), beside the all-pairs RMSD of the same pool (metrics.rmsd_neighbours) and the float64 numpy route.

    python tools/pca_cost.py [--out profiles/pca_cost.txt] [--repeats 5]

Inputs: pools of (N, m) = (400, 87), (4 096, 129), (16 384, 129), (65 536, 129) and (4 096, 1 075): one blob of m atoms of
spread 5 A, ten collective modes of amplitudes 1.0 .. 0.2 A, 0.05 A of noise per coordinate, every structure moved by a
random rotation and translation, fp32; fixed seeds.
  fit            HIP events around one mean_structure call (moments, set-up, the batches of iterations with the host's one
                 read per batch), and that time over the iterations it took
  covariance     HIP events around the three launches of codlad_pca_covariance on the deviations of that fit; the float64
                 rate counts the lower triangle's N d (d + 1) flop (what is asked for, not the whole tiles that are computed)
                 against the MI355X's 78.6 TFLOP/s of float64 matrix peak; rmsd_matrix's product reaches 38 TFLOP/s
                 (profiles/cluster_cost.txt)
  eigen-solve    HIP events around the whole call for k = 10 (block of 18), and per iteration
  projection     HIP events around codlad_pca_project
  rmsd_neighbours the all-pairs superposed msd of the same pool, bitmap alone (same run)
  numpy          float64 on the host cores numpy's BLAS uses: D^T D / N of the device's deviations, and eigh of it where d <=
                 400 (the full spectrum, which is what numpy offers); the reference's fit is a Python loop and is not timed
Needs a GPU."""
import importlib
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402

P = importlib.import_module("codlad_amd.metrics.pca")      # the module: metrics.pca is the function of that name

PEAK_FP64 = 78.6e12
SHAPES = ((400, 87), (4096, 129), (16384, 129), (65536, 129), (4096, 1075))
K = 10


def pool(N, m, seed=21):
    rng = np.random.default_rng(seed + N + m)
    base = rng.standard_normal((m, 3)) * 5.0
    modes = np.linalg.qr(rng.standard_normal((3 * m, K)))[0].T
    amp = np.linspace(1.0, 0.2, K)
    x = base.reshape(-1)[None] + (rng.standard_normal((N, K)) * amp) @ modes + 0.05 * rng.standard_normal((N, 3 * m))
    q = rng.standard_normal((N, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, a, b, c = q.T
    R = np.stack((1 - 2 * (b * b + c * c), 2 * (a * b - w * c), 2 * (a * c + w * b), 2 * (a * b + w * c), 1 - 2 * (a * a + c * c),
                  2 * (b * c - w * a), 2 * (a * c - w * b), 2 * (b * c + w * a), 1 - 2 * (a * a + b * b)), 1).reshape(N, 3, 3)
    x = np.einsum("skc,src->skr", x.reshape(N, m, 3), R) + 10.0 * rng.standard_normal((N, 1, 3))
    return x.astype(np.float32)


def body(args, dev, lines):
    med = lambda ts: float(np.median(ts))                 # noqa: E731
    for N, m in SHAPES:
        d = 3 * m
        x = torch.from_numpy(pool(N, m)).to(dev)
        fit = lambda: metrics.mean_structure(x)           # noqa: E731
        f0 = fit()
        fit()
        t_fit = events(fit, args.repeats)
        lines.append(f"N = {N}, m = {m} (d = {d}): fit {f0['status']} in {f0['n_iter']} iterations")
        lines.append(f"  fit                  HIP events {spread(t_fit)}   = {med(t_fit) / f0['n_iter'] * 1e3:.3f} ms per iteration")
        x_, sel, n_sel = P._inputs.pool(x, None, "pca_cost", P.PCA_MAX_N)
        rec = P._fit(x_, sel, n_sel, None, -1, 1e-6, 100)
        D, _ = P._deviations(rec, True, True)
        cov_call = lambda: P._covariance(rec, D)          # noqa: E731
        cov, _corr, _tot = cov_call()
        again = cov_call()[0]
        same = torch.equal(cov.view(torch.int64), again.view(torch.int64)) and torch.equal(cov, cov.t())
        cov_call()
        t_cov = events(cov_call, args.repeats)
        flop = float(N) * d * (d + 1)
        lines.append(f"  covariance           HIP events {spread(t_cov)}   {flop:.3e} flop -> {flop / med(t_cov) / 1e12:.2f} TFLOP/s = "
                     f"{100 * flop / med(t_cov) / PEAK_FP64:.1f} % of the float64 matrix peak (repeat bit-identical and symmetric: {same})")
        eig = lambda: P._eigen(cov, K, 1e-10, 1000)       # noqa: E731
        ev, comps, _res, it, status = eig()
        eig()
        t_eig = events(eig, args.repeats)
        lines.append(f"  eigen-solve, k = {K}   HIP events {spread(t_eig)}   {status} in {it} iterations = {med(t_eig) / it * 1e3:.3f} ms per "
                     f"iteration; explained by the first three {' '.join(f'{float(v):.3f}' for v in (ev[:3] / cov.diagonal().sum()))}")
        proj = lambda: P._project(D, comps)               # noqa: E731
        proj()
        t_proj = events(proj, args.repeats)
        lines.append(f"  projection           HIP events {spread(t_proj)}")
        nb = lambda: metrics.rmsd_neighbours(x, 3.0)      # noqa: E731
        nb()
        t_nb = events(nb, max(2, args.repeats // 2))
        lines.append(f"  rmsd_neighbours      HIP events {spread(t_nb)}   (all {N * (N - 1) // 2} pairs of the same pool, bitmap alone)")
        Dh = D.cpu().numpy()
        t0 = time.perf_counter()
        Ch = Dh.T @ Dh / N
        t_np = time.perf_counter() - t0
        line = f"  numpy float64        D^T D / N {t_np * 1e3:.1f} ms"
        if d <= 400:
            t0 = time.perf_counter()
            np.linalg.eigh(Ch)
            line += f", eigh (full spectrum) {(time.perf_counter() - t0) * 1e3:.1f} ms"
        else:
            line += ", eigh not timed at this d"
        lines.append(line + f"   (OMP_NUM_THREADS = {os.environ.get('OMP_NUM_THREADS', 'unset')})")
        lines.append("")
        del x, D, cov, rec, Dh, Ch
        torch.cuda.empty_cache()
    lines.append("not measured: hardware counters, the kernels one by one, d = 4 096 at N = 65 536 (2.2 GB of chunk partials)")


def header(args):
    return "", f"repeats: {args.repeats} (2 warm-up); times in ms per call"


if __name__ == "__main__":
    main("pca_cost", body, repeats=5, header=header)
