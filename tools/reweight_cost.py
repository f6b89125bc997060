#!/usr/bin/env python3
"""What maximum-entropy reweighting costs on the device (metrics.reweight, codlad_reweight_solve): a whole solve, one Newton
iteration, the covariance kernel's share of it and its float64 rate, and the float64 numpy solver of tests/reweight_ref.py
on the host beside them.

    python tools/reweight_cost.py [--out profiles/reweight_cost.txt] [--repeats 10]

Inputs: the Guinier-like family of tests/reweight_ref.py (Rg uniform in 15 .. 45 A, the experiment a Gaussian reweighting
in Rg plus 3 % noise) at (N, M) = (400, 51) - the bench's ensemble at the default q grid -, (4 096, 256) and (100 000, 512),
at theta = 10 and as a scan of 8 thetas from 1000 to 0.1 in one call.
  whole solve    HIP events around metrics.reweight(Y, y, sigma, theta) at the defaults (gtol 1e-9, max_iter 50), every
                 shape warmed up; the call enqueues max_iter rounds whatever the data, the rounds after the last
                 problem's end are launches that return at once, and their cost is part of the figure
  one iteration  (t(max_iter = 3) - t(max_iter = 1)) / 2 from mu = 0: two full rounds (weights, gradient, covariance,
                 Cholesky, line search), none of which converges
  covariance     the device time of cov_kernel's launches in one whole solve (torch.profiler), the n_iter longest of them
                 being the rounds that did work: their mean, their share of an iteration, and 2 * N * 4096 * tiles flop
                 per launch against the MI355X's 78.6 TFLOP/s of vector float64
  numpy          tests/reweight_ref.solve on the host's BLAS threads (OMP_NUM_THREADS as the environment sets it), for the
                 first two shapes
Needs a GPU."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cost_common import events, main, metrics, spread  # noqa: E402
from tests import reweight_ref as rr  # noqa: E402

PEAK_FP64_VECTOR = 78.6e12
SHAPES = ((400, 51), (4096, 256), (100000, 512))
SCAN = [float(t) for t in np.geomspace(1000.0, 0.1, 8)]


def cov_times(fn, n_launch):
    """Device seconds of every cov_kernel launch of one fn() -> the n_launch longest, or None when the profiler gives none."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        times = sorted((e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) * 1e-6
                       for e in prof.events() if "cov_kernel" in e.name)
    except Exception as e:                                # noqa: BLE001 (a profiler that is not there leaves the other figures)
        print(f"torch.profiler: {e}", file=sys.stderr)
        return None
    return times[-n_launch:] if len(times) >= n_launch and n_launch else None


def body(args, dev, lines):
    for N, M in SHAPES:
        c = rr.case(N, M)
        Y = torch.from_numpy(c["Y"].copy()).to(dev)
        tiles = ((M + 63) // 64) * ((M + 63) // 64 + 1) // 2
        lines.append(f"N = {N}, M = {M} ({tiles} tiles of the lower triangle, {2.0 * N * 4096 * tiles:.3e} flop per covariance)")
        for label, theta in (("theta 10", 10.0), ("scan of 8 thetas", SCAN)):
            fn = lambda theta=theta, **kw: metrics.reweight(Y, c["y"], c["sigma"], theta, **kw)      # noqa: E731
            out = fn()
            again = fn()
            same = all(torch.equal(out[k], again[k]) for k in ("mu", "w", "mean", "chi2", "s_rel"))
            n_iter, status = out["n_iter"].tolist(), out["status"].tolist()
            for _ in range(3):
                fn()
            whole = events(fn, args.repeats)
            t1 = events(lambda: fn(max_iter=1), args.repeats)
            t3 = events(lambda: fn(max_iter=3), args.repeats)
            per_iter = (float(np.median(t3)) - float(np.median(t1))) / 2
            lines.append(f"  {label}: Newton steps {n_iter}, status {status}, repeat call bit-identical: {same}")
            lines.append(f"    whole solve (max_iter 50)   HIP events {spread(whole)}")
            lines.append(f"    one iteration               {per_iter * 1e3:9.3f} ms   (max_iter 3: {float(np.median(t3)) * 1e3:.3f}, max_iter 1: "
                         f"{float(np.median(t1)) * 1e3:.3f} ms)")
            cov = cov_times(fn, max(n_iter))
            if cov is None:
                lines.append("    covariance kernel           no kernel times from torch.profiler on this build")
            else:
                mean = float(np.mean(cov))
                P = len(n_iter)
                done = sum(n_iter) / max(n_iter)          # the problems still running, averaged over the launches that worked
                lines.append(f"    covariance kernel           {mean * 1e3:9.3f} ms per working launch ({len(cov)} of them; {P} problem(s) a "
                             f"launch, {done:.2f} still running on average): {100 * mean / per_iter:.0f} % of an iteration, "
                             f"{2.0 * N * 4096 * tiles * done / mean / 1e12:.2f} TFLOP/s = "
                             f"{100 * 2.0 * N * 4096 * tiles * done / mean / PEAK_FP64_VECTOR:.1f} % of the vector float64 peak")
        if N <= 4096:
            for label, thetas in (("theta 10", [10.0]), ("scan of 8 thetas", SCAN)):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    its = [rr.solve(c["Y"], c["y"], c["sigma"], th)["n_iter"] for th in thetas]
                    ts.append(time.perf_counter() - t0)
                lines.append(f"  numpy float64 on the host, {label}: min {min(ts) * 1e3:.1f} ms of 3 (Newton steps {its}; "
                             f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')})")
        lines.append("")


def header(args):
    return "", f"repeats: {args.repeats} (3 warm-up); times in ms per call; one call = every theta of the line"


if __name__ == "__main__":
    main("reweight_cost", body, repeats=10, header=header)
