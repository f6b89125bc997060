"""Maximum-entropy reweighting on the device (codlad_amd/csrc/reweight_kernels.hip through codlad_amd.metrics) against
tests/reweight_ref.py.  The device's mu is not held to the host solver's bits: Gamma is strictly convex with H >= theta I,
so a mu is within |g(mu)|_2 / theta of the minimiser, and the tests evaluate g at the device's mu in np.longdouble - the
stop rule itself, in independent arithmetic.  Every other output is a function of mu and is held to the longdouble
evaluation at the device's mu within bounds derived from N, M and 2^-52 (test_outputs_are_consistent_with_mu).  Sums have
one order on the device, so repeats, batches and excluded rows are held to the bit."""

import numpy as np
import pytest

from codlad_amd import metrics
from tests import reweight_ref as rr
from tests.test_saxs import _cli, dev

pytestmark = pytest.mark.gpu
GTOL = 1e-9
EPS = rr.EPS
OUTPUTS = ("mu", "w", "mean", "chi2_prior", "chi2", "s_rel", "phi_eff", "n_iter", "status", "used")
_SOLVED = {}


def solved(N, M):
    """reweight of case (N, M) at the four thetas in one call, computed once and shared -> dict of numpy arrays."""
    if (N, M) not in _SOLVED:
        c = rr.case(N, M)
        out = metrics.reweight(dev(c["Y"]), c["y"], c["sigma"], list(rr.THETAS))
        _SOLVED[(N, M)] = {k: v.cpu().numpy() for k, v in out.items()}
        for v in _SOLVED[(N, M)].values():
            v.setflags(write=False)
    return _SOLVED[(N, M)]


def same_bits(a, b, keys=OUTPUTS):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True) for k in keys)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("N,M", rr.SHAPES, ids=lambda v: str(v))
def test_device_mu_meets_the_stop_rule_in_longdouble(N, M):
    """status 0, and |g|_inf / gscale at the device's mu, in np.longdouble, <= gtol + 4 * |rel_ld - rel_64| of the float64
    reference on the same case (the arithmetic's own deviation between a float64 and a longdouble evaluation of the rule).
    Then |mu_dev - mu_ref|_2 <= (|g_dev|_2 + |g_ref|_2) / theta by strong convexity, both gradients in longdouble (plus
    sqrt(M) gscale 2^-60 / theta for the longdouble evaluation's own rounding)."""
    c, out = rr.case(N, M), solved(N, M)
    shown = []
    for t, theta in enumerate(rr.THETAS):
        ref = rr.reference(N, M, theta)
        assert out["status"][t] == 0 and 0 <= out["n_iter"][t] <= 50, (theta, out["status"][t], out["n_iter"][t])
        ev = rr.evaluate(c["Y"], c["y"], c["sigma"], theta, out["mu"][t])
        rel = float(np.abs(ev["g"]).max() / ev["gscale"])
        g2 = float(np.sqrt((ev["g"] ** 2).sum()))
        allow = 4 * abs(ref["rel_ld"] - ref["rel_64"])
        dist = float(np.sqrt(((out["mu"][t] - ref["mu"]) ** 2).sum()))
        limit = (g2 + ref["g2_ld"]) / theta + np.sqrt(M) * float(ev["gscale"]) * 2.0 ** -60 / theta
        shown.append(f"theta {theta:g}: {out['n_iter'][t]} it (ref {ref['n_iter']}), rel {rel:.2e} (ref {ref['rel_ld']:.2e}, allowance "
                     f"{allow:.1e}), |mu - mu_ref| {dist:.2e} <= {limit:.2e}")
        assert rel <= GTOL + allow, (theta, rel, allow)
        assert dist <= limit, (theta, dist, limit)
    print(f"({N}, {M}) " + "; ".join(shown))


@pytest.mark.parametrize("N,M", rr.SHAPES, ids=lambda v: str(v))
def test_outputs_are_consistent_with_mu(N, M):
    """w, mean, chi2, chi2_prior, s_rel and phi_eff against their np.longdouble values at the device's mu.  With eps = 2^-52
    (twice the unit roundoff, which pays for the second-order terms), every bound from the operations the header states:
      a_j   = log w0_j - sum_k mu_k (c U_jk - v_k): M products and sums, three roundings in each z_jk, the log:
              |da_j| <= D = (M + 8) eps max_j (|log w0_j| + sum_k |mu_k| (|c U_jk| + |v_k|))
      w_j   = exp(a_j - max) / Z: the exponent's error D twice (in e_j and in Z), the sum of N positive terms, exp, divide:
              |dw_j| <= Bw w_j, Bw = 2 D + (N + 8) eps
      mean  = sigma_k sum_j w_j U_jk:  |dmean_k| <= (Bw + (N + 4) eps) sum_j w_j |Y_jk|
      r_k   = c <U_k> - v_k:           |dr_k| <= (Bw + (N + 6) eps) (|c| sum_j w_j |U_jk| + |v_k|)
      chi2  = sum_k r_k^2 / (M - 1):   |dchi2| <= sum_k (2 |r_k| dr_k + dr_k^2) / (M - 1) + (M + 4) eps chi2
              (chi2_prior: the same with the prior's weights, whose Bw is (N + 8) eps)
      s_rel = sum_j w_j (log w_j - log w0_j), T = sum_j w_j (|log w_j| + |log w0_j|):
              |ds| <= Bs = Bw (1 + T) + (N + 8) eps T        (dw in the factor and inside the log, the logs, the sum)
      phi   = exp(-s_rel):             |dphi| <= (Bs + 4 eps) phi
    Prints the largest measured deviation over its bound."""
    c, out = rr.case(N, M), solved(N, M)
    f = np.longdouble
    sig = c["sigma"].astype(f)
    U, v = c["Y"].astype(f) / sig, c["y"].astype(f) / sig
    worst = {}

    def note(name, err, bound):
        ratio = float(np.max(np.asarray(err, dtype=f) / np.maximum(np.asarray(bound, dtype=f), np.finfo(f).tiny)))
        worst[name] = max(worst.get(name, 0.0), ratio)
        assert ratio <= 1.0, (name, ratio)

    for t, theta in enumerate(rr.THETAS):
        mu = out["mu"][t].astype(f)
        ev = rr.evaluate(c["Y"], c["y"], c["sigma"], theta, out["mu"][t])
        logp0 = np.log(ev["p0"])
        D = (M + 8) * EPS * float((np.abs(logp0) + (np.abs(U) + np.abs(v)) @ np.abs(mu)).max())
        Bw = 2 * D + (N + 8) * EPS
        assert Bw < 1e-3                                   # the first-order bounds above mean something
        note("w", np.abs(out["w"][t] - ev["w"]), Bw * ev["w"])
        assert abs(float(out["w"][t].sum()) - 1.0) <= 2 * N * EPS and (out["w"][t] >= 0).all()
        note("mean", np.abs(out["mean"][t] - ev["mean"]), (Bw + (N + 4) * EPS) * (ev["w"] @ np.abs(c["Y"].astype(f))))
        for key, w, B in (("chi2", ev["w"], Bw), ("chi2_prior", ev["p0"], (N + 8) * EPS)):
            if M == 1:
                assert out[key][t] == 0.0
                continue
            r = w @ U - v
            dr = (B + (N + 6) * EPS) * (w @ np.abs(U) + np.abs(v))
            note(key, abs(out[key][t] - ev[key]), (2 * np.abs(r) * dr + dr * dr).sum() / (M - 1) + (M + 4) * EPS * ev[key])
        pos = ev["w"] > 0
        T = float((ev["w"][pos] * (np.abs(np.log(ev["w"][pos])) + np.abs(logp0[pos]))).sum())
        Bs = Bw * (1 + T) + (N + 8) * EPS * T
        note("s_rel", abs(out["s_rel"][t] - ev["s_rel"]), Bs)
        note("phi_eff", abs(out["phi_eff"][t] - ev["phi_eff"]), (Bs + 4 * EPS) * ev["phi_eff"])
        assert 0.0 < out["phi_eff"][t] <= 1.0 + Bs
        assert out["used"].all()
    print(f"({N}, {M}) largest deviation / bound: " + ", ".join(f"{k} {r:.2e}" for k, r in worst.items()))


def test_bits_repeat_and_do_not_depend_on_the_batch():
    """Two calls give the same bits; a theta solved alone and inside the list of four gives the same bits in every output;
    a permutation of the thetas permutes the outputs.  On (257, 64) - more than one block of rows, one tile - and on
    (1000, 129): four blocks, two chunks, tiles with an edge."""
    for N, M in ((257, 64), (1000, 129)):
        c, first = rr.case(N, M), solved(N, M)
        Y = dev(c["Y"])
        again = host(metrics.reweight(Y, c["y"], c["sigma"], list(rr.THETAS)))
        assert same_bits(first, again)
        for t, theta in enumerate(rr.THETAS):
            alone = host(metrics.reweight(Y, c["y"], c["sigma"], theta))
            assert alone["mu"].shape == (1, M) and alone["w"].shape == (1, N)
            for k in OUTPUTS:
                want = first[k] if k == "used" else first[k][t:t + 1]
                assert np.array_equal(alone[k], want), (N, M, theta, k)
        perm = [2, 0, 3, 1]
        mixed = host(metrics.reweight(Y, c["y"], c["sigma"], [rr.THETAS[i] for i in perm]))
        for k in OUTPUTS:
            assert np.array_equal(mixed[k], first[k] if k == "used" else first[k][perm]), (N, M, k)


def test_excluded_rows_get_weight_zero_and_add_exact_zeros():
    """Rows with w0 = 0, a NaN / +inf / -inf in Y or a NaN in w0 get weight exactly 0 and used = 0, and the rest of every
    output has the bits of two other solves of the same layout: one whose excluded rows hold ordinary numbers and w0 = 0, one
    whose excluded rows hold 1e300 and w0 = 0 - an excluded row adds exact zeros to every sum, whatever it holds.  (The
    blocks of 256 rows are fixed by N, so the comparison keeps the rows in place; against the COMPACTED problem, whose
    blocks differ, mu is held to the strong-convexity bound instead.)  All rows excluded: status 4 and NaN."""
    N, M = 300, 51
    c = rr.case(N, M)
    rows = {"w0": [3, 100], "nan": [7], "pinf": [255], "ninf": [256], "w0nan": [299]}
    bad = sorted(sum(rows.values(), []))
    rng = np.random.Generator(np.random.PCG64(9))
    prior = rng.uniform(0.5, 1.5, N)
    Y, w0 = c["Y"].copy(), prior.copy()
    w0[rows["w0"]] = 0.0
    Y[7, 5], Y[255, 0], Y[256, 50] = np.nan, np.inf, -np.inf
    w0[299] = np.nan
    thetas = [10.0, 1.0]
    got = host(metrics.reweight(dev(Y), c["y"], c["sigma"], thetas, w0=dev(w0)))
    assert (got["status"] == 0).all()
    assert (got["w"][:, bad] == 0.0).all() and not got["used"][bad].any() and got["used"].sum() == N - len(bad)
    keep = np.setdiff1d(np.arange(N), bad)
    assert (got["w"][:, keep] > 0).all()
    w0_clean = prior.copy()
    w0_clean[bad] = 0.0
    for fill in (None, 1e300):
        Y2 = c["Y"].copy()
        if fill is not None:
            Y2[bad] = fill
        other = host(metrics.reweight(dev(Y2), c["y"], c["sigma"], thetas, w0=dev(w0_clean)))
        assert same_bits(got, other), fill
    small = host(metrics.reweight(dev(c["Y"][keep]), c["y"], c["sigma"], thetas, w0=dev(prior[keep])))
    for t, theta in enumerate(thetas):
        ev_a = rr.evaluate(c["Y"][keep], c["y"], c["sigma"], theta, got["mu"][t], w0=prior[keep])
        ev_b = rr.evaluate(c["Y"][keep], c["y"], c["sigma"], theta, small["mu"][t], w0=prior[keep])
        limit = float(np.sqrt((ev_a["g"] ** 2).sum()) + np.sqrt((ev_b["g"] ** 2).sum())) / theta + \
            np.sqrt(M) * float(ev_a["gscale"]) * 2.0 ** -60 / theta
        dist = float(np.sqrt(((got["mu"][t] - small["mu"][t]) ** 2).sum()))
        print(f"theta {theta:g}: |mu - mu_compacted| {dist:.2e} <= {limit:.2e}")
        assert small["status"][t] == 0 and dist <= limit
    none = host(metrics.reweight(dev(Y), c["y"], c["sigma"], thetas, w0=dev(np.zeros(N))))
    assert (none["status"] == 4).all() and (none["n_iter"] == 0).all() and not none["used"].any()
    for k in ("mu", "w", "mean", "chi2", "chi2_prior", "s_rel", "phi_eff"):
        assert np.isnan(none[k]).all(), k
    nan_rows = c["Y"].copy()
    nan_rows[:, 1] = np.nan
    assert (host(metrics.reweight(dev(nan_rows), c["y"], c["sigma"], 1.0))["status"] == 4).all()


def test_statuses_cap_and_warm_start():
    N, M, theta = 257, 64, 0.1
    c, full = rr.case(N, M), solved(N, M)
    t = rr.THETAS.index(theta)
    assert full["n_iter"][t] > 1
    Y = dev(c["Y"])
    capped = host(metrics.reweight(Y, c["y"], c["sigma"], theta, max_iter=1))
    assert capped["status"].tolist() == [1] and capped["n_iter"].tolist() == [1]
    assert np.isfinite(capped["w"]).all() and abs(capped["w"].sum() - 1.0) <= 2 * N * EPS and np.isfinite(capped["mu"]).all()
    warm = host(metrics.reweight(Y, c["y"], c["sigma"], theta, mu0=dev(full["mu"][t])))
    assert warm["status"].tolist() == [0] and warm["n_iter"].tolist() == [0]
    for k in ("mu", "w", "mean", "chi2", "chi2_prior", "s_rel", "phi_eff"):
        assert np.array_equal(warm[k][0], full[k][t]), k
    both = host(metrics.reweight(Y, c["y"], c["sigma"], [theta, 10.0], mu0=dev(np.stack([full["mu"][t], np.zeros(M)]))))
    assert both["n_iter"].tolist() == [0, int(full["n_iter"][rr.THETAS.index(10.0)])]


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around reweight and weighted_mean: the results have the same bits under the three fills of every
    buffer the package allocates (the scratch with U, the partials, the covariance tiles and the matrix among them), every
    element of every output is written, no zone byte changes.  (300, 51): two blocks of rows, one tile with an edge, M
    padded from 51 to 64; (100, 200): N < M, ten tiles; with excluded rows; and the problem without a usable row."""
    import torch
    from tests.test_buffer_discipline import hold
    a, b = rr.case(300, 51), rr.case(100, 200)
    w0 = np.ones(300)
    w0[[2, 299]] = 0.0
    Ya = a["Y"].copy()
    Ya[17, 3] = np.nan

    def case(g):
        one = metrics.reweight(g(torch.from_numpy(Ya), "Y_a"), a["y"], a["sigma"], [10.0, 1.0], w0=g(torch.from_numpy(w0), "w0"))
        two = metrics.reweight(g(torch.from_numpy(b["Y"].copy()), "Y_b"), b["y"], b["sigma"], [1.0, 1000.0])      # two thetas a call:
        none = metrics.reweight(g(torch.from_numpy(Ya), "Y_none"), a["y"], a["sigma"], [1.0, 10.0],              # memcheck poisons no
                                w0=g(torch.from_numpy(np.zeros(300)), "w0_none"))                                  # one-element int buffer
        avg = metrics.weighted_mean(g(torch.from_numpy(b["Y"].copy()), "values"), two["w"])
        out = {f"{tag}_{k}": o[k] for tag, o in (("one", one), ("two", two), ("none", none)) for k in OUTPUTS}
        out["avg"] = avg
        return out, list(one["status"].tolist()) + list(two["status"].tolist()) + [int(v) - 4 for v in none["status"].tolist()]
    hold("reweight", case)


def _saxs_ensemble():
    """65 structures of a 32-residue topology: one random coil per structure, swollen or shrunk by a factor in 0.75 .. 1.35,
    and a curve made from a known reweighting in that factor, in another unit (x 2.5) with 1 % noise."""
    from codlad_amd.utils.cg_input import template_topology
    names = ["MET", "ALA", "PRO", "TRP", "GLY", "SER", "LYS", "HIS", "THR", "ARG", "CYS", "ASP", "TYR", "GLN", "LEU", "GLU"] * 2
    top = template_topology(names)
    rng = np.random.Generator(np.random.PCG64(65))
    S = 65
    swell = rng.uniform(0.75, 1.35, S)
    x = (rng.uniform(-14, 14, (S, top.n_atoms, 3)) * swell[:, None, None]).astype(np.float32)
    prof = metrics.saxs_profile(dev(x), top)
    I = prof["I"].cpu().numpy()
    wt = np.exp(-0.5 * ((swell - 1.15) / 0.08) ** 2)
    wt /= wt.sum()
    clean = 2.5 * (wt @ I)
    sigma = 0.01 * np.abs(clean) + 1e-4 * clean[0]
    curve = clean + sigma * rng.standard_normal(clean.shape[0])
    return prof, I, curve, sigma, swell, wt


def test_saxs_path_fits_the_scale_and_lowers_chi2():
    prof, I, curve, sigma, swell, wt = _saxs_ensemble()
    thetas = [100.0, 10.0, 1.0]
    out = metrics.saxs_reweight(prof["I"], prof["q"], curve, sigma, thetas, finite=prof["finite"])
    o = host(out)
    print("saxs_reweight: " + "; ".join(
        f"theta {th:g}: scale {o['scale'][t]:.6f} h {o['scale_residual'][t]:.1e} {o['rounds'][t]} rounds {o['n_iter'][t]} steps chi2 "
        f"{o['chi2_prior'][t]:.4g} -> {o['chi2'][t]:.4g} phi {o['phi_eff'][t]:.3f} <swell> {float(o['w'][t] @ swell):.3f}" for t, th in enumerate(thetas)))
    assert o["scale_converged"].all() and (o["status"] == 0).all() and (o["rounds"] <= 40).all()
    assert (np.abs(o["scale_residual"]) <= 1e-9 * np.abs(o["scale"])).all()
    assert (o["chi2"] < o["chi2_prior"]).all() and (np.abs(o["w"].sum(axis=1) - 1.0) <= 2 * 65 * EPS).all()
    # the scale is a fixed point: saxs_fit of the reweighted mean returns it
    for t in range(len(thetas)):
        fit = metrics.saxs_fit(out["mean"][t], prof["q"], curve, sigma)
        assert abs(float(fit["scale"]) - o["scale"][t]) <= 1e-9 * o["scale"][t] * 1.01
    # the planted reweighting moved the mean swelling factor up from the uniform ensemble's
    assert float(o["w"][-1] @ swell) > float(swell.mean())
    # fit="none" is reweight on the same arrays, to the bit
    scaled = curve / 2.5
    a = host(metrics.saxs_reweight(prof["I"], prof["q"], scaled, sigma, thetas, fit="none"))
    b = host(metrics.reweight(prof["I"], scaled, sigma, thetas))
    assert same_bits(a, b) and (a["scale"] == 1.0).all() and a["scale_converged"].all()
    # finite = False is w0 = 0
    fin = prof["finite"].clone()
    fin[[4, 40]] = False
    w0 = np.ones(65)
    w0[[4, 40]] = 0.0
    a = host(metrics.saxs_reweight(prof["I"], prof["q"], scaled, sigma, 10.0, finite=fin, fit="none"))
    b = host(metrics.reweight(prof["I"], scaled, sigma, 10.0, w0=dev(w0)))
    assert same_bits(a, b) and (a["w"][:, [4, 40]] == 0).all()


def test_saxs_reweight_restarts_cold_and_reports_a_stalled_solve():
    """Case (257, 64) in another unit (x 0.37), as tests/test_reweight_host.py runs the reference's loop.  theta = 1: the
    scale converges to the reference loop's (both are roots of h within 1e-9 |c|; 1e-6 leaves room for |h'| down to 1e-3).
    theta = 0.1: the reference's inner solves stall there - whatever the device meets, scale_converged is True only with
    status 0 and |h| <= 1e-9 |c|, the weights stay finite and normalised, and the rounds stay within 40."""
    from tests.test_reweight_host import SECANT_FACTOR, _secant
    N, M = 257, 64
    c = rr.case(N, M)
    I = dev(c["Y"] * SECANT_FACTOR)
    o = host(metrics.saxs_reweight(I, c["q"], c["y"], c["sigma"], [1.0, 0.1]))
    ref_c, _h, _rounds, ref_ok, _res = _secant(N, M, 1.0)
    print("saxs_reweight x 0.37: " + "; ".join(
        f"theta {th:g}: scale {o['scale'][t]:.9f} h {o['scale_residual'][t]:.1e} {o['rounds'][t]} rounds {o['n_iter'][t]} steps "
        f"{rr.STATUS[o['status'][t]]} converged {bool(o['scale_converged'][t])}" for t, th in enumerate((1.0, 0.1))) + f"; reference scale at theta 1 {ref_c:.9f}")
    assert ref_ok and o["scale_converged"][0] and o["status"][0] == 0 and abs(o["scale"][0] - ref_c) <= 1e-6 * ref_c
    for t in range(2):
        small = abs(o["scale_residual"][t]) <= 1e-9 * abs(o["scale"][t])
        assert bool(o["scale_converged"][t]) == bool(small and o["status"][t] == 0)
        assert o["rounds"][t] <= 40 and np.isfinite(o["w"][t]).all() and abs(o["w"][t].sum() - 1.0) <= 2 * N * EPS


def test_weighted_mean_adds_in_index_order():
    rng = np.random.Generator(np.random.PCG64(4))
    S = 300
    values = rng.standard_normal((S, 7, 3))
    uniform = np.full(S, 1.0 / S)
    want = np.zeros((7, 3))
    for s in range(S):
        want = want + uniform[s] * values[s]
    got = metrics.weighted_mean(dev(values), dev(uniform)).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (7, 3) and np.array_equal(got, want)
    assert np.abs(got - values.mean(axis=0)).max() <= 4 * S * EPS * np.abs(values).max()
    w = rng.uniform(0, 1, (2, S))
    w[:, [5, 17]] = 0.0
    values[5], values[17, 2, 1] = np.nan, np.inf          # a structure of weight 0 does not reach the average
    want = np.zeros((2, 7, 3))
    for s in range(S):
        if w[0, s] != 0:
            want = want + w[:, s, None, None] * values[s][None]
    got = metrics.weighted_mean(dev(values), dev(w)).cpu().numpy()
    assert got.shape == (2, 7, 3) and np.array_equal(got, want)
    rg = metrics.weighted_mean(dev(values[:, 0, 0].astype(np.float32)), dev(w[1])).cpu().numpy()      # a per-structure scalar, fp32
    assert rg.shape == () and abs(float(rg) - float(want[1, 0, 0])) <= 1e-6 * np.abs(w[1] * values[:, 0, 0])[np.isfinite(values[:, 0, 0])].sum()
    with pytest.raises(ValueError, match="values must be"):
        metrics.weighted_mean(dev(values[:10]), dev(w))


def test_cli_saxs_reweight_end_to_end(tmp_path):
    """--saxs 51 --saxs_data FILE --saxs_reweight 10 1 in a fresh child process: weights [n_theta, S] that sum to 1 per theta,
    the reweighted mean profiles beside them, and the L-curve on stdout."""
    q = np.linspace(0.0, 0.5, 51)
    curve = 3e5 * np.exp(-(q * 14.0) ** 2 / 3.0) + 2e3 / (1.0 + (q * 14.0) ** 2)
    sigma = 0.03 * curve
    path = tmp_path / "curve.dat"
    path.write_text("# q I sigma\n" + "".join(f"{float(a)!r} {float(b)!r} {float(s)!r}\n" for a, b, s in zip(q, curve, sigma)))
    files, stdout = _cli(tmp_path, "--saxs", "51", "--saxs_data", str(path), "--saxs_reweight", "10", "1")
    assert "SAXS reweighting" in stdout and stdout.count("theta 10 ") == 4 and stdout.count("theta 1 ") == 4     # four proteins
    weights = sorted(f for f in files if f.endswith("_saxs_weights.npy"))
    assert len(weights) == 4 and len([f for f in files if f.endswith("_saxs_reweighted.npy")]) == 4
    for f in weights:
        w = np.load(files[f])
        I = np.load(files[f.replace("_saxs_weights.npy", "_saxs.npy")])
        mean = np.load(files[f.replace("_saxs_weights.npy", "_saxs_reweighted.npy")])
        assert w.dtype == np.float64 and w.shape == (2, I.shape[0]) and mean.shape == (2, 51)
        assert (w >= 0).all() and (np.abs(w.sum(axis=1) - 1.0) <= 2 * I.shape[0] * EPS).all()
        assert np.abs(mean - w @ I).max() <= 1e-12 * np.abs(I).max()
