"""References of the reweighting feature (codlad_amd.metrics.reweight): the float64 numpy restatement of the damped Newton
solver that include/codlad_hip.h states, an np.longdouble evaluation of the gradient, the stop rule's scale, the weights and
chi^2 at a given mu, the secant loop of the fitted scale, and the seeded cases.  Nothing here reads a device result."""
import functools

import numpy as np

EPS = 2.0 ** -52
LADDER = 16
SHAPES = ((2, 1), (3, 2), (65, 3), (257, 64), (300, 51), (100, 200), (1000, 129), (2048, 512))
THETAS = (1000.0, 10.0, 1.0, 0.1)
STATUS = ("converged", "cap", "stalled", "failed", "none")


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(N, M):
    """Guinier-like curves 1e4 exp(-(q Rg)^2 / 3) + 30 / (1 + (q Rg)^2) of N structures, Rg uniform in 15 .. 45 A, on M
    points of (0, 0.3] 1/A; the experiment is the mean under a Gaussian reweighting in Rg plus 3 % noise (y lies inside the
    hull of the rows), sigma 3 % of the noiseless mean."""
    rng = np.random.Generator(np.random.PCG64(1000 * N + M))
    q = np.linspace(0.3 / M, 0.3, M)
    rg = rng.uniform(15.0, 45.0, N)
    Y = 1e4 * np.exp(-np.outer(rg, q) ** 2 / 3.0) + 30.0 / (1.0 + np.outer(rg, q) ** 2)
    wt = np.exp(-0.5 * ((rg - 24.0) / 4.0) ** 2) + 1e-3
    wt /= wt.sum()
    clean = wt @ Y
    sigma = 0.03 * clean
    y = clean + sigma * rng.standard_normal(M)
    return _freeze(dict(q=q, rg=rg, Y=Y, y=y, sigma=sigma, w_true=wt))


def case_keys():
    return [(N, M, th) for N, M in SHAPES for th in THETAS]


def usable(Y, w0):
    return np.isfinite(Y).all(axis=1) & np.isfinite(w0) & (w0 > 0)


def evaluate(Y, y, sigma, theta, mu, w0=None, scale=1.0, dtype=np.longdouble):
    """At a given mu, in `dtype`: dict(g, gscale, w, mean, chi2, chi2_prior, s_rel, phi_eff, gamma, absw) - absw =
    sum_j w_j |log(w_j / w0_j)|, the magnitude s_rel's rounding is measured against."""
    f = dtype
    Y = np.asarray(Y, dtype=np.float64)
    N, M = Y.shape
    w0 = np.ones(N) if w0 is None else np.asarray(w0, dtype=np.float64)
    use = usable(Y, w0)
    sig = np.asarray(sigma, dtype=np.float64).astype(f)
    U = np.where(use[:, None], Y, 0.0).astype(f) / sig
    v = np.asarray(y, dtype=np.float64).astype(f) / sig
    p0 = np.where(use, w0, 0.0).astype(f)
    p0 = p0 / p0.sum()
    mu = np.asarray(mu, dtype=np.float64).astype(f)
    c, th = f(scale), f(theta)
    z = c * U - v
    with np.errstate(divide="ignore"):
        logp0 = np.where(use, np.log(np.where(use, p0, 1)), -np.inf).astype(f)
    a = logp0 - z @ mu
    m = a[use].max()
    e = np.where(use, np.exp(np.where(use, a - m, 0)), 0).astype(f)
    Z = e.sum()
    w = e / Z
    ubar = w @ U
    g = th * mu - (c * ubar - v)
    gscale = (w @ np.abs(z)).max() + th * np.abs(mu).max()
    pos = w > 0
    logs = np.log(w[pos]) - logp0[pos]
    s_rel = (w[pos] * logs).sum()
    den = f(max(M - 1, 1))
    chi2 = ((c * ubar - v) ** 2).sum() / den if M > 1 else f(0)
    chi2_prior = ((c * (p0 @ U) - v) ** 2).sum() / den if M > 1 else f(0)
    return dict(g=g, gscale=gscale, w=w, mean=ubar * sig, chi2=chi2, chi2_prior=chi2_prior, s_rel=s_rel, phi_eff=np.exp(-s_rel),
                gamma=(m + np.log(Z)) + th / 2 * (mu @ mu), absw=(w[pos] * np.abs(logs)).sum(), p0=p0, use=use)


def residual(Y, y, sigma, theta, mu, w0=None, scale=1.0, dtype=np.longdouble):
    """(|g|_inf / gscale, |g|_2) at mu, in `dtype`."""
    ev = evaluate(Y, y, sigma, theta, mu, w0, scale, dtype)
    return float(np.abs(ev["g"]).max() / ev["gscale"]), float(np.sqrt((ev["g"] ** 2).sum()))


def solve(Y, y, sigma, theta, w0=None, scale=1.0, mu0=None, gtol=1e-9, max_iter=50):
    """The solver of include/codlad_hip.h in numpy float64 -> dict(mu, w, mean, chi2, chi2_prior, s_rel, phi_eff, n_iter,
    status, used)."""
    Y = np.asarray(Y, dtype=np.float64)
    N, M = Y.shape
    w0 = np.ones(N) if w0 is None else np.asarray(w0, dtype=np.float64)
    use = usable(Y, w0)
    if not use.any():
        nan = np.full(M, np.nan)
        return dict(mu=nan, w=np.full(N, np.nan), mean=nan.copy(), chi2=np.nan, chi2_prior=np.nan, s_rel=np.nan, phi_eff=np.nan,
                    n_iter=0, status=4, used=use)
    sig = np.asarray(sigma, dtype=np.float64)
    U = np.where(use[:, None], Y, 0.0) / sig
    v = np.asarray(y, dtype=np.float64) / sig
    p0 = np.where(use, w0, 0.0)
    p0 = p0 / p0.sum()
    with np.errstate(divide="ignore"):
        logp0 = np.where(use, np.log(np.where(use, p0, 1.0)), -np.inf)
    c = float(scale)
    z = c * U - v
    mu = np.zeros(M) if mu0 is None else np.array(mu0, dtype=np.float64)
    n_iter, status = 0, None
    ladder = 0.5 ** np.arange(LADDER)

    def lse(a):
        m = a[use].max()
        return m, np.where(use, np.exp(np.where(use, a - m, 0.0)), 0.0)

    while True:
        a = logp0 - z @ mu
        m, e = lse(a)
        Z = e.sum()
        w = e / Z
        ubar = w @ U
        g = theta * mu - (c * ubar - v)
        gscale = (w @ np.abs(z)).max() + theta * np.abs(mu).max()
        gamma = (m + np.log(Z)) + 0.5 * theta * (mu @ mu)
        if np.abs(g).max() <= gtol * gscale:
            status = 0
            break
        if n_iter >= max_iter:
            status = 1
            break
        d = U - ubar
        H = c * c * ((d * w[:, None]).T @ d) + theta * np.eye(M)
        try:
            L = np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            status = 3
            break
        if not np.isfinite(L).all():
            status = 3
            break
        p = -np.linalg.solve(L.T, np.linalg.solve(L, g))
        s = z @ p
        gp = g @ p
        step = None
        for t in ladder:
            mt, et = lse(a - t * s)
            x = mu + t * p
            trial = (mt + np.log(et.sum())) + 0.5 * theta * (x @ x)
            if trial <= gamma + 1e-4 * t * gp + 8 * EPS * (1 + abs(gamma)):
                step = t
                break
        if step is None:
            status = 2
            break
        mu = mu + step * p
        n_iter += 1
    pos = w > 0
    s_rel = float((w[pos] * (np.log(w[pos]) - logp0[pos])).sum())
    den = max(M - 1, 1)
    return dict(mu=mu, w=w, mean=ubar * sig, chi2=float(((c * ubar - v) ** 2).sum() / den) if M > 1 else 0.0,
                chi2_prior=float(((c * (p0 @ U) - v) ** 2).sum() / den) if M > 1 else 0.0, s_rel=s_rel,
                phi_eff=float(np.exp(-s_rel)), n_iter=n_iter, status=status, used=use)


def fit_scale(mean, y, sigma):
    """saxs_fit's closed form: c = sum(y m / sigma^2) / sum(m^2 / sigma^2)."""
    wk = 1.0 / (np.asarray(sigma) ** 2)
    return float((y * mean * wk).sum() / (mean * mean * wk).sum())


def secant(solve_at, fit, c0, rtol=1e-9, max_rounds=40):
    """The fixed point c = fit(w(c)) by the secant method on h(c) = fit(w(c)) - c with the plain update as the fall-back (and a cold
    restart of a warm-started solve that did not converge):
    solve_at(c, mu_warm) -> (result, mu), fit(result) -> float.  -> (c, h, rounds, converged, result).  The loop that
    codlad_amd.metrics.reweight.saxs_reweight runs per theta, stated once more."""
    c, mu = float(c0), None
    c_prev = h_prev = None
    for rounds in range(1, max_rounds + 1):
        res, mu_new = solve_at(c, mu)
        if mu is not None and res["status"] != 0:          # a warm start that did not converge: once more from mu = 0
            res, mu_new = solve_at(c, None)
        mu = mu_new
        h = fit(res) - c
        if not np.isfinite(h) or abs(h) <= rtol * abs(c):
            return c, h, rounds, bool(np.isfinite(h)) and res["status"] == 0, res
        nxt = c + h                                        # the plain update c <- fit(w)
        if h_prev is not None and h != h_prev:
            sec = c - h * (c - c_prev) / (h - h_prev)
            if np.isfinite(sec) and c / 2 < sec < 2 * c:
                nxt = sec
        c_prev, h_prev, c = c, h, nxt
    return c_prev, h_prev, max_rounds, False, res


@functools.lru_cache(maxsize=None)
def reference(N, M, theta):
    """The float64 solve of case (N, M) at theta, with its own longdouble and float64 residuals."""
    c = case(N, M)
    out = solve(c["Y"], c["y"], c["sigma"], theta)
    rel_ld, g2_ld = residual(c["Y"], c["y"], c["sigma"], theta, out["mu"])
    rel_64, _g2 = residual(c["Y"], c["y"], c["sigma"], theta, out["mu"], dtype=np.float64)
    out.update(rel_ld=rel_ld, g2_ld=g2_ld, rel_64=rel_64)
    return _freeze(out)
