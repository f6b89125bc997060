"""Maximum-entropy (BME) reweighting of an ensemble against experimental data (codlad_reweight_solve,
csrc/reweight_kernels.hip): the weights closest to the prior, in relative entropy, whose averages agree with the data at
the confidence theta - for any per-structure observables (reweight), and for SAXS profiles with the arbitrary scale of the
intensities fitted along (saxs_reweight).  weighted_mean turns the weights into the reweighted average of anything else
that is known per structure.  The Newton iteration runs on the device without a host synchronisation; the scale's fixed
point is a scalar loop here."""
import math

import numpy as np
import torch

from .. import _lib
from . import _inputs

REWEIGHT_STATUS = _lib.REWEIGHT_STATUS
REWEIGHT_MAX_OBS = _lib.SAXS_MAX_Q
SECANT_RTOL, SECANT_MAX_ROUNDS = 1e-9, 40


def _host64(a, what, n=None):
    a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a), dtype=np.float64).reshape(-1)
    if n is not None and a.shape[0] != n:
        raise ValueError(f"{what} must have {n} values, got {a.shape[0]}")
    return a


def _problem_inputs(what, Y, y, sigma, theta, w0, scale, mu0, gtol, max_iter):
    """Checked arguments of codlad_reweight_solve -> (Y, y, sigma, w0 or None, mu0 or None on the device, theta and scale
    float64 numpy [n_problems], whether theta was a list)."""
    _inputs.need_cuda(Y, f"{what}: Y")
    if Y.dim() != 2 or 0 in Y.shape:
        raise ValueError(f"{what}: Y must be a non-empty [N, M] tensor (M observables of N structures), got {tuple(Y.shape)}")
    N, M = Y.shape
    if M > REWEIGHT_MAX_OBS:
        raise ValueError(f"{what}: at most {REWEIGHT_MAX_OBS} observables, got {M}")
    dev = Y.device
    yh, sh = _host64(y, f"{what}: y", M), _host64(sigma, f"{what}: sigma", M)
    if not (np.isfinite(yh).all() and np.isfinite(sh).all() and (sh > 0).all()):
        raise ValueError(f"{what}: y and sigma must be finite and every sigma positive")
    many = not (np.isscalar(theta) or (torch.is_tensor(theta) and theta.dim() == 0) or np.ndim(theta) == 0)
    th = _host64(theta, f"{what}: theta")
    if not th.shape[0] or th.shape[0] > _lib.REWEIGHT_MAX_PROBLEMS or not (np.isfinite(th).all() and (th > 0).all()):
        raise ValueError(f"{what}: theta must be 1 .. {_lib.REWEIGHT_MAX_PROBLEMS} positive finite numbers")
    sc = _host64(scale, f"{what}: scale")
    sc = np.full(th.shape[0], sc[0]) if sc.shape[0] == 1 else sc
    if sc.shape[0] != th.shape[0] or not (np.isfinite(sc).all() and (sc > 0).all()):
        raise ValueError(f"{what}: scale must be one positive finite number, or one per theta")
    if not (isinstance(max_iter, (int, np.integer)) and 1 <= max_iter <= _lib.REWEIGHT_MAX_ITER):
        raise ValueError(f"{what}: max_iter must be an integer in 1 .. {_lib.REWEIGHT_MAX_ITER}")
    if not (math.isfinite(float(gtol)) and float(gtol) > 0):
        raise ValueError(f"{what}: gtol must be a positive finite number")
    Yd = Y.detach().to(torch.float64).contiguous()
    w0d = None
    if w0 is not None:
        w0d = torch.as_tensor(w0).detach().to(device=dev, dtype=torch.float64).reshape(-1).contiguous()
        if w0d.shape[0] != N:
            raise ValueError(f"{what}: w0 must have one weight per structure ({N}), got {w0d.shape[0]}")
    mu0d = None
    if mu0 is not None:
        mu0d = torch.as_tensor(mu0).detach().to(device=dev, dtype=torch.float64)
        mu0d = (mu0d.reshape(1, M).expand(th.shape[0], M) if mu0d.numel() == M else mu0d.reshape(th.shape[0], M)).contiguous()
    up = lambda a: torch.from_numpy(a.copy()).to(dev)                                # noqa: E731
    return Yd, up(yh), up(sh), w0d, mu0d, th, sc, many


def _solve(what, Y, y, sigma, theta, w0, scale, mu0, gtol, max_iter):
    Yd, yd, sd, w0d, mu0d, th, sc, many = _problem_inputs(what, Y, y, sigma, theta, w0, scale, mu0, gtol, max_iter)
    dev = Yd.device
    (N, M), T = Yd.shape, th.shape[0]
    lib = _lib.lib()
    scratch = _inputs.scratch("codlad_reweight_scratch_bytes", N, M, T, dev=dev)
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)     # noqa: E731
    mu, w, mean, scal = f64(T, M), f64(T, N), f64(T, M), f64(T, _lib.REWEIGHT_SCALARS)
    n_iter = torch.empty(T, dtype=torch.int32, device=dev)
    status = torch.empty(T, dtype=torch.int32, device=dev)
    used = torch.empty(N, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    rc = lib.codlad_reweight_solve(p(Yd), p(yd), p(sd), p(w0d), N, M, th.ctypes.data, sc.ctypes.data, T, p(mu0d), float(gtol),
                                   int(max_iter), p(scratch), 8 * scratch.numel(), p(mu), p(w), p(mean), p(scal), p(n_iter), p(status), p(used),
                                   _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_reweight_solve")
    out = dict(mu=mu, w=w, mean=mean, chi2_prior=scal[:, 0], chi2=scal[:, 1], s_rel=scal[:, 2], phi_eff=scal[:, 3], n_iter=n_iter,
               status=status, used=used.to(torch.bool), theta=torch.from_numpy(th.copy()).to(dev), scale=torch.from_numpy(sc.copy()).to(dev))
    return out, many


def reweight(Y, y, sigma, theta, w0=None, scale=1.0, mu0=None, gtol=1e-9, max_iter=50):
    """Reweight N structures so that the averages of their M observables Y [N, M] (device) agree with the experiment y +-
    sigma [M]: for every theta (one number or a list; each an independent problem of the same call) the weights
      w_j = w0_j exp(-mu . z_j) / Z,  z_jk = (scale * Y_jk - y_k) / sigma_k
    at the unique minimiser mu of Gamma(mu) = log sum_j w0_j exp(-mu . z_j) + (theta / 2) |mu|^2, by the damped Newton
    iteration include/codlad_hip.h states.  A large theta keeps the prior, a small one trusts the data.  w0 [N]: prior
    weights >= 0 (default uniform; normalised here).  A structure with w0 = 0, a w0 that is not finite, or a NaN / infinity
    in its row of Y is excluded: weight exactly 0, used False.  scale: one number or one per theta.  mu0 [M] or
    [n_theta, M]: a warm start.  -> dict of device tensors with a leading theta axis (also for a single theta):
      mu [T, M], w [T, N], mean [T, M] (= w @ Y)        float64
      chi2_prior, chi2 [T]     sum(((scale * <Y> - y) / sigma)^2) / (M - 1) under w0 and under w (0 for M = 1)
      s_rel, phi_eff [T]       sum w log(w / w0) and exp(-s_rel), the effective share of the ensemble that is kept
      n_iter, status int32 [T] the Newton steps taken; REWEIGHT_STATUS[status]: 0 converged (|g|_inf <= gtol * gscale), 1
                               max_iter reached, 2 no step of the ladder lowers Gamma, 3 the Hessian is not positive
                               definite in float64, 4 no usable structure (then everything else is NaN)
      used bool [N], theta, scale [T]
    No host synchronisation; the bits repeat from call to call and a theta's results do not depend on the others.
    ValueError for a y or sigma that is not finite, a sigma <= 0, a theta / scale / gtol that is not a positive finite
    number, more than REWEIGHT_MAX_OBS observables."""
    return _solve("reweight", Y, y, sigma, theta, w0, scale, mu0, gtol, max_iter)[0]


def _fit_scale(mean, y, wk):
    """saxs_fit's closed form for every row of mean [T, M] -> [T] (device float64)."""
    return (y * mean * wk).sum(dim=1) / (mean * mean * wk).sum(dim=1)


def saxs_reweight(I, q, I_exp, sigma, theta, w0=None, finite=None, fit="scale"):
    """reweight for SAXS profiles: I [S, Q] (device; saxs_profile's or saxs_combine's, on the experiment's q grid - q is
    only checked for its length), I_exp and sigma [Q], theta as for reweight.  finite bool [S] (saxs_profile's): a False row
    gets w0 = 0.  fit="none": the intensities are compared as they are (scale 1) - reweight(I, I_exp, sigma, theta, w0) to
    the bit.  fit="scale": per theta the scale c of the calculated intensities is a fixed point of c = fit(w(c)), fit being
    saxs_fit's closed form on the reweighted mean: h(c) = fit(w(c)) - c = 0 by the secant method, warm-starting mu from
    round to round, with the plain update c <- fit(w) when the secant step is not finite or leaves (c / 2, 2 c); it ends at
    |h| <= 1e-9 |c| or after 40 rounds, reading two numbers per theta and round (h and the status: a theta whose
    warm-started solve did not converge is solved once more from mu = 0 at the same c).  -> reweight's dict (scale = the c of the
    last solve) and scale_residual [T] (h there), rounds int [T], scale_converged bool [T] (|h| <= 1e-9 |c| AND the last
    solve's status is 0: a scale read off a solve that stalled is not a fixed point of anything), n_iter the Newton steps of
    all rounds."""
    _inputs.need_cuda(I, "saxs_reweight: I")
    if fit not in ("none", "scale"):
        raise ValueError(f"saxs_reweight: fit must be 'none' or 'scale', got {fit!r}")
    if I.dim() != 2 or _host64(q, "saxs_reweight: q").shape[0] != I.shape[1]:
        raise ValueError("saxs_reweight: I must be [S, Q] on the Q values of q")
    dev = I.device
    if finite is not None:
        fin = torch.as_tensor(finite).to(device=dev).reshape(-1).to(torch.bool)
        if fin.shape[0] != I.shape[0]:
            raise ValueError(f"saxs_reweight: finite must have one entry per structure ({I.shape[0]})")
        prior = torch.ones(I.shape[0], dtype=torch.float64, device=dev) if w0 is None else \
            torch.as_tensor(w0).detach().to(device=dev, dtype=torch.float64).reshape(-1)
        w0 = torch.where(fin, prior, torch.zeros_like(prior))
    if fit == "none":
        out, _many = _solve("saxs_reweight", I, I_exp, sigma, theta, w0, 1.0, None, 1e-9, 50)
        T = out["theta"].shape[0]
        out.update(scale_residual=torch.zeros(T, dtype=torch.float64, device=dev), rounds=torch.ones(T, dtype=torch.int32, device=dev),
                   scale_converged=torch.ones(T, dtype=torch.bool, device=dev))
        return out
    if I.shape[1] < 2:
        raise ValueError("saxs_reweight: fitting the scale needs two q values or more")
    Yd, yd, sd, w0d, _mu0, th, _sc, _many = _problem_inputs("saxs_reweight", I, I_exp, sigma, theta, w0, 1.0, None, 1e-9, 50)
    T = th.shape[0]
    wk = 1.0 / (sd * sd)
    # the start: the fit of the prior mean over the usable rows
    prior = w0d if w0d is not None else torch.ones(Yd.shape[0], dtype=torch.float64, device=dev)
    ok = torch.isfinite(Yd).all(dim=1) & torch.isfinite(prior) & (prior > 0)
    pw = torch.where(ok, prior, torch.zeros_like(prior))
    prior_mean = (torch.where(ok[:, None], Yd, torch.zeros_like(Yd)) * pw[:, None]).sum(dim=0) / pw.sum()
    c0 = float(_fit_scale(prior_mean[None], yd, wk)[0])
    if not (math.isfinite(c0) and c0 > 0):
        c0 = 1.0                                              # no usable row (status 4 below), or a curve that fits no positive scale
    c = np.full(T, c0)
    c_prev, h_prev = np.full(T, np.nan), np.full(T, np.nan)
    done = np.zeros(T, dtype=bool)
    rounds, total_iter = np.zeros(T, dtype=np.int64), None
    mu, out = None, None
    h_at, c_at = np.full(T, np.nan), c.copy()
    for _round in range(SECANT_MAX_ROUNDS):
        res = _solve("saxs_reweight", Yd, yd, sd, th, w0d, c, mu, 1e-9, 50)[0]
        live = torch.from_numpy(~done).to(dev)
        n_it = res["n_iter"]
        look = lambda r: torch.stack([_fit_scale(r["mean"], yd, wk) - r["scale"], r["status"].to(torch.float64)]).cpu().numpy()   # noqa: E731
        h, st = look(res)                                     # the one transfer of the round
        if mu is not None and (st[~done] != 0).any():
            # a warm start from the last scale's mu can lie where no step of the ladder lowers Gamma: those thetas start cold
            cold = torch.from_numpy((st != 0) & ~done).to(dev)
            again = _solve("saxs_reweight", Yd, yd, sd, th, w0d, c, torch.where(cold[:, None], torch.zeros_like(mu), mu), 1e-9, 50)[0]
            for k, v in again.items():
                if k != "used":
                    res[k] = torch.where(cold.reshape(-1, *[1] * (v.dim() - 1)), v, res[k])
            n_it = n_it + torch.where(cold, again["n_iter"], torch.zeros_like(n_it))
            h, st = look(res)
        if out is None:
            out, total_iter = res, n_it.clone()
        else:                                                 # a finished theta keeps the solve it finished with
            for k, v in res.items():
                if k != "used":
                    out[k] = torch.where(live.reshape(-1, *[1] * (v.dim() - 1)), v, out[k])
            total_iter = total_iter + torch.where(live, n_it, torch.zeros_like(n_it))
        mu = torch.nan_to_num(out["mu"], nan=0.0)
        for k in np.nonzero(~done)[0]:
            rounds[k] += 1
            h_at[k], c_at[k] = h[k], c[k]
            if not np.isfinite(h[k]) or abs(h[k]) <= SECANT_RTOL * abs(c[k]):
                done[k] = True
                continue
            nxt = c[k] + h[k]
            if np.isfinite(h_prev[k]) and h[k] != h_prev[k]:
                sec = c[k] - h[k] * (c[k] - c_prev[k]) / (h[k] - h_prev[k])
                if np.isfinite(sec) and c[k] / 2 < sec < 2 * c[k]:
                    nxt = sec
            if not (np.isfinite(nxt) and nxt > 0):
                done[k] = True
                continue
            c_prev[k], h_prev[k], c[k] = c[k], h[k], nxt
        if done.all():
            break
    out["n_iter"] = total_iter
    out["scale_residual"] = torch.from_numpy(h_at).to(dev)
    out["rounds"] = torch.from_numpy(rounds.astype(np.int32)).to(dev)
    out["scale_converged"] = torch.from_numpy(np.isfinite(h_at) & (np.abs(h_at) <= SECANT_RTOL * np.abs(c_at))).to(dev) & (out["status"] == 0)
    return out


def weighted_mean(values, w):
    """The reweighted average of a per-structure quantity: values [S, ...] (any dtype; the leading axis is the structure)
    and w [S] or [T, S] (reweight's w) -> float64 [...] or [T, ...] on the device of w: sum_s w_s values_s added to 0 in
    index order (codlad_weighted_mean).  A structure of weight 0 is left out, whatever its values hold (a NaN row of an excluded structure does not
    reach the average)."""
    _inputs.need_cuda(w, "weighted_mean: w")
    wd = w.detach().to(torch.float64)
    lead = wd.dim() == 2
    wd = wd.reshape(-1, wd.shape[-1])
    v = torch.as_tensor(values).detach().to(device=wd.device, dtype=torch.float64)
    if v.dim() < 1 or v.shape[0] != wd.shape[1] or w.dim() not in (1, 2):
        raise ValueError(f"weighted_mean: values must be [S, ...] and w [S] or [T, S], got {tuple(v.shape)} and {tuple(w.shape)}")
    flat = v.reshape(v.shape[0], -1).contiguous()
    if 0 in flat.shape:
        raise ValueError("weighted_mean: values holds no element")
    wd = wd.contiguous()
    out = torch.empty(wd.shape[0], flat.shape[1], dtype=torch.float64, device=wd.device)
    p = _lib.ptr
    rc = _lib.lib().codlad_weighted_mean(p(flat), p(wd), flat.shape[0], flat.shape[1], wd.shape[0], p(out), _lib.stream_ptr(wd.device))
    _lib.check(rc, "codlad_weighted_mean")
    out = out.reshape(wd.shape[0], *v.shape[1:])
    return out if lead else out[0]
