"""Essential dynamics of an ensemble (csrc/pca_kernels.hip; the arithmetic is stated in include/codlad_hip.h): the mean
structure of a pool of up to 65 536 structures after mutual superposition (mean_structure, generalised Procrustes), the
per-atom fluctuation about it (rmsf), the covariance of the aligned coordinates as one float64 matrix product on the MFMA
units (covariance), its largest eigenpairs with the projections of the pool (pca), and the projections of another pool on a
model (pca_project).  The host enqueues the iterations of the fit and of the eigen-solve in batches and reads one word per
batch.  weights [N] (>= 0, finite; for instance reweight's w) make every average the weighted one; uniform weights that
are 1 or another power of two return the bits of weights=None (a weight enters every sum as one exact factor)."""
import torch

from .. import _lib
from . import _inputs
from .ensemble import _moments

PCA_MAX_N, PCA_MAX_DIM, PCA_MAX_COMPONENTS = _lib.PCA_MAX_N, _lib.PCA_MAX_DIM, _lib.PCA_MAX_COMPONENTS
PCA_FIT_BATCH = 8             # iterations of the fit enqueued between two looks at its state
PCA_EIG_BATCH = 16            # iterations of the eigen-solve enqueued between two looks


def _fit_args(N, weights, start, tol, max_iter, what):
    tol = _inputs.positive(tol, "tol", what)
    max_iter = _inputs.count(max_iter, "max_iter", _lib.PCA_MAX_ITER, what)
    if start is not None:
        if isinstance(start, bool) or not isinstance(start, int) or not 0 <= start < N:
            raise ValueError(f"{what}: start must be the index of a structure (0 .. {N - 1}), got {start!r}")
        if weights is not None and not float(weights[start]) > 0:
            raise ValueError(f"{what}: the start structure {start} has weight 0")
    return tol, max_iter, -1 if start is None else start


def _dim(n_sel, n_atoms, what):
    m = n_sel or n_atoms
    if 3 * m > PCA_MAX_DIM:
        raise ValueError(f"{what}: 3 x {m} selected atoms = {3 * m} coordinates, at most {PCA_MAX_DIM} (select fewer atoms)")
    return m


def _fit(x, sel, n_sel, w, start, tol, max_iter):
    """-> the internal record of a fit: every device buffer the later stages read."""
    N, n = x.shape[:2]
    m = n_sel or n
    dev = x.device
    lib = _lib.lib()
    p = _lib.ptr
    mom = _moments(x, N, n, sel, n_sel)
    scratch = _inputs.scratch("codlad_pca_fit_scratch_bytes", N, m, dev=dev)
    state = torch.zeros(_lib.PCA_STATE_WORDS, dtype=torch.int32, device=dev)          # phase 0: new
    scal = torch.empty(_lib.PCA_SCALARS, dtype=torch.float64, device=dev)
    target, mean = torch.empty(2, m, 3, dtype=torch.float64, device=dev).unbind(0)
    Rt = torch.empty(N, 12, dtype=torch.float64, device=dev)
    finite = _inputs.flags(N, dev)
    for _batch in range(max_iter // PCA_FIT_BATCH + 2):
        rc = lib.codlad_pca_fit(p(x), p(mom), N, n, p(sel), n_sel, p(w), start, tol, max_iter, PCA_FIT_BATCH, p(state), p(scal),
                                p(target), p(mean), p(Rt), p(finite), p(scratch), _lib.stream_ptr(dev))
        _lib.check(rc, "codlad_pca_fit")
        if int(state[_lib.PCA_ST_PHASE]) == 2:                # the one transfer of the batch
            break
    else:
        raise RuntimeError("mean_structure: the fit did not finish")
    st = state.tolist()
    sc = scal.tolist()
    return dict(x=x, sel=sel, n_sel=n_sel, m=m, w=w, mom=mom, mean=mean, target=target, Rt=Rt, finite=finite, scal=scal,
                n_iter=st[_lib.PCA_ST_ITER], status=_lib.PCA_STATUS[st[_lib.PCA_ST_STATUS]], start=st[_lib.PCA_ST_START],
                step=sc[_lib.PCA_SC_STEP], total_weight=sc[_lib.PCA_SC_W])


def _public_fit(f):
    return dict(mean=f["mean"], target=f["target"], R=f["Rt"][:, :9].reshape(-1, 3, 3), t=f["Rt"][:, 9:], n_iter=f["n_iter"],
                step=f["step"], status=f["status"], finite=f["finite"].to(torch.bool), start=f["start"],
                total_weight=f["total_weight"])


def _deviations(f, want_D, want_rmsf):
    x = f["x"]
    N, n = x.shape[:2]
    dev = x.device
    D = torch.empty(N, 3 * f["m"], dtype=torch.float64, device=dev) if want_D else None
    r = torch.empty(f["m"], dtype=torch.float64, device=dev) if want_rmsf else None
    p = _lib.ptr
    rc = _lib.lib().codlad_pca_deviations(p(x), p(f["Rt"]), p(f["finite"]), p(f["w"]), N, n, p(f["sel"]), f["n_sel"], p(f["mean"]),
                                          p(f["scal"]), p(D), p(r), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_pca_deviations")
    return D, r


def _covariance(f, D):
    N, d = D.shape
    dev = D.device
    lib = _lib.lib()
    scratch = _inputs.scratch("codlad_pca_covariance_scratch_bytes", N, d, dev=dev)
    cov = torch.empty(d, d, dtype=torch.float64, device=dev)
    corr = torch.empty(d // 3, d // 3, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    p = _lib.ptr
    rc = lib.codlad_pca_covariance(p(D), p(f["w"]), p(f["finite"]), N, d, p(f["scal"]), p(cov), p(corr), p(total), p(scratch),
                                   _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_pca_covariance")
    return cov, corr, total


def _eigen(cov, k, rtol, max_iter):
    d = cov.shape[0]
    dev = cov.device
    lib = _lib.lib()
    scratch = _inputs.scratch("codlad_pca_eigen_scratch_bytes", d, k, dev=dev)
    state = torch.zeros(_lib.PCA_STATE_WORDS, dtype=torch.int32, device=dev)
    evals, resid = torch.empty(2, k, dtype=torch.float64, device=dev).unbind(0)
    comps = torch.empty(k, d, dtype=torch.float64, device=dev)
    p = _lib.ptr
    for _batch in range(max_iter // PCA_EIG_BATCH + 2):
        rc = lib.codlad_pca_eigen(p(cov), d, k, rtol, max_iter, PCA_EIG_BATCH, p(state), p(evals), p(comps), p(resid), p(scratch),
                                  _lib.stream_ptr(dev))
        _lib.check(rc, "codlad_pca_eigen")
        if int(state[_lib.PCA_ST_PHASE]) == 2:
            break
    else:
        raise RuntimeError("pca: the eigen-solve did not finish")
    st = state.tolist()
    return evals, comps, resid, st[_lib.PCA_ST_ITER], _lib.PCA_STATUS[st[_lib.PCA_ST_STATUS]]


def _project(D, comps):
    N, d = D.shape
    k = comps.shape[0]
    P = torch.empty(N, k, dtype=torch.float64, device=D.device)
    rc = _lib.lib().codlad_pca_project(_lib.ptr(D), _lib.ptr(comps), N, d, k, _lib.ptr(P), _lib.stream_ptr(D.device))
    _lib.check(rc, "codlad_pca_project")
    return P


def _checked_fit(x, sel, weights, start, tol, max_iter, what, need_dim=False):
    x, sel, n_sel = _inputs.pool(x, sel, what, PCA_MAX_N)
    if need_dim:
        _dim(n_sel, x.shape[1], what)
    w = _inputs.weights(weights, x.shape[0], x.device, what, True)
    tol, max_iter, start = _fit_args(x.shape[0], w, start, tol, max_iter, what)
    return _fit(x, sel, n_sel, w, start, tol, max_iter)


def mean_structure(x, sel=None, weights=None, start=None, tol=1e-6, max_iter=100):
    """The mean structure of the pool x [N, n, 3] (N <= 65 536) over the atoms sel (default: all) by generalised Procrustes:
    from the centred structure `start` (default: the first finite structure of positive weight) every structure is superposed
    on the current mean (proper rotation plus translation), the weighted average of the superposed structures is the next
    mean, until it moves by no more than `tol` (RMS over the atoms, in the units of x; 1e-6 A is below the spacing of fp32
    coordinates at protein scale) or `max_iter` iterations are done.  -> dict: mean float64 [m, 3]; target [m, 3], the mean
    of the iteration before, which the returned transforms superpose on; R [N, 3, 3] and t [N, 3] float64 with x[s] @ R[s].T +
    t[s] the superposed structure, so that mean is the weighted average of exactly these; n_iter; step (the last move);
    status "converged", "limit" or "no_weight" (no finite structure of positive weight: everything NaN); finite bool [N] (a
    structure with a NaN or an infinity among its selected atoms takes no part and has NaN transforms); start;
    total_weight."""
    return _public_fit(_checked_fit(x, sel, weights, start, tol, max_iter, "mean_structure"))


def rmsf(x, sel=None, weights=None, start=None, tol=1e-6, max_iter=100):
    """-> float64 [m]: the root of the weighted mean squared deviation of every selected atom from the mean structure after
    the fit of mean_structure (same arguments), from its own sum; any number of atoms."""
    f = _checked_fit(x, sel, weights, start, tol, max_iter, "rmsf")
    return _deviations(f, False, True)[1]


def covariance(x, sel=None, weights=None, start=None, tol=1e-6, max_iter=100):
    """The covariance of the coordinates after the fit of mean_structure (same arguments; 3 m <= 4 096): cov float64 [3 m, 3 m] =
    sum_s w_s D_s D_s^T / W with D_s the deviation of structure s from the mean - the population covariance, divisor W, as
    GROMACS covar has it - symmetric to the bit; cross_correlation [m, m], the trace of each 3 x 3 block over the root of the
    two diagonal traces (diagonal 1; NaN for an atom that does not move); total_variance = trace(cov), a 0-dim tensor;
    deviations [N, 3 m] (NaN rows for structures that are not finite); plus mean_structure's dict."""
    f = _checked_fit(x, sel, weights, start, tol, max_iter, "covariance", need_dim=True)
    D, _ = _deviations(f, True, False)
    cov, corr, total = _covariance(f, D)
    return dict(_public_fit(f), cov=cov, cross_correlation=corr, total_variance=total[0], deviations=D)


def pca(x, n_components=10, sel=None, weights=None, rtol=1e-10, max_iter=1000, return_covariance=False, return_deviations=False,
        start=None, tol=1e-6, fit_max_iter=100):
    """Principal components of the pool x [N, n, 3] over the atoms sel (3 m <= 4 096): the fit of mean_structure (start, tol,
    fit_max_iter), the covariance, and its n_components <= min(64, 3 m) largest eigenpairs by blocked subspace iteration,
    stopped when every wanted pair has |C v - theta v| <= rtol * theta_1 or after max_iter iterations.  -> mean_structure's
    dict plus eigenvalues float64 [k] (descending), components [k, m, 3] (orthonormal; the entry of largest magnitude of
    each is positive), explained = eigenvalues / total_variance, total_variance, projections [N, k] of the deviations on the
    components (NaN rows for structures that are not finite), rmsf [m], residuals [k], eig_iter, eig_status ("converged" or
    "limit"); with return_covariance cov and cross_correlation, with return_deviations deviations [N, 3 m].  A covariance of
    rank below k gives eigenvalues that are zero within rounding and still orthonormal components."""
    what = "pca"
    x, sel, n_sel = _inputs.pool(x, sel, what, PCA_MAX_N)
    m = _dim(n_sel, x.shape[1], what)
    k = _inputs.count(n_components, "n_components", min(PCA_MAX_COMPONENTS, 3 * m), what)
    rtol = _inputs.positive(rtol, "rtol", what)
    max_iter = _inputs.count(max_iter, "max_iter", _lib.PCA_MAX_ITER, what)
    w = _inputs.weights(weights, x.shape[0], x.device, what, True)
    tol, fit_max_iter, start = _fit_args(x.shape[0], w, start, tol, fit_max_iter, what)
    f = _fit(x, sel, n_sel, w, start, tol, fit_max_iter)
    D, fluct = _deviations(f, True, True)
    cov, corr, total = _covariance(f, D)
    evals, comps, resid, eig_iter, eig_status = _eigen(cov, k, rtol, max_iter)
    out = dict(_public_fit(f), eigenvalues=evals, components=comps.view(k, m, 3), explained=evals / total[0], total_variance=total[0],
               projections=_project(D, comps), rmsf=fluct, residuals=resid, eig_iter=eig_iter, eig_status=eig_status,
               sel=None if sel is None else sel.to(torch.int64))
    if return_covariance:
        out["cov"], out["cross_correlation"] = cov, corr
    if return_deviations:
        out["deviations"] = D
    return out


def pca_project(y, model):
    """The pool y [Ny, n, 3] on a model (pca's dict): every structure superposed on model["mean"] over the model's atoms, its
    deviation from the mean projected on model["components"] -> float64 [Ny, k]; NaN rows for structures that are not
    finite."""
    what = "pca_project"
    if not isinstance(model, dict) or "mean" not in model or "components" not in model:
        raise ValueError(f"{what}: model must be the dict pca returns (mean, components)")
    y, sel, n_sel = _inputs.pool(y, model.get("sel"), what, PCA_MAX_N)
    N, n = y.shape[:2]
    mean, comps = model["mean"], model["components"]
    m = _dim(n_sel, n, what)
    if tuple(mean.shape) != (m, 3) or comps.dim() != 3 or tuple(comps.shape[1:]) != (m, 3) or mean.device != y.device:
        raise ValueError(f"{what}: the model's mean {tuple(mean.shape)} and components {tuple(comps.shape)} do not match the "
                         f"{m} selected atoms of y (same device)")
    dev = y.device
    mean = mean.to(torch.float64).contiguous()
    comps = comps.to(torch.float64).contiguous().view(comps.shape[0], 3 * m)
    mom = _moments(y, N, n, sel, n_sel)
    tmom = torch.empty(4, dtype=torch.float64, device=dev)
    Rt = torch.empty(N, 12, dtype=torch.float64, device=dev)
    finite = _inputs.flags(N, dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_pca_align(p(y), p(mom), N, n, p(sel), n_sel, p(mean), p(tmom), p(Rt), p(finite), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_pca_align")
    D, _ = _deviations(dict(x=y, Rt=Rt, finite=finite, w=None, sel=sel, n_sel=n_sel, m=m, mean=mean, scal=None), True, False)
    return _project(D, comps)


__all__ = ["PCA_MAX_N", "PCA_MAX_DIM", "PCA_MAX_COMPONENTS", "PCA_FIT_BATCH", "PCA_EIG_BATCH", "mean_structure", "rmsf",
           "covariance", "pca", "pca_project"]
