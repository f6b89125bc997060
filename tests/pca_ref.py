"""Host reference and inputs of the essential-dynamics tests (tests/test_pca.py, tests/test_pca_host.py).

The reference is float64 numpy: the Procrustes rule of include/codlad_hip.h on ensemble_ref.kabsch, the covariance by plain
numpy (np.longdouble where a bound is held), np.linalg.eigh.  Every layer of the device is compared with the reference AT THE
DEVICE'S OWN INPUT to that layer (the alignment at the device's target, the covariance at the device's deviations, the
eigenpairs at the device's covariance), so that a bound comes from rounding and not from where an iteration stopped.
Inputs are built on the CPU in fp32 from fixed seeds, once per session, read-only."""
import functools

import numpy as np

from tests import ensemble_ref as er

EPS = 2.0 ** -52
LD = np.longdouble

# (N, m, kind): every N of 1, 2, 3, 15, 16, 17, 65, 130, 1030 and every m of 1, 2, 21, 22, 43, 65 (d = 3, 6, 63, 66, 129, 195:
# below, at and across one, two and three 64-wide tiles)
SHAPES = ((1, 21, "compact"), (2, 1, "compact"), (3, 2, "compact"), (15, 22, "compact"), (16, 43, "compact"),
          (17, 65, "compact"), (65, 21, "far"), (65, 65, "compact"), (130, 65, "walk"), (130, 1, "far"), (1030, 43, "walk"),
          (1030, 2, "compact"), (130, 22, "far"))
LARGE_DIM = (20, 1365, "compact")           # d = 4 095
MANY = (16400, 2, "compact")                # 32 chunks of 528 structures, the last one of 32; 17 blocks of 1 024
PLANTED = {"plain": (130, 43, (0.9, 0.6, 0.4, 0.25)), "three tiles": (65, 65, (1.0, 0.5, 0.3)),
           "equal pair": (130, 22, (0.8, 0.5, 0.5, 0.2)), "rank deficient": (3, 21, (0.7, 0.4))}
# how closely the reference (Procrustes, covariance, eigh, all float64) recovers a planted eigenvalue sigma_i^2 from the
# fp32 pool, relative to sigma_1^2: twice the largest value test_pca_host.py measures over PLANTED (4.3e-7, "rank
# deficient": the fp32 rounding of the coordinates, 2^-24 of 10 A against amplitudes below 1 A).  Eigenvalues only: the
# recovered vectors live in the frame of the Procrustes mean, not in the base's.
PLANTED_RECOVERY = 1e-6


def _frozen(a):
    a.setflags(write=False)
    return a


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@functools.lru_cache(maxsize=None)
def pool(N, m, kind="compact"):
    """fp32 [N, m, 3].  compact: noisy copies (0.5 A) of one blob of spread 5 A, each rigidly moved; far: the same with
    every other structure 1000 A from the origin; walk: independent random walks of 3.8 A steps."""
    rng = np.random.default_rng(7919 * N + 31 * m + {"compact": 0, "far": 1, "walk": 2}[kind])
    if kind == "walk":
        steps = rng.standard_normal((N, m, 3))
        steps *= 3.8 / np.linalg.norm(steps, axis=-1, keepdims=True)
        x = np.cumsum(steps, axis=1)
    else:
        base = rng.standard_normal((m, 3)) * 5.0
        x = base[None] + 0.5 * rng.standard_normal((N, m, 3))
    out = np.empty((N, m, 3))
    for s in range(N):
        shift = rng.standard_normal(3) * 3.0
        if kind == "far" and s % 2:
            shift = shift + np.array([1000.0, -500.0, 250.0])
        out[s] = x[s] @ _rotation(rng).T + shift
    return _frozen(out.astype(np.float32))


def rigid_basis(base):
    """The six infinitesimal rigid motions of base [m, 3] as orthonormal rows [6 or fewer, 3 m]."""
    m = base.shape[0]
    c = base - base.mean(0)
    rows = []
    for a in range(3):
        t = np.zeros((m, 3))
        t[:, a] = 1.0
        rows.append(t.reshape(-1))
        axis = np.zeros(3)
        axis[a] = 1.0
        rows.append(np.cross(axis, c).reshape(-1))
    q, r = np.linalg.qr(np.array(rows).T)
    return q[:, np.abs(np.diag(r)) > 1e-9].T


@functools.lru_cache(maxsize=None)
def planted(name):
    """-> (x fp32 [N, m, 3], modes [r, 3 m] orthonormal and orthogonal to the rigid motions of the base, lam [r] = the planted
    eigenvalues sigma_i^2): base + sum_i c_si sigma_i u_i with the columns of c exactly centred and orthogonal (c^T c = N I
    where N - 1 >= r), a random rigid motion per structure, rounded to fp32."""
    N, m, sigma = PLANTED[name]
    rng = np.random.default_rng(1000 + sorted(PLANTED).index(name))
    base = rng.standard_normal((m, 3)) * 5.0
    base -= base.mean(0)
    r = len(sigma)
    rigid = rigid_basis(base)
    u = rng.standard_normal((r, 3 * m))
    u -= (u @ rigid.T) @ rigid
    u = np.linalg.qr(u.T)[0].T
    c = rng.standard_normal((N, r))
    c -= c.mean(0)
    if N - 1 >= r:
        c = np.linalg.qr(c)[0] * np.sqrt(N)
        c -= c.mean(0)
    sig = np.array(sigma)
    x = base.reshape(-1)[None] + (c * sig) @ u
    out = np.empty((N, m, 3))
    for s in range(N):
        out[s] = x[s].reshape(m, 3) @ _rotation(rng).T + rng.standard_normal(3) * 3.0
    lam = sig ** 2 * (c ** 2).sum(0) / N
    return _frozen(out.astype(np.float32)), _frozen(u), _frozen(lam)


def weights(N, seed=3):
    w = np.random.default_rng(seed).uniform(0.2, 1.0, N)
    return _frozen(w)


# ------------------------------------------------------------------------------------------------------ Procrustes --
def total_weight(w):
    W = 0.0
    for v in w:                                       # ascending index
        W += float(v)
    return W


def align(xs, M):
    """xs [N, m, 3], M [m, 3] float64 -> (A [N, m, 3], R [N, 3, 3], t [N, 3], msd [N], e0n [N]) by ensemble_ref.kabsch."""
    N = xs.shape[0]
    A, R, t, msd, e0n = np.empty_like(xs), np.empty((N, 3, 3)), np.empty((N, 3)), np.empty(N), np.empty(N)
    for s in range(N):
        k = er.kabsch(xs[s], M)
        R[s], t[s], msd[s], e0n[s] = k["R"], k["t"], k["msd"], k["e0n"]
        A[s] = xs[s] @ k["R"].T + k["t"]
    return A, R, t, msd, e0n


def procrustes(x, sel=None, w=None, start=None, tol=1e-6, max_iter=100):
    """The rule of include/codlad_hip.h in float64 -> dict(mean, target, A, R, t, n_iter, step, status, finite, W)."""
    xs = np.asarray(x, dtype=np.float64)
    if sel is not None:
        xs = xs[:, np.asarray(sel)]
    N, m = xs.shape[:2]
    finite = np.isfinite(xs).all(axis=(1, 2))
    w = np.ones(N) if w is None else np.asarray(w, dtype=np.float64).copy()
    w[~finite] = 0.0
    W = total_weight(w)
    use = np.flatnonzero(w > 0)
    if start is None:
        start = int(use[0])
    M = xs[start] - xs[start].mean(0)
    for it in range(1, max_iter + 1):
        A = np.full_like(xs, np.nan)
        R, t = np.full((N, 3, 3), np.nan), np.full((N, 3), np.nan)
        A[use], R[use], t[use], _msd, _e0n = align(xs[use], M)
        new = np.einsum("s,skc->kc", w[use], A[use]) / W
        step = float(np.sqrt(((new - M) ** 2).sum(-1).mean()))
        if step <= tol:
            return dict(mean=new, target=M, A=A, R=R, t=t, n_iter=it, step=step, status="converged", finite=finite, W=W)
        if it == max_iter:
            return dict(mean=new, target=M, A=A, R=R, t=t, n_iter=it, step=step, status="limit", finite=finite, W=W)
        M = new


def iteration(xs, M, w):
    """One more reference iteration from M over the structures xs [N, m, 3] (all finite) with weights w -> the next mean."""
    A = align(np.asarray(xs, dtype=np.float64), np.asarray(M, dtype=np.float64))[0]
    return np.einsum("s,skc->kc", w, A) / total_weight(w)


# ------------------------------------------------------------------------------------------------------ covariance --
def covariance_ld(D, w, W, rows=None):
    """D [N, d] float64 (finite rows only), w [N] -> (C, T) in longdouble, C = sum_s w_s D_si D_sj / W and T the same sum of
    absolute values; `rows`: only these rows i."""
    Dl, wl = D.astype(LD), np.asarray(w, dtype=LD)
    left = Dl if rows is None else Dl[:, rows]
    C = (left * wl[:, None]).T @ Dl / LD(W)
    T = (np.abs(left) * wl[:, None]).T @ np.abs(Dl) / LD(W)
    return C, T


def cross_correlation(C):
    m = C.shape[0] // 3
    tr = np.einsum("acbc->ab", C.reshape(m, 3, m, 3))
    dg = np.diag(tr)
    with np.errstate(invalid="ignore", divide="ignore"):
        return tr / np.sqrt(np.outer(dg, dg))


def eigh_desc(C):
    lam, vec = np.linalg.eigh(C)
    return lam[::-1].copy(), vec[:, ::-1].T.copy()


def reference_pca(x, k, sel=None, w=None, **fit):
    """The whole chain in float64 -> dict(fit, D, C, lam [k], vec [k, d])."""
    f = procrustes(x, sel, w, **fit)
    use = np.flatnonzero(f["finite"])
    ww = np.ones(len(f["finite"])) if w is None else np.asarray(w, dtype=np.float64)
    D = (f["A"] - f["mean"]).reshape(len(ww), -1)
    C = (D[use] * ww[use, None]).T @ D[use] / f["W"]
    lam, vec = eigh_desc(C)
    return dict(fit=f, D=D, C=C, lam=lam[:k], vec=vec[:k])
