"""Essential dynamics on the device (codlad_amd/csrc/pca_kernels.hip through codlad_amd.metrics) against tests/pca_ref.py.
Every layer is held to the float64 / longdouble reference at the device's own input to that layer: the alignment at the
device's last target, the mean at the device's transforms, the covariance and the RMSF at the device's deviations, the
eigenpairs at the device's covariance, the projections at the device's deviations and components.  The bounds are derived
from N, d and 2^-52 (include/codlad_hip.h), not fitted."""
import functools

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import ensemble_ref as er
from tests import memcheck
from tests import pca_ref as pr
from tests.test_saxs import _cli, dev

pytestmark = pytest.mark.gpu
EPS, LD = pr.EPS, pr.LD
ALL_SHAPES = pr.SHAPES + (pr.LARGE_DIM, pr.MANY)
_RUN = {}


def host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)


def same_dict(a, b):
    bad = [k for k in a if not (same(a[k], b[k]) if isinstance(a[k], np.ndarray) else
                                (a[k] == b[k] or (isinstance(a[k], float) and a[k] != a[k] and b[k] != b[k])))]
    assert not bad, bad
    return True


def weights_of(N, weighted):
    return pr.weights(N) if weighted else None


def device_cov(N, m, kind, weighted=False):
    """covariance() and rmsf() of a pool of pca_ref on the device, computed once and shared."""
    key = (N, m, kind, weighted)
    if key not in _RUN:
        w = weights_of(N, weighted)
        x = dev(pr.pool(N, m, kind))
        o = host(metrics.covariance(x, weights=None if w is None else dev(w)))
        o["rmsf"] = metrics.rmsf(x, weights=None if w is None else dev(w)).cpu().numpy()
        for v in o.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _RUN[key] = o
    return _RUN[key]


def device_pca(name, k=None):
    """pca() of a planted pool on the device, computed once and shared."""
    key = ("planted", name, k)
    if key not in _RUN:
        x, _u, lam = pr.planted(name)
        o = host(metrics.pca(dev(x), n_components=k or len(lam), return_covariance=True, return_deviations=True))
        _RUN[key] = o
    return _RUN[key]


@functools.lru_cache(maxsize=None)
def reference_fit(N, m, kind, weighted):
    return pr.procrustes(pr.pool(N, m, kind), w=weights_of(N, weighted))


def cases():
    return [(N, m, kind, (i % 3 == 1)) for i, (N, m, kind) in enumerate(ALL_SHAPES)]


def moved_ld(x, R, t):
    """x [N, m, 3] fp32, the device's transforms -> A and the sum of the magnitudes of its terms, in longdouble."""
    xl, Rl, tl = x.astype(LD), R.astype(LD), t.astype(LD)
    A = np.einsum("skc,src->skr", xl, Rl) + tl[:, None, :]
    mag = np.einsum("skc,src->skr", np.abs(xl), np.abs(Rl)) + np.abs(tl)[:, None, :]
    return A, mag


@pytest.mark.parametrize("N,m,kind,weighted", cases(), ids=lambda v: str(v))
def test_alignment_and_mean(N, m, kind, weighted):
    x = pr.pool(N, m, kind)
    w = np.ones(N) if not weighted else pr.weights(N)
    o = device_cov(N, m, kind, weighted)
    ref = reference_fit(N, m, kind, weighted)
    assert o["status"] == "converged" == ref["status"] and o["finite"].all() and o["start"] == 0
    print(f"({N}, {m}, {kind}): n_iter device {o['n_iter']} reference {ref['n_iter']}, step {o['step']:.2e}")
    assert abs(o["n_iter"] - ref["n_iter"]) <= 1 and o["step"] <= 1e-6
    assert o["total_weight"] == pr.total_weight(w)
    # every transform reproduces the reference's superposed msd on the device's last target
    A, mag = moved_ld(x, o["R"], o["t"])
    msd_dev = ((A - o["target"].astype(LD)) ** 2).sum(-1).mean(-1).astype(np.float64)
    _A, _R, _t, msd_ref, e0n = pr.align(x.astype(np.float64), o["target"])
    lim = er.msd_bound(m, e0n)
    ratio = np.abs(msd_dev - np.maximum(msd_ref, 0.0)) / np.where(lim > 0, lim, 1.0)
    print(f"  max |msd_dev - msd_ref| / bound {float(ratio.max()):.3f}")
    assert (np.abs(msd_dev - np.maximum(msd_ref, 0.0)) <= lim).all()
    # the mean is the weighted average of the device's own superposed structures: 4 roundings for A_s, then a sum of N terms
    # in chunks (at most N + 32 additions) and a division -> (N + 40) 2^-52 sum |terms|
    W = LD(pr.total_weight(w))
    avg = (A * w.astype(LD)[:, None, None]).sum(0) / W
    bound = (N + 40) * EPS * (mag * w.astype(LD)[:, None, None]).sum(0) / W
    err = np.abs(o["mean"].astype(LD) - avg)
    print(f"  max |mean - average| / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # one more reference iteration from the device's mean moves it by no more than tol plus that bound
    nxt = pr.iteration(x, o["mean"], w)
    move = float(np.sqrt(((nxt - o["mean"]) ** 2).sum(-1).mean()))
    assert move <= 1e-6 + float(np.sqrt((bound.astype(np.float64) ** 2).sum(-1).mean())), move


def cov_rows(d):
    if d <= 1024:
        return None
    rows = {0, 1, 63, 64, 65, 127, 128, d - 65, d - 64, d - 2, d - 1} | set(np.random.default_rng(4).integers(0, d, 24).tolist())
    return np.array(sorted(rows))


@pytest.mark.parametrize("N,m,kind,weighted", cases(), ids=lambda v: str(v))
def test_rmsf_and_covariance_at_the_device_deviations(N, m, kind, weighted):
    w = np.ones(N) if not weighted else pr.weights(N)
    o = device_cov(N, m, kind, weighted)
    D, C, d = o["deviations"], o["cov"], 3 * m
    W = pr.total_weight(w)
    assert D.shape == (N, d) and C.shape == (d, d) and C.dtype == np.float64 and np.isfinite(C).all()
    assert same(C, C.T)                                                  # symmetric to the bit
    rows = cov_rows(d)
    ref, T = pr.covariance_ld(D, w, W, rows)
    got = C if rows is None else C[rows]
    err, lim = np.abs(got.astype(LD) - ref), (N + 34) * EPS * T
    print(f"({N}, {m}, {kind}): max |C_dev - C_ref| / bound {float((err / np.where(lim > 0, lim, 1)).max()):.3f}")
    assert (err <= lim).all(), np.argwhere(err > lim)[:5].tolist()
    tr = 0.0
    for i in range(d):
        tr += float(C[i, i])
    assert float(o["total_variance"]) == tr
    corr = o["cross_correlation"]
    var = np.einsum("acac->a", C.reshape(m, 3, m, 3))
    assert corr.shape == (m, m) and same(corr, corr.T)
    assert (np.diag(corr)[var > 0] == 1.0).all() and np.isnan(np.diag(corr)[var == 0]).all()
    if (var > 0).all():
        want = pr.cross_correlation(C)
        mag = np.einsum("acbc->ab", np.abs(C).reshape(m, 3, m, 3)) / np.sqrt(np.outer(var, var))
        assert (np.abs(corr - want) <= 8 * EPS * mag).all()
    # the RMSF from its own sum: N fused multiply-adds, a division, a root
    want = np.sqrt((w.astype(LD)[:, None] * (D.astype(LD) ** 2).reshape(N, m, 3).sum(-1)).sum(0) / LD(W))
    assert o["rmsf"].shape == (m,) and (np.abs(o["rmsf"].astype(LD) - want) <= (N + 6) * EPS * want).all()


def round_term(C):
    """What float64 evaluation of C v costs: d products per element, |C v - fl(C v)|_2 <= d 2^-52 |C|_F |v|, with a factor 8
    for the two sides (device and numpy), the Rayleigh-Ritz rotation and the normalisation."""
    return 8 * C.shape[0] * EPS * float(np.linalg.norm(C))


def check_eigenpairs(o, k):
    C = o["cov"]
    d = C.shape[0]
    b = min(k + 8, d)
    th, V = o["eigenvalues"], o["components"].reshape(k, d)
    lam, vec = pr.eigh_desc(C)
    rt = round_term(C)
    assert o["eig_status"] == "converged" and np.isfinite(th).all() and np.isfinite(V).all()
    assert (np.diff(th) <= 0).all()
    res = np.linalg.norm(V @ C - th[:, None] * V, axis=1)
    print(f"  eig_iter {o['eig_iter']}, max residual / (rtol theta_1) {float(res.max() / (1e-10 * th[0])):.3f}, "
          f"max |theta - lambda| {float(np.abs(th - lam[:k]).max()):.2e}")
    assert (o["residuals"] <= 1e-10 * th[0]).all() and (res <= 1e-10 * th[0] + rt).all()
    assert (np.abs(th - lam[:k]) <= res + rt).all()
    # orthonormal: Gram-Schmidt twice leaves d-term dot products (2 d 2^-52 with the normalisation), the Jacobi rotations of
    # up to ten sweeps 4 roundings each on b / 2 pairs a column, the product Q S b more
    gram = V @ V.T
    assert (np.abs(gram - np.eye(k)) <= (4 * d + 64 * b) * EPS).all(), float(np.abs(gram - np.eye(k)).max())
    big = np.abs(V).argmax(axis=1)                                      # the first among equals
    assert (V[np.arange(k), big] > 0).all()
    assert same(o["explained"], th / o["total_variance"])
    return th, V, lam, vec, res, rt


@pytest.mark.parametrize("name", ["plain", "three tiles"])
def test_eigenpairs_of_a_planted_spectrum(name):
    _x, _u, planted_lam = pr.planted(name)
    k = len(planted_lam)
    o = device_pca(name)
    th, V, lam, vec, res, rt = check_eigenpairs(o, k)
    # the device against the reference at the device's covariance; the reference against the truth is test_pca_host.py's
    assert (np.abs(lam[:k] - planted_lam) <= pr.PLANTED_RECOVERY * planted_lam[0]).all()
    for i in range(k):
        gap = min(abs(lam[i] - lam[j]) for j in range(len(lam)) if j != i)
        dot = float(V[i] @ vec[i])
        assert np.linalg.norm(V[i] - np.sign(dot) * vec[i]) <= 2 * (res[i] + rt) / gap + 4 * len(lam) * EPS


def test_equal_eigenvalues_are_compared_through_the_projector():
    o = device_pca("equal pair")
    th, V, lam, vec, res, rt = check_eigenpairs(o, 4)
    gap = min(lam[0] - lam[1], lam[2] - lam[3])
    P_dev, P_ref = V[1:3].T @ V[1:3], vec[1:3].T @ vec[1:3]
    lim = 2 * (float(np.linalg.norm(res[1:3])) + 2 * rt) / gap + 8 * len(lam) * EPS
    print(f"  |P_dev - P_ref|_2 {np.linalg.norm(P_dev - P_ref, 2):.2e}, bound {lim:.2e}, lambda_2 - lambda_3 {lam[1] - lam[2]:.2e}")
    assert np.linalg.norm(P_dev - P_ref, 2) <= lim


def test_rank_deficient_pool_gives_zeros_and_orthonormal_components():
    o = device_pca("rank deficient", 4)                                # N = 3: rank 2 at most
    th, V, lam, vec, res, rt = check_eigenpairs(o, 4)
    assert (th[:2] > 0.1).all() and (np.abs(th[2:]) <= res[2:] + rt).all()
    assert not np.isnan(o["projections"]).any() and not np.isnan(o["rmsf"]).any()
    one = host(metrics.pca(dev(pr.pool(1, 21)), n_components=2))       # a single structure: no variance at all
    assert np.isfinite(one["eigenvalues"]).all() and (np.abs(one["eigenvalues"]) <= 1e-20).all()
    assert (np.abs(one["components"].reshape(2, -1) @ one["components"].reshape(2, -1).T - np.eye(2)) <= (4 * 63 + 64 * 10) * EPS).all()
    tiny = host(metrics.pca(dev(pr.pool(2, 1)), n_components=3))        # d = 3 = b: the block is the whole space
    assert np.isfinite(tiny["components"]).all() and np.isfinite(tiny["eigenvalues"]).all()


@pytest.mark.parametrize("name", ["plain", "three tiles", "equal pair"])
def test_projections(name):
    x, _u, lam = pr.planted(name)
    o = device_pca(name)
    k, m = len(lam), x.shape[1]
    D, V = o["deviations"], o["components"].reshape(k, -1)
    want = D.astype(LD) @ V.astype(LD).T
    lim = (3 * m + 1) * EPS * (np.abs(D).astype(LD) @ np.abs(V).astype(LD).T)
    assert o["projections"].shape == (x.shape[0], k) and (np.abs(o["projections"].astype(LD) - want) <= lim).all()
    # The pool itself through pca_project is superposed on the mean, not on the target of the last iteration, which lies
    # `step` (RMS per atom, so step sqrt(m) in all) away: for structures this close to the mean the rotation follows a
    # change of the target with a factor below 2 and the translation with 1, and a projection on a unit vector is no
    # longer than the change of the deviation -> 4 step sqrt(m), plus the rounding of a projection
    model = {k2: (dev(v) if isinstance(v, np.ndarray) else v) for k2, v in o.items() if k2 in ("mean", "components")}
    again = metrics.pca_project(dev(x), model).cpu().numpy()
    err = np.abs(again - o["projections"])
    print(f"{name}: max |pca_project - projections| {float(err.max()):.2e}, step {o['step']:.2e}")
    assert (err <= 4 * o["step"] * np.sqrt(m) + 2 * lim.astype(np.float64)).all()
    # another pool: translated copies, whose fp32 coordinates (spacing 2^-19 up to 32 A) move by 2e-6 each, 3 m of them
    other = metrics.pca_project(dev(x[:5] + np.float32(0.25)), model).cpu().numpy()
    assert other.shape == (5, k) and (np.abs(other - again[:5]) <= 4 * o["step"] * np.sqrt(m) + 2e-6 * 3 * m).all()


def run_all(x, w, k):
    """Every output of every entry of the module for one pool, as host arrays."""
    wd = None if w is None else dev(w)
    xd = dev(x)
    p = host(metrics.pca(xd, n_components=k, weights=wd, return_covariance=True, return_deviations=True, max_iter=40))
    ms = host(metrics.mean_structure(xd, weights=wd))
    out = {f"pca.{a}": v for a, v in p.items() if a != "sel"}
    out.update({f"mean.{a}": v for a, v in ms.items()})
    out["rmsf"] = metrics.rmsf(xd, weights=wd).cpu().numpy()
    out["project"] = metrics.pca_project(xd, {"mean": dev(p["mean"]), "components": dev(p["components"])}).cpu().numpy()
    return out


def test_uniform_weights_give_the_bits_of_no_weights():
    x = pr.planted("plain")[0]
    plain = run_all(x, None, 4)
    assert same_dict(plain, run_all(x, np.ones(x.shape[0]), 4))
    half = run_all(x, np.full(x.shape[0], 0.5), 4)                     # a power of two scales every sum exactly
    skip = ("pca.total_weight", "mean.total_weight")
    assert same_dict({k: v for k, v in plain.items() if k not in skip}, {k: v for k, v in half.items() if k not in skip})
    assert same_dict(plain, run_all(x, None, 4))                        # a replay


def test_a_structure_without_weight_or_with_a_nan_changes_nothing_for_the_others():
    x = pr.planted("plain")[0].copy()
    N = x.shape[0]
    out = np.array([0, 7])
    keep = np.setdiff1d(np.arange(N), out)
    w = pr.weights(N).copy()
    w[out] = 0.0
    a = run_all(x, w, 4)
    assert a["pca.start"] == 1 and a["pca.finite"].all() and a["pca.status"] == "converged"
    other = x.copy()
    other[out] = pr.pool(2, x.shape[1], "far")                          # whatever a structure of weight 0 holds
    b = run_all(other, w, 4)
    bad = x.copy()
    bad[0, 3, 1] = np.nan
    bad[7, 0, 0] = np.inf
    w1 = pr.weights(N).copy()                                           # the weights of the two do not matter either
    c = run_all(bad, w1, 4)
    assert c["pca.finite"].tolist() == [i not in (0, 7) for i in range(N)] and c["pca.start"] == 1
    per_structure = ("pca.R", "pca.t", "pca.deviations", "pca.projections", "mean.R", "mean.t", "project", "pca.finite", "mean.finite")
    for k in a:
        if k in per_structure:
            assert same(a[k][keep], b[k][keep]) and same(a[k][keep], c[k][keep]), k
        elif k in ("pca.total_weight", "mean.total_weight"):
            assert a[k] == b[k] == pr.total_weight(w)
        else:
            assert same_dict({k: a[k]}, {k: b[k]}) and same_dict({k: a[k]}, {k: c[k]})
    for k in ("pca.R", "pca.t", "pca.deviations", "pca.projections", "project"):
        assert np.isnan(c[k][out]).all() and np.isfinite(a[k][out]).all(), k
    # against the pool without the two: the same numbers up to the order of the sums
    d = run_all(x[keep], w[keep], 4)
    lim = (N + 40) * EPS * (np.abs(a["pca.mean"]) + 20.0)
    assert (np.abs(d["pca.mean"] - a["pca.mean"]) <= 1e-6 + lim).all() and abs(d["pca.n_iter"] - a["pca.n_iter"]) <= 1
    assert (np.abs(d["pca.eigenvalues"] - a["pca.eigenvalues"]) <= 1e-5 * a["pca.eigenvalues"][0]).all()


def test_no_usable_structure_is_refused_or_reported():
    x = pr.pool(15, 22)
    with pytest.raises(ValueError, match="every weight is 0"):
        metrics.pca(dev(x), 2, weights=dev(np.zeros(15)))
    with pytest.raises(ValueError, match="has weight 0"):
        w = np.ones(15)
        w[3] = 0
        metrics.mean_structure(dev(x), weights=dev(w), start=3)
    bad = np.full_like(x, np.nan)
    o = host(metrics.mean_structure(dev(bad)))                          # only the device can know
    assert o["status"] == "no_weight" and not o["finite"].any() and np.isnan(o["mean"]).all() and np.isnan(o["R"]).all()
    assert o["total_weight"] == 0.0 and o["n_iter"] == 0
    one_bad = x.copy()
    one_bad[4] = np.nan
    o = host(metrics.mean_structure(dev(one_bad), start=4))
    assert o["status"] == "no_weight"
    sel = [0, 2, 5, 21]
    s = host(metrics.mean_structure(dev(x), sel=sel))
    full = host(metrics.mean_structure(dev(np.ascontiguousarray(x[:, sel]))))
    assert same_dict(s, full)                                           # a selection is the pool of the selected atoms


@pytest.mark.parametrize("key", [(1, 21, "compact"), (65, 65, "compact"), (130, 43, "planted"), pr.LARGE_DIM, (1030, 2, "compact")],
                         ids=lambda v: str(v))
def test_buffers_are_written_before_they_are_read_and_within_bounds(key):
    N, m, kind = key
    x = pr.planted("plain")[0] if kind == "planted" else pr.pool(N, m, kind)
    w = pr.weights(N) if N > 1 else None
    got = {}
    for fill in memcheck.FILLS:
        with memcheck.patched_allocations(fill):
            got[fill] = run_all(x, w, min(4, 3 * m))
            torch.cuda.synchronize()
        assert memcheck.zones_intact()
        memcheck.release()
    for fill in memcheck.FILLS[1:]:
        assert same_dict(got["zero"], got[fill]), fill
    assert same_dict(got["zero"], run_all(x, w, min(4, 3 * m)))          # and without the guards: a replay


def test_cli_pca_end_to_end(tmp_path):
    files, stdout = _cli(tmp_path, "--pca", "3")
    means = sorted(f for f in files if f.endswith("_pca_mean.npy"))
    assert len(means) == 4 and "essential dynamics" in stdout and stdout.count("pca_total_variance") == 4      # four proteins
    for f in means:
        stem = f[:-len("_pca_mean.npy")]
        mean, ev = np.load(files[f]), np.load(files[f"{stem}_pca_eigenvalues.npy"])
        comp, proj, fl = (np.load(files[f"{stem}_{s}.npy"]) for s in ("pca_components", "pca_projections", "rmsf"))
        xyz = np.load(files[f"{stem}_xyz_recon.npy"])
        pool, m = xyz.shape[0] * xyz.shape[1], mean.shape[0]
        assert mean.shape == (m, 3) and ev.shape == (3,) and comp.shape == (3, m, 3) and proj.shape == (pool, 3) and fl.shape == (m,)
        assert mean.dtype == ev.dtype == comp.dtype == proj.dtype == fl.dtype == np.float64 and m < xyz.shape[2]      # the CA atoms
        assert (np.diff(ev) <= 0).all() and (ev >= -1e-12).all() and (fl >= 0).all()
        assert (np.abs(comp.reshape(3, -1) @ comp.reshape(3, -1).T - np.eye(3)) <= 1e-12).all()
    import os
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test.py"),
                          "--synthetic", "--pca", "0"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert res.returncode != 0 and "--pca takes the number of components, 1 .. 64" in res.stderr
