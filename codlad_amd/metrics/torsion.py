"""Torsion-space analysis of an ensemble (csrc/torsion_kernels.hip; the arithmetic and its bounds are stated in
include/codlad_hip.h): every structure as the unit vectors f_t = (cos theta_t, sin theta_t) of T backbone and side-chain
torsions, the periodicity-free representation of dihedral PCA (Mu, Nguyen and Stock 2005), and what a disordered ensemble
is analysed by in it: the table itself (torsion_features), per-torsion circular statistics (circular_stats, the torsional
counterpart of rmsf), principal components of the table (dihedral_pca, dihedral_pca_project: no superposition anywhere),
the TORSION DISTANCE |f_i - f_j| / sqrt(T) = sqrt(mean_t 2 (1 - cos dtheta_t)) - the RMS angular difference in radians for
small differences, at most 2 - of every pair of a pool or of two pools as one float64 matrix product (torsion_matrix), the
neighbour bitmap at a cut-off without the N x N table (torsion_neighbours), a list of pairs by the direct sum
(torsion_pairs), and Daura's clustering of the bitmap through cluster_neighbours, unchanged (cluster_torsion).  `quads` is
what dihedral_quads makes of a topology, or any integer [T, 4] table of atom indices."""
import math

import torch

from .. import _lib
from . import _inputs
from .cluster import CLUSTER_MAX_N, cluster_neighbours
from .pca import PCA_MAX_COMPONENTS, _eigen, _project
from .stereo import STEREO_COLUMNS, stereo_tables

TORSION_MAX_T = _lib.TORSION_MAX_T
TORSION_NAMES = STEREO_COLUMNS[:7]            # phi psi omega chi1 chi2 chi3 chi4

__all__ = ["TORSION_MAX_T", "TORSION_NAMES", "dihedral_quads", "torsion_features", "circular_stats", "dihedral_pca",
           "dihedral_pca_project", "torsion_matrix", "torsion_neighbours", "torsion_pairs", "cluster_torsion"]


def dihedral_quads(top, which=("phi", "psi")):
    """The torsions `which` (any of phi psi omega chi1 chi2 chi3 chi4, in that order of a residue) of a
    dataset_builder.Topology -> dict: quads int32 [T, 4], the atoms of every torsion the topology HAS (stereo_tables' rows
    without a -1: no phi at a chain start, no psi at a chain end, as many chi as the residue type), residue by residue;
    residue int64 [T] and column int64 [T] (index into TORSION_NAMES) of each.  On the host, kept on the topology."""
    which = (which,) if isinstance(which, str) else tuple(which)
    if not which or len(set(which)) != len(which) or any(w not in TORSION_NAMES for w in which):
        raise ValueError(f"dihedral_quads: which must be different names of {TORSION_NAMES}, got {which!r}")
    cols = sorted(TORSION_NAMES.index(w) for w in which)

    def build():
        sites = stereo_tables(top)[0][:, cols].to(torch.int64)                  # [R, len(cols), 4]
        has = (sites >= 0).all(-1)
        res, col = has.nonzero(as_tuple=True)
        return dict(quads=sites[has].to(torch.int32).contiguous(), residue=res.contiguous(),
                    column=torch.tensor(cols, dtype=torch.int64)[col].contiguous())
    return _inputs.cached(top, "_dihedral_quads", tuple(cols), build)


def _quads(quads, n_atoms, dev, what):
    """quads (dihedral_quads' dict or an integer [T, 4] table) -> int32 [T, 4] on dev; ValueError for a float table, another
    shape, T outside 1 .. TORSION_MAX_T or an index outside the atoms."""
    if isinstance(quads, dict):
        quads = quads["quads"]
    q = torch.as_tensor(quads)
    if q.is_floating_point() or q.is_complex() or q.dtype == torch.bool:
        raise ValueError(f"{what}: quads must be an integer [T, 4] table, got {q.dtype}")
    if q.dim() != 2 or q.shape[1] != 4:
        raise ValueError(f"{what}: quads must be an integer [T, 4] table, got {tuple(q.shape)}")
    if not 1 <= q.shape[0] <= TORSION_MAX_T:
        raise ValueError(f"{what}: 1 .. {TORSION_MAX_T} torsions, got {q.shape[0]}")
    if int(q.min()) < 0 or int(q.max()) >= n_atoms:
        raise ValueError(f"{what}: quads has an index outside [0, {n_atoms})")
    return q.to(device=dev, dtype=torch.int32).contiguous()


def _pool(x, quads, what, name="x"):
    """(the checked structures, quads on the device): a CPU tensor is refused first, then a pool that is too large, then
    the table."""
    x = _inputs.structures(x, f"{what}: {name}")
    if x.shape[0] > CLUSTER_MAX_N:
        raise ValueError(f"{what}: at most {CLUSTER_MAX_N} structures in one pool, got {x.shape[0]}")
    return x, _quads(quads, x.shape[1], x.device, what)


def _second(x, y, what, name):
    """The second pool of a call, on the first one's atoms and device."""
    y = _inputs.structures(y, f"{what}: {name}")
    if y.shape[0] > CLUSTER_MAX_N:
        raise ValueError(f"{what}: at most {CLUSTER_MAX_N} structures in one pool, got {y.shape[0]}")
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"{what}: the two pools have {x.shape[1]} and {y.shape[1]} atoms")
    if y.device != x.device:
        raise ValueError(f"{what}: the two pools are on {x.device} and {y.device}")
    return y


def _features(x, q):
    N, T = x.shape[0], q.shape[0]
    F = torch.empty(N, 2 * T, dtype=torch.float64, device=x.device)
    finite = _inputs.flags(N, x.device)
    p = _lib.ptr
    rc = _lib.lib().codlad_torsion_features(p(x), N, x.shape[1], p(q), T, p(F), p(finite), _lib.stream_ptr(x.device))
    _lib.check(rc, "codlad_torsion_features")
    return F, finite


def _mean(F, finite, w, want_D):
    N, K = F.shape
    dev = F.device
    scratch = _inputs.scratch("codlad_torsion_mean_scratch_bytes", N, K // 2, dev=dev)
    mean = torch.empty(K, dtype=torch.float64, device=dev)
    scal = torch.empty(_lib.PCA_SCALARS, dtype=torch.float64, device=dev)
    D = torch.empty(N, K, dtype=torch.float64, device=dev) if want_D else None
    p = _lib.ptr
    rc = _lib.lib().codlad_torsion_mean(p(F), p(finite), p(w), N, K // 2, p(mean), p(scal), p(D), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_torsion_mean")
    return mean, scal, D


def torsion_features(x, quads):
    """x [N, n, 3] (N <= 65 536), quads [T, 4] (T <= 2 048) -> (features float64 [N, T, 2] = (cos, sin) of every torsion,
    finite bool [N]).  A float64 sequence of + - * / sqrt on the fp32 coordinates, stated in the header: a numpy
    restatement gives the same bits.  A structure with a NaN or an infinity in an atom a quad names, or with a collinear
    quad (no angle exists), has finite False and a row of NaN; the others keep their bits."""
    x, q = _pool(x, quads, "torsion_features")
    F, finite = _features(x, q)
    return F.view(x.shape[0], q.shape[0], 2), finite.to(torch.bool)


def circular_stats(x, quads, weights=None):
    """Per torsion over the pool (weights [N] >= 0 make every average the weighted one) -> dict of float64 [T]: mean_cos,
    mean_sin (the resultant: the device's sums in an order that depends on N alone), resultant R = sqrt(C^2 + S^2),
    circular_variance = 1 - R (0: every structure has the angle; 1: no preferred angle - what rmsf is for coordinates),
    mean_angle in degrees by torch.atan2 of the two sums (the one transcendental, outside the kernels); finite bool [N],
    total_weight.  Structures that are not finite or have weight 0 take no part."""
    what = "circular_stats"
    x, q = _pool(x, quads, what)
    w = _inputs.weights(weights, x.shape[0], x.device, what, True)
    F, finite = _features(x, q)
    mean, scal, _ = _mean(F, finite, w, False)
    c, s = mean[0::2].contiguous(), mean[1::2].contiguous()
    R = torch.sqrt(c * c + s * s)
    return dict(mean_cos=c, mean_sin=s, resultant=R, circular_variance=1.0 - R, mean_angle=torch.rad2deg(torch.atan2(s, c)),
                finite=finite.to(torch.bool), total_weight=float(scal[_lib.PCA_SC_W]))


def _feature_covariance(D, w, finite, scal):
    N, d = D.shape
    dev = D.device
    scratch = _inputs.scratch("codlad_feature_covariance_scratch_bytes", N, d, dev=dev)
    cov = torch.empty(d, d, dtype=torch.float64, device=dev)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    p = _lib.ptr
    rc = _lib.lib().codlad_feature_covariance(p(D), p(w), p(finite), N, d, p(scal), p(cov), p(total), p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_feature_covariance")
    return cov, total


def dihedral_pca(x, quads, n_components=10, weights=None, rtol=1e-10, max_iter=1000, return_covariance=False):
    """Principal components of the pool in its torsions (dPCA): the features, their weighted mean, the deviations, the
    covariance [2 T, 2 T] as pca's float64 matrix product and its n_components <= min(64, 2 T) largest eigenpairs by pca's
    solver.  No superposition is involved: rigid motions of any structure change nothing.  -> dict in pca's vocabulary:
    mean float64 [T, 2], eigenvalues [k] (descending), components [k, T, 2] (orthonormal, the entry of largest magnitude
    positive), explained = eigenvalues / total_variance, total_variance, projections [N, k] (NaN rows for structures that
    are not finite), residuals [k], eig_iter, eig_status, finite bool [N], total_weight, quads; with return_covariance cov."""
    what = "dihedral_pca"
    x, q = _pool(x, quads, what)
    T = q.shape[0]
    k = _inputs.count(n_components, "n_components", min(PCA_MAX_COMPONENTS, 2 * T), what)
    rtol = _inputs.positive(rtol, "rtol", what)
    max_iter = _inputs.count(max_iter, "max_iter", _lib.PCA_MAX_ITER, what)
    w = _inputs.weights(weights, x.shape[0], x.device, what, True)
    F, finite = _features(x, q)
    mean, scal, D = _mean(F, finite, w, True)
    cov, total = _feature_covariance(D, w, finite, scal)
    evals, comps, resid, eig_iter, eig_status = _eigen(cov, k, rtol, max_iter)
    out = dict(mean=mean.view(T, 2), eigenvalues=evals, components=comps.view(k, T, 2), explained=evals / total[0],
               total_variance=total[0], projections=_project(D, comps), residuals=resid, eig_iter=eig_iter, eig_status=eig_status,
               finite=finite.to(torch.bool), total_weight=float(scal[_lib.PCA_SC_W]), quads=q)
    if return_covariance:
        out["cov"] = cov
    return out


def dihedral_pca_project(y, model):
    """The pool y [Ny, n, 3] on a model (dihedral_pca's dict): the deviations of its features from model["mean"] projected
    on model["components"] -> float64 [Ny, k]; NaN rows for structures that are not finite."""
    what = "dihedral_pca_project"
    if not isinstance(model, dict) or any(key not in model for key in ("mean", "components", "quads")):
        raise ValueError(f"{what}: model must be the dict dihedral_pca returns (mean, components, quads)")
    y, q = _pool(y, model["quads"], what, name="y")
    T = q.shape[0]
    mean, comps = model["mean"], model["components"]
    if tuple(mean.shape) != (T, 2) or comps.dim() != 3 or tuple(comps.shape[1:]) != (T, 2) or mean.device != y.device:
        raise ValueError(f"{what}: the model's mean {tuple(mean.shape)} and components {tuple(comps.shape)} do not match its "
                         f"{T} torsions (same device as y)")
    F, finite = _features(y, q)
    mean = mean.to(torch.float64).contiguous().view(1, 2 * T)
    D = torch.where(finite.to(torch.bool)[:, None], F - mean, torch.full_like(F, math.nan))      # dev_kernel's one subtraction
    return _project(D.contiguous(), comps.to(torch.float64).contiguous().view(comps.shape[0], 2 * T))


def _matrix(Fx, fx, Fy, fy, cut2, squared, want_matrix, want_bits):
    Na, K = Fx.shape
    Nb = 0 if Fy is None else Fy.shape[0]
    dev = Fx.device
    scratch = _inputs.scratch("codlad_torsion_matrix_scratch_bytes", Na, Nb, dev=dev)
    out = torch.empty(Na, Nb or Na, dtype=torch.float64, device=dev) if want_matrix else None
    bits = torch.empty(max(2, Na * ((Na + 63) // 64)), dtype=torch.int64, device=dev)[:Na * ((Na + 63) // 64)].view(Na, -1) \
        if want_bits else None
    p = _lib.ptr
    rc = _lib.lib().codlad_torsion_matrix(p(Fx), p(fx), Na, p(Fy), p(fy), Nb, K // 2, float(cut2), int(bool(squared)), p(out), p(bits),
                                          p(scratch), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_torsion_matrix")
    return out, bits


def torsion_matrix(x, quads, y=None, squared=False):
    """x [N, n, 3] (one pool, N <= 65 536) -> float64 [N, N] on the device: the torsion distance of every pair over the
    torsions `quads`; its square (the mean over the torsions of 2 (1 - cos dtheta)) with squared=True.  Symmetric to the
    bit, the diagonal exactly 0, and exactly 0 between two structures with the same features (a duplicate, an fp32-exact
    translate); the row and the column of a structure that is not finite are NaN.  An element depends on its two structures
    and quads alone, and a repeat gives the same bits.  With y [Nb, n, 3]: float64 [N, Nb], every structure of x against
    every structure of y (generated against true frames)."""
    what = "torsion_matrix"
    x, q = _pool(x, quads, what)
    if y is not None:
        y = _second(x, y, what, "y")
    Fx, fx = _features(x, q)
    Fy, fy = (None, None) if y is None else _features(y, q)
    return _matrix(Fx, fx, Fy, fy, 0.0, squared, True, False)[0]


def torsion_neighbours(x, quads, cutoff, return_matrix=False):
    """Who is within `cutoff` (a torsion distance in radians, a positive finite number) of whom -> rmsd_neighbours' dict:
    bits int64 [N, ceil(N / 64)] in its layout (cluster_neighbours takes it unchanged), finite bool [N], n = N, and with
    return_matrix torsion float64 [N, N].  Without return_matrix no N x N table is made."""
    c = _inputs.positive(cutoff, "cutoff", "torsion_neighbours")
    x, q = _pool(x, quads, "torsion_neighbours")
    F, finite = _features(x, q)
    out, bits = _matrix(F, finite, None, None, c * c, False, return_matrix, True)
    res = dict(bits=bits, finite=finite.to(torch.bool), n=x.shape[0])
    if return_matrix:
        res["torsion"] = out
    return res


def _pairs(Fa, Fb, pairs, per_torsion):
    dev = Fa.device
    K, T = pairs.shape[0], Fa.shape[1] // 2
    tmsd = torch.empty(max(K, 2), dtype=torch.float64, device=dev)[:K]
    terms = torch.empty(K, T, dtype=torch.float64, device=dev) if per_torsion else None
    p = _lib.ptr
    rc = _lib.lib().codlad_torsion_pairs(p(Fa), Fa.shape[0], p(Fb), Fb.shape[0], T, p(pairs), K, p(tmsd), p(terms), _lib.stream_ptr(dev))
    _lib.check(rc, "codlad_torsion_pairs")
    return tmsd, terms


def torsion_pairs(a, b, pairs, quads, per_torsion=False, squared=False):
    """The torsion distance (its square with squared=True) of the pairs [K, 2] (index into a [Na, n, 3], index into b [Nb,
    n, 3]) by the direct sum of (cos_a - cos_b)^2 + (sin_a - sin_b)^2 in float64: no cancellation, the route for a
    structure against its cluster centre -> float64 [K] (NaN where a structure is not finite).  With per_torsion: (that,
    float64 [K, T]): the term of every torsion, 2 (1 - cos dtheta_t) - where the two structures differ."""
    what = "torsion_pairs"
    a, q = _pool(a, quads, what, name="a")
    b = _second(a, b, what, "b")
    pairs = torch.as_tensor(pairs)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] == 0 or pairs.is_floating_point():
        raise ValueError(f"{what}: pairs must be a non-empty integer [K, 2] tensor, got {tuple(pairs.shape)}")
    lo, hi = pairs.min(0).values.tolist(), pairs.max(0).values.tolist()
    if min(lo) < 0 or hi[0] >= a.shape[0] or hi[1] >= b.shape[0]:
        raise ValueError(f"{what}: pairs has an index outside the pools ({a.shape[0]}, {b.shape[0]})")
    pairs = pairs.to(device=a.device, dtype=torch.int32).contiguous()
    Fa = _features(a, q)[0]
    Fb = _features(b, q)[0]
    tmsd, terms = _pairs(Fa, Fb, pairs, per_torsion)
    out = tmsd if squared else torch.sqrt(tmsd)
    return (out, terms) if per_torsion else out


def cluster_torsion(x, quads, cutoff, weights=None, return_matrix=False):
    """Daura's clustering of the pool x [N, n, 3] at the torsion-distance cut-off `cutoff` (radians): torsion_neighbours, then
    cluster_neighbours of its bitmap -> cluster's dict with centre_distance float64 [N] in the place of centre_rmsd (the
    torsion distance of every structure to the centre of its cluster, NaN for a structure that is not finite) and, with
    return_matrix, torsion [N, N].  centre_distance is read from the matrix when it was asked for; otherwise it is N pairs
    through torsion_pairs' kernel."""
    c = _inputs.positive(cutoff, "cutoff", "cluster_torsion")
    x, q = _pool(x, quads, "cluster_torsion")
    N = x.shape[0]
    if weights is not None:
        _inputs.weights(weights, N, x.device, "cluster_torsion", False)              # refused before any launch
    F, finite = _features(x, q)
    table, bits = _matrix(F, finite, None, None, c * c, False, return_matrix, True)
    out = cluster_neighbours(bits, N, finite=finite, weights=weights)
    lab = out["labels"].to(torch.int64)
    ok = lab >= 0
    idx = torch.arange(N, device=x.device)
    centre_of = torch.where(ok, out["centres"].to(torch.int64)[lab.clamp(min=0)], idx) if out["n_clusters"] else idx
    if return_matrix:
        cd = table[idx, centre_of]
    else:
        pairs = torch.stack((idx, centre_of), 1).to(torch.int32).contiguous()
        cd = torch.sqrt(_pairs(F, F, pairs, False)[0])
    out["centre_distance"] = torch.where(ok, cd, torch.full_like(cd, math.nan))
    out["finite"] = finite.to(torch.bool)
    out["bits"] = bits
    if return_matrix:
        out["torsion"] = table
    return out
