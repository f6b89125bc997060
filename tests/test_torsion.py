"""The torsion kernels on the device against tests/torsion_ref.py: the features to the bit of the float64 restatement,
every element of the matrix within the header's bound of the longdouble DIRECT sum over those features (the bound comes
from the operation count of the header; it is not fitted), exact zeros for a duplicate and an fp32-exact translate,
symmetry, repeats, permutations and two pools to the bit, the bitmap on EVERY pair of cases whose cut-off the CPU suite has
shown to leave no pair undecided, defined results for non-finite input, the pair route and its per-torsion rows, the
circular statistics, dihedral PCA on the device's own covariance, the clustering, and tests/memcheck.py around the
launches.  Every accuracy test prints the largest measured fraction of its bound; on an MI355X: matrix 0.25 (at T = 1;
0.12 at T = 9 with 1 473 structures, 0.04 at T = 33, 0.007 at T = 129, 0.0001 at T = 2 048), two pools 0.024, pair route 0.11,
per-torsion terms 0.46, resultant 0.017, covariance 0.029; mean_angle against numpy.arctan2 of the device's sums: 2.8e-14
degrees (one ulp of an angle above 128) where 2e-13 is allowed."""
import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import cluster_ref as cr
from tests import memcheck as mc
from tests import torsion_ref as tr
from tests.polymer_ref import walk
from tests.test_saxs import dev

pytestmark = pytest.mark.gpu
LD = tr.LD
EPS = tr.EPS


def _np(t):
    return t.detach().cpu().numpy()


def _q(c):
    return torch.from_numpy(np.array(c["quads"]))


@pytest.mark.parametrize("N,T", tr.CASES)
def test_features_to_the_bit_and_every_element_of_the_matrix_within_the_header_bound(N, T):
    c = tr.case(N, T)
    x, q = dev(c["x"]), _q(c)
    F, finite = metrics.torsion_features(x, q)
    assert F.dtype == torch.float64 and tuple(F.shape) == (N, T, 2) and finite.dtype == torch.bool and bool(finite.all())
    assert mc.same_bits(F.reshape(N, 2 * T), torch.from_numpy(np.array(c["F"])))
    sq = metrics.torsion_matrix(x, q, squared=True)
    assert sq.dtype == torch.float64 and tuple(sq.shape) == (N, N)
    f = tr.worst(_np(sq), c["tmsd"], c["scale"], tr.matrix_bound(T))
    print(f"N{N}-T{T}: largest fraction of the matrix bound: {f:.4f}")
    assert f <= 1.0 and not bool(torch.isnan(sq).any())
    assert mc.same_bits(sq, sq.T.contiguous()) and bool((sq.diagonal() == 0).all())
    assert mc.same_bits(metrics.torsion_matrix(x, q), torch.sqrt(sq))
    assert mc.same_bits(sq, metrics.torsion_matrix(x, q, squared=True))          # a repeat
    assert float(sq.max()) <= 4.0


def test_non_finite_input_has_a_defined_result():
    N, T = 70, 9
    x0 = walk(N, T + 3, seed=2, n_extra=1)               # atom T + 3 is named by no quad
    q = torch.from_numpy(tr.chain_quads(T))
    c0 = metrics.cluster_torsion(dev(x0), q, 1.3, return_matrix=True)
    F0 = metrics.torsion_features(dev(x0), q)[0]
    assert _np(c0["finite"]).all()
    keep = [i for i in range(N) if i not in (1, 66)]
    fin = np.ones(N, dtype=bool)
    fin[[1, 66]] = False
    for kind in ("nan", "inf", "-inf", "collinear"):
        x = x0.copy()
        if kind == "collinear":
            # four atoms on a line, on an integer grid: the bond vectors are exact multiples of one another
            x[1, 3:7] = np.array([1.0, 2.0, 3.0], dtype=np.float32) + np.arange(4, dtype=np.float32)[:, None] * np.array([1.0, 2.0, -1.0], dtype=np.float32)
            x[66, 0:3] = x[66, 0]                        # three coincident atoms
        else:
            x[1, 4, 1] = x[66, T + 2, 0] = float(kind)
        x[2, T + 3, 2] = np.nan                          # an atom no quad names: changes nothing
        F, finite = metrics.torsion_features(dev(x), q)
        want, ok = tr.features64(x, tr.chain_quads(T))
        assert (ok == fin).all() and (_np(finite) == fin).all() and mc.same_bits(F.reshape(N, -1), torch.from_numpy(want))
        assert torch.isnan(F[[1, 66]]).all() and mc.same_bits(F[keep].contiguous(), F0[keep].contiguous())
        out = metrics.cluster_torsion(dev(x), q, 1.3, return_matrix=True)
        d = out["torsion"]
        assert (_np(out["finite"]) == fin).all() and torch.isnan(d[[1, 66]]).all() and torch.isnan(d[:, [1, 66]]).all()
        assert mc.same_bits(d[keep][:, keep].contiguous(), c0["torsion"][keep][:, keep].contiguous())
        bits, bits0 = cr.unpack(_np(out["bits"]), N), cr.unpack(_np(c0["bits"]), N)
        assert not bits[[1, 66]].any() and not bits[:, [1, 66]].any() and not bits[:, N:].any()
        assert (bits[keep][:, keep] == bits0[keep][:, keep]).all() and bits[keep, keep].all()
        lab = _np(out["labels"])
        assert lab[1] == -1 and lab[66] == -1 and (lab[keep] >= 0).all()
        assert (lab == cr.daura(bits[:, :N], finite=fin)["labels"]).all() and np.isnan(_np(out["centre_distance"])[[1, 66]]).all()
        direct, terms = metrics.torsion_pairs(dev(x), dev(x), torch.tensor([[0, 1], [2, 3], [66, 5]]), q, per_torsion=True)
        assert np.isnan(_np(direct)).tolist() == [True, False, True] and torch.isnan(terms[[0, 2]]).all() and torch.isfinite(terms[1]).all()
        st = metrics.circular_stats(dev(x), q)
        assert st["total_weight"] == N - 2 and torch.isfinite(st["resultant"]).all()
        assert mc.same_bits(st["mean_cos"], metrics.circular_stats(dev(x0[keep]), q)["mean_cos"])      # one chunk either way
        cross = metrics.torsion_matrix(dev(x0[:5]), q, y=dev(x))
        assert torch.isnan(cross[:, [1, 66]]).all() and mc.same_bits(cross[:, keep].contiguous(), c0["torsion"][:5][:, keep].contiguous())


def test_equal_features_are_at_exactly_zero_and_bits_do_not_depend_on_the_pool():
    N, T = 130, 33
    c = tr.case(N, T)
    x = c["x"].copy()
    quads = _q(c)
    g, moved = tr.translated(walk(4, T + 3, seed=7))
    x[0:4], x[64:68] = g, moved
    x[100], x[129] = x[31], x[31]                        # duplicates in other blocks
    xd = dev(x)
    F = metrics.torsion_features(xd, quads)[0]
    assert mc.same_bits(F[0:4].contiguous(), F[64:68].contiguous())               # the translation keeps every difference's bits
    sq = metrics.torsion_matrix(xd, quads, squared=True)
    for i in range(4):
        assert float(sq[i, 64 + i]) == 0.0 and float(sq[64 + i, i]) == 0.0 and float(sq[i, (i + 1) % 4]) > 0.0
    for i, j in ((31, 100), (31, 129), (100, 129)):
        assert float(sq[i, j]) == 0.0 and float(sq[j, i]) == 0.0
    assert mc.same_bits(sq[31].contiguous(), sq[100].contiguous()) and mc.same_bits(sq[31].contiguous(), sq[129].contiguous())
    assert mc.same_bits(sq, sq.T.contiguous())
    d = metrics.torsion_matrix(xd, quads)
    assert float(d[31, 100]) == 0.0 and mc.same_bits(d, torch.sqrt(sq))
    perm = torch.from_numpy(np.random.default_rng(5).permutation(N)).to(xd.device)
    assert mc.same_bits(metrics.torsion_matrix(xd[perm].contiguous(), quads, squared=True), sq[perm][:, perm].contiguous())
    for i, j in ((5, 77), (64, 129), (63, 64)):          # two structures alone, in either order, and inside the pool
        two = metrics.torsion_matrix(xd[[i, j]].contiguous(), quads, squared=True)
        assert mc.same_bits(two[0, 1], sq[i, j]) and mc.same_bits(two[1, 0], sq[i, j])
        assert mc.same_bits(metrics.torsion_matrix(xd[[j, i]].contiguous(), quads, squared=True)[0, 1], sq[i, j])


@pytest.mark.parametrize("Na,Nb", [(65, 3), (3, 130)])
def test_two_pools(Na, Nb):
    T = 33
    a, b = tr.case(Na, T), tr.case(Nb, T)
    xa, xb, q = dev(a["x"]), dev(b["x"]), _q(a)
    tmsd, scale = tr.tmsd_cross(a["F"], b["F"])
    got = metrics.torsion_matrix(xa, q, y=xb, squared=True)
    assert tuple(got.shape) == (Na, Nb)
    f = tr.worst(_np(got), tmsd, scale, tr.matrix_bound(T))
    print(f"cross-{Na}x{Nb}: largest fraction of the matrix bound: {f:.4f}")
    assert f <= 1.0
    assert mc.same_bits(got, metrics.torsion_matrix(xb, q, y=xa, squared=True).T.contiguous())          # swapped: the transpose
    joined = metrics.torsion_matrix(torch.cat((xa, xb)), q, squared=True)
    assert mc.same_bits(got, joined[:Na, Na:].contiguous())
    assert mc.same_bits(metrics.torsion_matrix(xa, q, y=xb), torch.sqrt(got))
    own = metrics.torsion_matrix(xa, q, y=xa.clone())
    assert bool((own.diagonal() == 0).all()) and bool((own.min(1).values == 0).all())


@pytest.mark.parametrize("N,T", tr.BITMAP_CASES)
def test_the_bitmap_is_the_reference_decision_on_every_pair(N, T):
    c = tr.case(N, T)
    cutoff = tr.cutoff_of(c)
    assert not tr.undecided(c, cutoff * cutoff)[~np.eye(N, dtype=bool)].any()                 # what the CPU suite has shown
    want = np.array(c["tmsd"] <= cutoff * cutoff)
    np.fill_diagonal(want, True)
    x, q = dev(c["x"]), _q(c)
    for return_matrix in (False, True):
        out = metrics.torsion_neighbours(x, q, cutoff, return_matrix=return_matrix)
        got = cr.unpack(_np(out["bits"]), N)
        assert out["bits"].dtype == torch.int64 and tuple(out["bits"].shape) == (N, (N + 63) // 64) and out["n"] == N
        assert (got[:, :N] == want).all() and not got[:, N:].any() and _np(out["finite"]).all()
        assert ("torsion" in out) == return_matrix
    assert mc.same_bits(out["torsion"], metrics.torsion_matrix(x, q))
    res = metrics.cluster_torsion(x, q, cutoff)
    ref = cr.daura(got[:, :N])
    assert (_np(res["labels"]) == ref["labels"]).all() and (_np(res["centres"]) == ref["centres"]).all()
    assert (_np(res["sizes"]) == ref["sizes"]).all() and res["n_clusters"] == ref["n_clusters"]


def test_the_bitmap_alone_allocates_no_table():
    N, T = 1473, 9
    c = tr.case(N, T)
    q = _q(c)
    mc.release()
    try:
        with mc.patched_allocations("nan", devices=["cuda"]):
            x = mc.guard_copy(torch.from_numpy(np.array(c["x"])), "nan", "x", device="cuda")
            out = metrics.torsion_neighbours(x, q, 1.4)
            torch.cuda.synchronize()
            sizes = [nbytes for _name, _raw, _off, nbytes in mc._registry]
        mc.zones_intact()
    finally:
        mc.release()
    assert len(sizes) >= 4 and max(sizes) == 8 * N * max(2 * T, (N + 63) // 64)                 # the features or the bitmap
    assert sum(sizes) < N * N                            # below one byte per pair: no N x N table of any type
    got = cr.unpack(_np(out["bits"]), N)
    want = np.array(c["tmsd"] <= 1.4 * 1.4)
    near = tr.undecided(c, 1.4 * 1.4)
    assert (got[:, :N] == want)[~near].all() and got[np.arange(N), np.arange(N)].all() and not got[:, N:].any()


@pytest.mark.parametrize("T", [1, 7, 33, 129, 2048])
def test_the_pair_route_and_its_per_torsion_rows(T):
    a, b = walk(9, T + 3, seed=11), walk(7, T + 3, seed=12)
    quads = tr.chain_quads(T)
    q = torch.from_numpy(quads)
    rng = np.random.default_rng(T)
    pairs = np.stack((rng.integers(0, 9, 12), rng.integers(0, 7, 12)), 1)
    Fa, Fb = tr.features64(a, quads)[0], tr.features64(b, quads)[0]
    tmsd, scale = tr.tmsd_cross(Fa, Fb)
    got, terms = metrics.torsion_pairs(dev(a), dev(b), torch.from_numpy(pairs), q, per_torsion=True, squared=True)
    only = metrics.torsion_pairs(dev(a), dev(b), torch.from_numpy(pairs), q, squared=True)
    assert mc.same_bits(got, only) and mc.same_bits(torch.sqrt(got), metrics.torsion_pairs(dev(a), dev(b), torch.from_numpy(pairs), q))
    want = np.array([tmsd[i, j] for i, j in pairs])
    f = float(np.max(np.abs(_np(got).astype(LD) - want) / (LD(tr.pairs_bound(T)) * want)))
    d = Fa[pairs[:, 0]].astype(LD) - Fb[pairs[:, 1]].astype(LD)
    ref = (d[:, 0::2] ** 2 + d[:, 1::2] ** 2)
    ft = float(np.max(np.abs(_np(terms).astype(LD) - ref) / (LD(tr.term_bound()) * ref)))
    print(f"T{T}: largest fraction of the bound: pairs {f:.3f}, per torsion {ft:.3f}")
    assert f <= 1.0 and ft <= 1.0 and tuple(terms.shape) == (12, T)
    same = metrics.torsion_pairs(dev(a), dev(a), torch.tensor([[0, 0], [8, 8]]), q, per_torsion=True)
    assert bool((same[0] == 0).all()) and bool((same[1] == 0).all())             # (s, s): exactly 0
    tab = metrics.torsion_matrix(dev(a), q, y=dev(b), squared=True)              # the matrix route agrees within the two bounds
    for k, (i, j) in enumerate(pairs):
        lim = LD(tr.matrix_bound(T)) * scale[i, j] + LD(tr.pairs_bound(T)) * tmsd[i, j]
        assert abs(LD(float(tab[i, j])) - LD(float(got[k]))) <= lim


@pytest.mark.parametrize("N,T", [(65, 33), (1473, 9), (2, 2048)])
def test_circular_statistics(N, T):
    c = tr.case(N, T)
    x, q = dev(c["x"]), _q(c)
    rng = np.random.default_rng(N)
    w = rng.uniform(0.5, 2.0, N)
    fin = np.ones(N, bool)
    for label, weights in (("plain", None), ("weighted", w)):
        st = metrics.circular_stats(x, q, weights=None if weights is None else dev(weights))
        mean, scale, W = tr.mean_ld(c["F"], fin, weights)
        got = np.stack([_np(st["mean_cos"]), _np(st["mean_sin"])], 1).reshape(-1)
        f = float(np.max(np.abs(got.astype(LD) - mean) / (LD(tr.mean_bound(N)) * scale)))
        print(f"N{N}-T{T} {label}: largest fraction of the mean bound: {f:.4f}")
        assert f <= 1.0 and abs(LD(st["total_weight"]) - W) <= LD(tr.mean_bound(N)) * W
        C, S = _np(st["mean_cos"]), _np(st["mean_sin"])
        assert mc.same_bits(st["resultant"], torch.sqrt(st["mean_cos"] * st["mean_cos"] + st["mean_sin"] * st["mean_sin"]))
        assert mc.same_bits(st["circular_variance"], 1.0 - st["resultant"]) and float(st["resultant"].max()) <= 1.0 + 4 * EPS
        # atan2 of the device's own sums against numpy's: both libraries document errors of a few ulp (torch's device
        # atan2 within 2 ulp, numpy's within 1), the conversion to degrees one more on each side: 5 ulp of 180 at most
        gap = float(np.abs(_np(st["mean_angle"]) - np.rad2deg(np.arctan2(S, C))).max())
        print(f"N{N}-T{T} {label}: mean_angle against numpy.arctan2: {gap:.2e} degrees")
        assert gap <= 5 * 180.0 * EPS
    plain = metrics.circular_stats(x, q)
    for p2 in (1.0, 0.25, 8.0):                          # uniform power-of-two weights: the bits of weights=None
        st = metrics.circular_stats(x, q, weights=dev(np.full(N, p2)))
        assert st["total_weight"] == p2 * N
        assert all(mc.same_bits(st[k], plain[k]) for k in ("mean_cos", "mean_sin", "resultant", "circular_variance", "mean_angle"))
    if N >= 3:                                           # a weight-0 or non-finite structure leaves the others' bits alone
        w0 = w.copy()
        w0[[1, N - 2]] = 0.0
        a = metrics.circular_stats(x, q, weights=dev(w0))
        other = c["x"].copy()
        other[1], other[N - 2] = other[0] * 3.0, np.nan
        b = metrics.circular_stats(dev(other), q, weights=dev(w0))
        bad = c["x"].copy()
        bad[1, 2, 0], bad[N - 2, 1, 1] = np.nan, np.inf
        cc = metrics.circular_stats(dev(bad), q, weights=dev(w))
        assert _np(cc["finite"]).tolist() == [i not in (1, N - 2) for i in range(N)] and _np(a["finite"]).all()
        for k in ("mean_cos", "mean_sin", "resultant", "mean_angle"):
            assert mc.same_bits(a[k], b[k]) and mc.same_bits(a[k], cc[k]), k
        assert a["total_weight"] == b["total_weight"] == cc["total_weight"]


def _check_pca(o, D, C, k, rtol=1e-10):
    d = C.shape[0]
    b = min(k + 8, d)
    th, V = _np(o["eigenvalues"]), _np(o["components"]).reshape(k, d)
    lam = np.linalg.eigvalsh(C)[::-1]
    rt = 8 * d * EPS * float(np.linalg.norm(C))
    assert o["eig_status"] == "converged" and np.isfinite(th).all() and np.isfinite(V).all() and (np.diff(th) <= 0).all()
    res = np.linalg.norm(V @ C - th[:, None] * V, axis=1)
    print(f"  eig_iter {o['eig_iter']}, max |theta - lambda| {float(np.abs(th - lam[:k]).max()):.2e}")
    assert (_np(o["residuals"]) <= rtol * th[0]).all() and (res <= rtol * th[0] + rt).all()
    assert (np.abs(th - lam[:k]) <= res + rt).all()
    gram = V @ V.T
    assert (np.abs(gram - np.eye(k)) <= (4 * d + 64 * b) * EPS).all(), float(np.abs(gram - np.eye(k)).max())
    return th, V


@pytest.mark.parametrize("N,T,weighted,k", [(65, 33, False, 6), (130, 7, True, 6), (1473, 9, True, 10), (300, 129, False, 6)])
def test_dihedral_pca_on_the_device_covariance(N, T, weighted, k):
    """Random-walk chains have no preferred torsion, so the spectrum is a noise spectrum: k + 8 >= 2 T (the iterated block is
    the whole space) or N close to 2 T (a wide spread of eigenvalues) keeps the subspace iteration short."""
    x = walk(N, T + 3, seed=3)
    quads = tr.chain_quads(T)
    w = np.random.default_rng(N).uniform(0.5, 2.0, N) if weighted else None
    xd, q = dev(x), torch.from_numpy(quads)
    o = metrics.dihedral_pca(xd, q, n_components=k, weights=None if w is None else dev(w), return_covariance=True)
    F, fin = tr.features64(x, quads)
    mean, scale, W = tr.mean_ld(F, fin, w)
    f = float(np.max(np.abs(_np(o["mean"]).reshape(-1).astype(LD) - mean) / (LD(tr.mean_bound(N)) * scale)))
    C = _np(o["cov"])
    assert tuple(C.shape) == (2 * T, 2 * T) and (C == C.T).all() and tuple(o["projections"].shape) == (N, k)
    # the covariance at the device's own deviations: D = F - mean in one rounding, restated
    D = F - _np(o["mean"]).reshape(1, -1)
    ref, Tij = tr.cov_ld(D, fin, w)
    with np.errstate(invalid="ignore", divide="ignore"):
        fc = float(np.nanmax(np.where(Tij > 0, np.abs(C.astype(LD) - ref) / (LD((N + tr.COV_BOUND_EXTRA) * EPS) * Tij), 0)))
    print(f"N{N}-T{T}: largest fraction of the bound: mean {f:.4f}, covariance {fc:.4f}")
    assert f <= 1.0 and fc <= 1.0
    total = float(o["total_variance"])
    assert abs(total - float(np.trace(C.astype(LD)))) <= 2 * T * EPS * total
    th, V = _check_pca(o, D, C, k)
    assert mc.same_bits(o["explained"], o["eigenvalues"] / o["total_variance"])
    assert mc.same_bits(o["projections"], metrics.dihedral_pca_project(xd, o))
    proj = D.astype(LD) @ V.T.astype(LD)
    lim = (2 * T + 2) * EPS * (np.abs(D) @ np.abs(V.T))
    assert (np.abs(_np(o["projections"]).astype(LD) - proj) <= lim).all()
    moved = x @ tr.rotations(1, 9)[0].T.astype(np.float32) + np.float32(3.0)     # a rigid motion changes the features in rounding only
    assert np.abs(_np(metrics.dihedral_pca_project(dev(np.ascontiguousarray(moved)), o)) - _np(o["projections"])).max() <= 1e-3


def test_dihedral_pca_of_a_rank_deficient_pool_and_of_a_planted_one():
    c = tr.case(2, 2048)
    o = metrics.dihedral_pca(dev(c["x"]), _q(c), n_components=3)                   # N = 2: rank 1
    th, V = _np(o["eigenvalues"]), _np(o["components"]).reshape(3, -1)
    assert np.isfinite(th).all() and np.isfinite(V).all() and th[0] > 0 and (np.abs(th[1:]) <= 1e-12 * th[0]).all()
    assert (np.abs(V @ V.T - np.eye(3)) <= (4 * 4096 + 64 * 11) * EPS).all() and torch.isfinite(o["projections"]).all()
    one = metrics.dihedral_pca(dev(tr.case(1, 33)["x"]), _q(tr.case(1, 33)), n_components=2)      # no variance at all
    assert bool((one["eigenvalues"].abs() <= 1e-20).all()) and torch.isfinite(one["components"]).all()
    p = tr.planted(2)
    q = metrics.dihedral_quads(p["top"])
    o = metrics.dihedral_pca(dev(p["x"]), q, n_components=2)
    side = _np(o["projections"])[:, 0] > 0
    assert (side == (p["state"] == p["state"][0])).all() or (side == (p["state"] != p["state"][0])).all()
    print(f"planted: the first component explains {float(o['explained'][0]):.3f}")
    assert float(o["explained"][0]) > 0.5 and _np(o["finite"]).all() and o["quads"].dtype == torch.int32


def test_clustering_of_a_planted_pool_whatever_the_orientation():
    p = tr.planted(3)
    q = metrics.dihedral_quads(p["top"])
    x, member = p["x"], p["state"]
    N, T = x.shape[0], q["quads"].shape[0]
    F, _ = tr.features64(x, q["quads"].numpy())
    tmsd, scale = tr.tmsd_cross(F, F)
    out = {rm: metrics.cluster_torsion(dev(x), q, 0.5, return_matrix=rm) for rm in (False, True)}
    for rm, res in out.items():
        lab = _np(res["labels"])
        assert res["n_clusters"] == 3 and sorted(_np(res["sizes"]).tolist()) == [13, 13, 14] and ("torsion" in res) == rm
        for k in range(3):
            assert len(set(member[lab == k])) == 1       # the planted membership
        ref = cr.daura(cr.unpack(_np(res["bits"]), N)[:, :N])
        assert (lab == ref["labels"]).all() and (_np(res["centres"]) == ref["centres"]).all()
        assert abs(float(res["populations"].sum()) - 1.0) <= 1e-15
    assert (_np(out[False]["labels"]) == _np(out[True]["labels"])).all()
    lab, centres = _np(out[True]["labels"]), _np(out[True]["centres"])
    for i in range(N):                                   # centre_distance by the pair route and read from the matrix
        j = centres[lab[i]]
        direct, table = LD(float(out[False]["centre_distance"][i])) ** 2, LD(float(out[True]["centre_distance"][i])) ** 2
        slack = 4 * EPS * tmsd[i, j]                     # the root and this square
        assert abs(direct - tmsd[i, j]) <= tr.pairs_bound(T) * tmsd[i, j] + slack
        assert abs(table - tmsd[i, j]) <= tr.matrix_bound(T) * scale[i, j] + slack
    w = np.random.default_rng(1).uniform(0.5, 2.0, N)
    res = metrics.cluster_torsion(dev(x), q, 0.5, weights=w)
    want = np.array([w[lab == k].sum() for k in range(3)]) / w.sum()
    assert np.abs(_np(res["populations"]) - want).max() <= 1e-14


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around one call of every entry point: the same bits under the three fills of every buffer the
    package allocates, no zone byte changed."""
    from tests.test_buffer_discipline import hold
    one = tr.case(65, 33)["x"].copy()
    one[7, 4, 2] = np.nan
    other = tr.case(3, 33)["x"].copy()
    q = torch.from_numpy(tr.chain_quads(33))
    odd = torch.from_numpy(tr.chain_quads(7))            # 2 T = 14: the last K step is half padding
    w = torch.from_numpy(np.random.default_rng(2).uniform(0.5, 2.0, 65))
    pairs = torch.tensor([[0, 1], [7, 2], [64, 0]])

    def case(g):
        out = {}
        x = g(torch.from_numpy(one), "x")
        a = metrics.cluster_torsion(x, q, 1.4, return_matrix=True)
        out.update({f"one_{k}": v for k, v in a.items() if torch.is_tensor(v)})
        b = metrics.cluster_torsion(x, odd, 1.4, weights=w)
        out.update({f"odd_{k}": v for k, v in b.items() if torch.is_tensor(v)})
        out["features"], out["finite"] = metrics.torsion_features(x, q)
        out["cross"] = metrics.torsion_matrix(x, odd, y=g(torch.from_numpy(other), "y"))
        out["pairs"], out["terms"] = metrics.torsion_pairs(x, g(torch.from_numpy(other), "b"), pairs, q, per_torsion=True)
        st = metrics.circular_stats(x, q, weights=g(w, "w"))
        out.update({f"stats_{k}": v for k, v in st.items() if torch.is_tensor(v)})
        pc = metrics.dihedral_pca(x, odd, n_components=3, weights=g(w, "w"), return_covariance=True, max_iter=40)
        out.update({f"pca_{k}": v for k, v in pc.items() if torch.is_tensor(v)})
        out["project"] = metrics.dihedral_pca_project(g(torch.from_numpy(other), "y"), pc)
        return out, []
    hold("torsion", case)
