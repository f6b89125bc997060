"""Clustering on the device (codlad_amd/csrc/cluster_kernels.hip through codlad_amd.metrics) against tests/cluster_ref.py:
the all-pairs msd against the float64 SVD route within ensemble_ref.msd_bound, its independence of everything but the
pair, the bitmap against the device's own matrix and against the reference decision, Daura's clustering against the
plain loop on the same bitmap and against answers derived by hand, non-finite input, weights, buffers and the CLI."""
import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import cluster_ref as cr
from tests import memcheck
from tests.test_saxs import _cli, dev

pytestmark = pytest.mark.gpu
_MSD = {}


def host(out):
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in out.items()}


def device_msd(kind, *key):
    """The device's msd table of a case of cluster_ref, computed once and shared."""
    if (kind, key) not in _MSD:
        x = {"planted": lambda: cr.planted(*key)[0], "continuum": cr.continuum, "degenerate": cr.degenerate,
             "pool": lambda: cr.pool(*key)}[kind]()
        m = metrics.rmsd_matrix(dev(x), squared=True).cpu().numpy()
        m.setflags(write=False)
        _MSD[(kind, key)] = m
    return _MSD[(kind, key)]


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a,
                                                                          b.view(np.int64) if b.dtype == np.float64 else b)


def check_matrix(msd, kind, *key):
    ref, bound = cr.reference(kind, *key)
    N = ref.shape[0]
    assert msd.shape == (N, N) and msd.dtype == np.float64
    assert (np.diag(msd) == 0.0).all() and same(msd, np.ascontiguousarray(msd.T))
    off = ~np.eye(N, dtype=bool)
    err = np.abs(msd - ref)
    ratio = float((err[off] / bound[off]).max()) if N > 1 and (bound[off] > 0).all() else float(err.max() > 0)
    print(f"{kind} {key}: max |msd_dev - msd_ref| / bound {ratio:.3f}")
    assert (err[off] <= bound[off]).all(), np.argwhere((err > bound) & off)[:5].tolist()


@pytest.mark.parametrize("N,n", cr.SHAPES, ids=lambda v: str(v))
def test_matrix_against_the_float64_reference(N, n):
    msd = device_msd("pool", N, n)
    check_matrix(msd, "pool", N, n)
    if (N, n) in ((65, 65), (17, 5)):                                  # the rmsd is the square root of the msd
        rmsd = metrics.rmsd_matrix(dev(cr.pool(N, n))).cpu().numpy()
        assert same(rmsd, np.sqrt(msd))


def test_matrix_of_degenerate_and_continuum_pools():
    check_matrix(device_msd("degenerate"), "degenerate")
    check_matrix(device_msd("continuum"), "continuum")
    for key in cr.PLANTED_CASES:
        check_matrix(device_msd("planted", *key), "planted", *key)


def test_an_element_depends_on_its_pair_alone():
    x = cr.pool(130, 65)
    full = device_msd("pool", 130, 65)
    perm = np.random.default_rng(5).permutation(130)
    assert same(metrics.rmsd_matrix(dev(x[perm]), squared=True).cpu().numpy(), np.ascontiguousarray(full[np.ix_(perm, perm)]))
    sub = np.array(cr.SUB_POOL)
    assert same(metrics.rmsd_matrix(dev(x[sub]), squared=True).cpu().numpy(), np.ascontiguousarray(full[np.ix_(sub, sub)]))
    assert same(metrics.rmsd_matrix(dev(x), squared=True).cpu().numpy(), full)                       # a replay
    d = cr.degenerate()
    p16 = np.random.default_rng(6).permutation(16)
    assert same(metrics.rmsd_matrix(dev(d[p16]), squared=True).cpu().numpy(), np.ascontiguousarray(device_msd("degenerate")[np.ix_(p16, p16)]))
    a = host(metrics.rmsd_neighbours(dev(x), cr.PLANTED_CUTOFF))
    b = host(metrics.rmsd_neighbours(dev(x), cr.PLANTED_CUTOFF, return_matrix=True))
    assert same(a["bits"], b["bits"]) and same(b["rmsd"], np.sqrt(full)) and "rmsd" not in a


def _cases():
    return [("planted", key, cr.PLANTED_CUTOFF) for key in cr.PLANTED_CASES] + [("continuum", (), cr.CONTINUUM_CUTOFF)]


@pytest.mark.parametrize("kind,key,cutoff", _cases(), ids=lambda v: str(v))
def test_bitmap_and_clustering(kind, key, cutoff):
    """The bitmap is msd_dev <= cut2 of the device's own matrix, and the reference decision on every pair that is not
    undecided - of which there are none (test_cluster_host.py); the clustering of that bitmap is the plain loop's."""
    x = cr.planted(*key)[0] if kind == "planted" else cr.continuum()
    N = x.shape[0]
    msd = device_msd(kind, *key)
    ref, bound = cr.reference(kind, *key)
    cut2 = float(cutoff) * float(cutoff)
    out = metrics.cluster(dev(x), cutoff)
    o = host(out)
    assert o["bits"].dtype == np.int64 and o["bits"].shape == (N, (N + 63) // 64) and o["finite"].all()
    nb = cr.unpack(o["bits"], N)
    assert not nb[:, N:].any()                                         # the padding bits
    nb = nb[:, :N]
    assert (nb == (msd <= cut2)).all() and nb.diagonal().all()
    und = cr.undecided(ref, bound, cut2)
    assert int(und.sum()) == 0 and (nb == (ref <= cut2))[~und].all()
    want = cr.daura(nb)
    assert o["labels"].dtype == np.int32 and o["labels"].tolist() == want["labels"].tolist()
    assert o["centres"].tolist() == want["centres"].tolist() and o["sizes"].tolist() == want["sizes"].tolist()
    assert o["n_clusters"] == want["n_clusters"] and same(o["populations"], o["sizes"] / o["sizes"].sum())
    print(f"{kind} {key}: {o['n_clusters']} clusters in {o['rounds']} rounds, sizes {o['sizes'][:6].tolist()}")
    if kind == "planted":
        blob = cr.planted(*key)[1]
        assert o["n_clusters"] == len(set(blob.tolist()))
        assert all(len(set(blob[o["labels"] == k].tolist())) == 1 for k in range(o["n_clusters"]))
    else:
        # the rule picks a centre that is not the first structure; the closing launch numbers the tail as the loop does
        assert o["centres"][0] != 0 and (o["sizes"] > 1).sum() >= 1 and (o["sizes"] == 1).sum() > 10
        assert o["rounds"] < o["n_clusters"]
    # centre_rmsd: the pair route is superposed_rmsd_batch of (structure, its centre); the matrix route reads the matrix
    centre_of = o["centres"][o["labels"]].astype(np.int64)
    pair = metrics.superposed_rmsd_batch(dev(x), dev(x[centre_of])).cpu().numpy()
    assert same(o["centre_rmsd"], pair)
    om = host(metrics.cluster(dev(x), cutoff, return_matrix=True))
    assert same(om["centre_rmsd"], np.ascontiguousarray(np.sqrt(msd)[np.arange(N), centre_of])) and same(om["rmsd"], np.sqrt(msd))
    assert om["labels"].tolist() == o["labels"].tolist() and (om["centre_rmsd"][o["centres"]] == 0).all()


def test_large_pool_clusters_as_the_loop():
    N, n = cr.LARGE
    out = host(metrics.cluster(dev(cr.pool(N, n)), cr.PLANTED_CUTOFF))
    nb = cr.unpack(out["bits"], N)
    assert not nb[:, N:].any() and (nb[:, :N] == (device_msd("pool", N, n) <= 1.0)).all()
    want = cr.daura(nb[:, :N])
    assert out["labels"].tolist() == want["labels"].tolist() and out["centres"].tolist() == want["centres"].tolist()
    assert out["sizes"].tolist() == want["sizes"].tolist() and int(out["sizes"].sum()) == N


@pytest.mark.parametrize("name", list(cr.HAND), ids=lambda s: s.split(":")[0])
def test_hand_written_bitmaps(name):
    N, edges, labels, centres, sizes = cr.HAND[name]
    nb = cr.from_edges(N, edges)
    for garbage in (False, True):
        o = host(metrics.cluster_neighbours(dev(cr.pack(nb, garbage)), N))
        assert o["labels"].tolist() == list(labels) and o["centres"].tolist() == list(centres) and o["sizes"].tolist() == list(sizes)
        assert o["n_clusters"] == len(centres)
    if "second batch" in name:
        assert o["rounds"] > metrics.CLUSTER_BATCH
    fin = np.ones(N, dtype=bool)
    fin[centres[0]] = False
    want = cr.daura(nb, fin)
    o = host(metrics.cluster_neighbours(dev(cr.pack(nb)), N, finite=dev(fin)))
    assert o["labels"].tolist() == want["labels"].tolist() and o["centres"].tolist() == want["centres"].tolist()
    assert o["sizes"].tolist() == want["sizes"].tolist() and o["labels"][centres[0]] == -1


def test_non_finite_structures_are_left_out():
    x = cr.planted(65, 65, 3)[0]
    sel = np.arange(0, 65, 2)
    clean = host(metrics.cluster(dev(x), cr.PLANTED_CUTOFF, sel=sel.tolist(), return_matrix=True))
    bad = x.copy()
    bad[3, 4, 1] = np.nan                                              # atoms 4 and 64 are selected
    bad[64, 64, 0] = np.inf
    bad[10, 5, 2] = np.nan                                             # atom 5 is not: this changes nothing
    o = host(metrics.cluster(dev(bad), cr.PLANTED_CUTOFF, sel=sel.tolist(), return_matrix=True))
    out = np.array([3, 64])
    keep = np.setdiff1d(np.arange(65), out)
    assert o["finite"].tolist() == [i not in (3, 64) for i in range(65)]
    assert np.isnan(o["rmsd"][out]).all() and np.isnan(o["rmsd"][:, out]).all()
    assert same(np.ascontiguousarray(o["rmsd"][np.ix_(keep, keep)]), np.ascontiguousarray(clean["rmsd"][np.ix_(keep, keep)]))
    nb = cr.unpack(o["bits"], 65)[:, :65]
    assert not nb[out].any() and not nb[:, out].any()
    assert (nb[np.ix_(keep, keep)] == cr.unpack(clean["bits"], 65)[:, :65][np.ix_(keep, keep)]).all()
    want = cr.daura(nb, o["finite"])
    assert o["labels"].tolist() == want["labels"].tolist() and (o["labels"][out] == -1).all() and (o["labels"][keep] >= 0).all()
    assert o["centres"].tolist() == want["centres"].tolist() and int(o["sizes"].sum()) == 63
    assert np.isnan(o["centre_rmsd"][out]).all() and np.isfinite(o["centre_rmsd"][keep]).all()
    only_outside = x.copy()
    only_outside[10, 5, 2] = np.nan
    o2 = host(metrics.cluster(dev(only_outside), cr.PLANTED_CUTOFF, sel=sel.tolist(), return_matrix=True))
    assert same(o2["rmsd"], clean["rmsd"]) and same(o2["bits"], clean["bits"]) and o2["labels"].tolist() == clean["labels"].tolist()


def test_weights_give_the_populations_in_index_order():
    x, _blob = cr.planted(130, 65, 5)
    w = np.random.default_rng(9).uniform(0.0, 1.0, 130)
    w[[7, 100]] = 0.0
    o = host(metrics.cluster(dev(x), cr.PLANTED_CUTOFF, weights=dev(w)))
    sums, total = np.zeros(o["n_clusters"]), 0.0
    for i in range(130):
        sums[o["labels"][i]] += w[i]
        total += w[i]
    assert same(o["populations"], sums / total) and abs(o["populations"].sum() - 1.0) < 1e-12
    plain = host(metrics.cluster_neighbours(dev(o["bits"]), 130))
    assert same(plain["populations"], plain["sizes"] / plain["sizes"].sum()) and plain["labels"].tolist() == o["labels"].tolist()


@pytest.mark.parametrize("N,n", [(1, 65), (65, 65), cr.LARGE], ids=lambda v: str(v))
def test_buffers_are_written_before_they_are_read_and_within_bounds(N, n):
    x = dev(cr.pool(N, n))
    got = {}
    for fill in memcheck.FILLS:
        with memcheck.patched_allocations(fill):
            m = metrics.rmsd_matrix(x, squared=True)
            nbm = metrics.rmsd_neighbours(x, cr.PLANTED_CUTOFF, return_matrix=True)
            cl = metrics.cluster(x, cr.PLANTED_CUTOFF)
            torch.cuda.synchronize()
        assert memcheck.zones_intact()
        memcheck.release()
        got[fill] = [m.cpu().numpy(), nbm["bits"].cpu().numpy(), nbm["rmsd"].cpu().numpy(), nbm["finite"].cpu().numpy()] + \
                    [cl[k].cpu().numpy() for k in ("labels", "centres", "sizes", "populations", "centre_rmsd", "bits")]
    for fill in memcheck.FILLS[1:]:
        assert all(same(a, b) for a, b in zip(got["zero"], got[fill])), fill
    assert same(got["zero"][0], device_msd("pool", N, n))


def test_cli_cluster_end_to_end(tmp_path):
    files, stdout = _cli(tmp_path, "--cluster", "1.0")
    labels = sorted(f for f in files if f.endswith("_cluster_labels.npy"))
    assert len(labels) == 4 and "clustering (Daura / GROMOS" in stdout and stdout.count("cluster_top5_share") == 4      # four proteins
    for f in labels:
        stem = f[:-len("_cluster_labels.npy")]
        lab, cen, siz = np.load(files[f]), np.load(files[f"{stem}_cluster_centres.npy"]), np.load(files[f"{stem}_cluster_sizes.npy"])
        xyz = np.load(files[f"{stem}_xyz_recon.npy"])
        pool = xyz.shape[0] * xyz.shape[1]
        assert lab.dtype == cen.dtype == siz.dtype == np.int32 and lab.shape == (pool,) and cen.shape == siz.shape
        assert (lab >= 0).all() and lab.max() + 1 == cen.shape[0] and int(siz.sum()) == pool
        assert (np.bincount(lab, minlength=cen.shape[0]) == siz).all() and (lab[cen] == np.arange(cen.shape[0])).all()
    import os
    import subprocess
    import sys
    res = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "test.py"),
                          "--synthetic", "--cluster", "0"], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert res.returncode != 0 and "--cluster takes an RMSD cut-off in A, a positive number" in res.stderr
