"""The ensemble-comparison kernels on the device against tests/compare_ref.py: codlad_dist_hist's counts equal the float32
restatement in every element and lie in the float64 sandwich; the bits repeat, survive a permutation and add up over a
split; codlad_column_hist equals its float64 restatement; codlad_hist_divergence holds the hand cases exactly where the
header says so and stays within the header's bounds (from cols, 2^-52 and a log2 within one unit in the last place; not
fitted) of the longdouble value - largest measured fraction of a bound on an MI355X: js 0.034, tv 0.12, w1 0.037;
ensemble_compare gives exactly 0 for a pool against itself and the planted values for planted pools."""
import numpy as np
import pytest
import torch

from codlad_amd import metrics
from tests import compare_ref as cr
from tests.test_saxs import _cli, dev

pytestmark = pytest.mark.gpu


def _hist(c, dr, n_bins, x=None):
    return metrics.distance_histogram(dev(c["x"] if x is None else x), sel=None if c["sel"] is None else c["sel"].tolist(),
                                      dr=dr, n_bins=n_bins)


def _check(out, c, n_bins):
    H = out["H"].cpu().numpy()
    assert H.dtype == np.int32 and H.shape == c["H32"].shape and out["finite"].cpu().numpy().tolist() == c["finite"].tolist()
    assert int(out["n_counted"]) == c["n_counted"] and (H.sum(1) == c["n_counted"]).all() and (H[:, 0] == 0).all()
    wrong = np.argwhere(H != c["H32"])
    assert wrong.size == 0, (len(wrong), wrong[:5].tolist())
    assert cr.sandwich(H, c["t64"], c["delta"], n_bins) == 0


@pytest.mark.parametrize("key", cr.SHAPES, ids=cr.shape_id)
def test_counts_equal_the_float32_restatement_and_lie_in_the_float64_sandwich(key):
    N, m, n_bins, dr, kind = key
    c = cr.case(key)
    out = _hist(c, dr, n_bins)
    _check(out, c, n_bins)
    assert out["pairs"].cpu().numpy().tolist() == np.stack(cr.pairs(m), 1).tolist() and out["edges"].shape == (n_bins + 1,)
    over = int(out["H"][:, -1].sum())
    print(f"{cr.shape_id(key)}: delta {c['delta']:.2e} bins, {over} of {c['H32'].sum()} counts beyond the grid, "
          f"{int((c['H32'] != c['H64']).sum())} elements where float32 and float64 decide differently")
    assert (over > 0) == (kind == "far")


@pytest.mark.parametrize("key", cr.LIMITS, ids=lambda k: f"N{k[0]}-m{k[1]}-B{k[2]}")
def test_the_declared_limits_are_held_to_the_restatement(key):
    N, m, n_bins, dr = key
    c = cr.pool(N, m, "all", seed=1)
    H32, fin, n = cr.hist32(c["x"], None, np.float32(1.0 / dr), n_bins)
    out = metrics.distance_histogram(dev(c["x"]), dr=dr, n_bins=n_bins)
    H = out["H"].cpu().numpy()
    assert H.shape == (m * (m - 1) // 2, n_bins + 2) and int(out["n_counted"]) == n == N
    assert (H == H32).all() and (H.sum(1) == N).all()


def test_lattice_distances_on_bin_edges_and_coincident_atoms():
    for dr, n_bins in ((0.5, 50), (1.0, 20), (2.0, 256)):
        H = metrics.distance_histogram(dev(cr.lattice_pool(7, 17)), dr=dr, n_bins=n_bins)["H"].cpu().numpy()
        assert (H == cr.lattice_hist(7, 17, dr, n_bins)).all(), (dr, n_bins)
    x = np.zeros((5, 3, 3), dtype=np.float32)
    x[:, 2, 0] = 1000.0                                              # atoms 0 and 1 coincide, atom 2 is beyond any grid
    H = metrics.distance_histogram(dev(x), dr=0.5, n_bins=50)["H"].cpu().numpy()
    assert H[0, 1] == 5 and H[0].sum() == 5 and H[1, -1] == 5 and H[2, -1] == 5 and H[:, :-1].sum() == 5


def test_bits_repeat_and_do_not_depend_on_order_split_or_unselected_atoms():
    key = (300, 33, 50, 0.5, "sel")
    c = cr.case(key)
    sel = c["sel"].tolist()
    runs = [_hist(c, 0.5, 50)["H"].cpu().numpy() for _ in range(3)]
    assert (runs[0] == runs[1]).all() and (runs[0] == runs[2]).all() and (runs[0] == c["H32"]).all()
    perm = np.random.default_rng(3).permutation(300)
    assert (_hist(c, 0.5, 50, x=c["x"][perm])["H"].cpu().numpy() == runs[0]).all()
    H1 = _hist(c, 0.5, 50, x=c["x"][:137])["H"].cpu().numpy()
    H2 = _hist(c, 0.5, 50, x=c["x"][137:])["H"].cpu().numpy()
    assert (H1 + H2 == runs[0]).all()
    x = c["x"].copy()
    unsel = [a for a in range(x.shape[1]) if a not in set(sel)]
    x[5, unsel[0], 1], x[17, unsel[1], 2] = np.nan, np.inf             # not selected: nothing changes
    out = _hist(c, 0.5, 50, x=x)
    assert (out["H"].cpu().numpy() == runs[0]).all() and bool(out["finite"].all()) and int(out["n_counted"]) == 300
    x[9, sel[2], 0] = np.nan                                          # selected: the structure takes no part
    out = _hist(c, 0.5, 50, x=x)
    H32, fin, n = cr.hist32(x, c["sel"], np.float32(2.0), 50)
    assert not fin[9] and n == 299 and out["finite"].cpu().numpy().tolist() == fin.tolist() and int(out["n_counted"]) == 299
    assert (out["H"].cpu().numpy() == H32).all()
    rest = np.delete(c["x"], 9, axis=0)
    assert (_hist(c, 0.5, 50, x=rest)["H"].cpu().numpy() == H32).all()


@pytest.mark.parametrize("C", (1, 7, 903))
def test_column_hist_equals_its_float64_restatement(C):
    rng = np.random.default_rng(40 + C)
    N = 157
    v = rng.uniform(-200.0, 200.0, (N, C))
    special = np.array([-180.0, 180.0, 179.99999999999997, -170.0, -190.0, 540.0, 0.0, np.nan, np.inf, -np.inf, 1e300, -1e300,
                        3e11, -3e11, np.nextafter(-180.0, -np.inf), -0.0])
    v[:special.size, 0] = special
    v[rng.random((N, C)) < 0.05] = np.nan
    for lo, hi, n_bins, periodic in ((-180.0, 180.0, 36, True), (-180.0, 180.0, 36, False), (-150.0, 170.0, 256, False),
                                     (0.0, 7.0, 1, True), (-200.0, 200.0, 255, False)):
        out = metrics.column_histogram(dev(v), lo, hi, n_bins, periodic=periodic)
        H, n_valid = cr.column_hist_ref(v, lo, n_bins / (hi - lo), n_bins, periodic)
        got = out["H"].cpu().numpy()
        assert got.shape == (C, n_bins + 2) and (got == H).all(), (lo, hi, n_bins, periodic, np.argwhere(got != H)[:5].tolist())
        assert (out["n_valid"].cpu().numpy() == n_valid).all() and (got.sum(1) == n_valid).all()
        if periodic:
            assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all()
    one = metrics.column_histogram(dev(v[:, 0]), -180.0, 180.0, 36, periodic=True)           # a vector is one column
    assert (one["H"].cpu().numpy() == cr.column_hist_ref(v[:, :1], -180.0, 0.1, 36, True)[0]).all()


def _div(A, B):
    out = metrics.histogram_divergence(dev(np.asarray(A, dtype=np.int32)), dev(np.asarray(B, dtype=np.int32)))
    return tuple(out[k].cpu().numpy() for k in ("js", "tv", "w1"))


def test_divergence_hand_cases_symmetry_and_empty_rows():
    js, tv, w1 = _div([[1, 0]], [[0, 1]])
    assert js[0] == 1.0 and tv[0] == 1.0 and w1[0] == 1.0
    js, tv, w1 = _div([[7, 7]], [[0, 5]])
    assert abs(js[0] - cr.HAND_JS) <= cr.bounds(2)[0] and tv[0] == 0.5 and w1[0] == 0.5
    js, tv, w1 = _div([[3, 1, 0, 6], [1, 1, 1, 1]], [[21, 7, 0, 42], [5, 5, 5, 5]])
    assert (js == 0.0).all() and (tv == 0.0).all() and (w1 == 0.0).all()                  # exactly, with different totals
    a, b = np.zeros((3, 70), dtype=np.int32), np.zeros((3, 70), dtype=np.int32)
    for r, k in enumerate((1, 3, 66)):                                                   # point masses k columns apart
        a[r, 2], b[r, 2 + k] = 9, 4
    js, tv, w1 = _div(a, b)
    assert w1.tolist() == [1.0, 3.0, 66.0] and (js == 1.0).all() and (tv == 1.0).all()
    js, tv, w1 = _div([[0, 0], [1, -1], [2, 2], [1, 3]], [[1, 1], [1, 1], [0, 0], [1, 3]])
    assert np.isnan(js[:3]).all() and np.isnan(tv[:3]).all() and np.isnan(w1[:3]).all() and js[3] == 0.0
    A, B = cr.count_tables(130, 258, 5, sparse=True)
    for x, y in zip(_div(A, B), _div(B, A)):
        assert (x.view(np.int64) == y.view(np.int64)).all()


@pytest.mark.parametrize("shape", cr.DIVERGENCE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}{'-sparse' if s[2] else ''}")
def test_divergences_within_the_derived_bounds_of_longdouble(shape):
    rows, cols, sparse = shape
    A, B = cr.count_tables(rows, cols, 100 + rows + cols, sparse)
    got = _div(A, B)
    want = cr.divergence_ld(A, B)
    frac = [float(np.abs(g.astype(np.longdouble) - w).max() / b) for g, w, b in zip(got, want, cr.bounds(cols))]
    print(f"{rows} x {cols}{' sparse' if sparse else ''}: |device - longdouble| / bound  js {frac[0]:.4f}  tv {frac[1]:.4f}  "
          f"w1 {frac[2]:.5f}")
    assert all(np.isfinite(g).all() for g in got) and max(frac) <= 1.0, frac
    assert (got[0] >= 0).all() and (got[0] <= 1.0 + cr.bounds(cols)[0]).all()


def _protein_pool(N, seed):
    from codlad_amd.utils.cg_input import template_topology
    top = template_topology(["ALA", "TRP", "GLY", "SEP", "LYS", "ILE", "PRO"])
    rng = np.random.default_rng(seed)
    base = rng.uniform(-6, 6, (1, top.n_atoms, 3))
    return top, (base + rng.normal(0, 1.5, (N, top.n_atoms, 3))).astype(np.float32)


def test_a_pool_against_itself_and_against_its_duplicate_scores_exactly_zero():
    top, x = _protein_pool(40, 21)
    sel = list(range(0, top.n_atoms, 3))
    a = dev(x)
    for b in (a, torch.cat((a, a))[torch.randperm(80, generator=torch.Generator().manual_seed(1)).to(a.device)]):
        out = metrics.ensemble_compare(a, b, top=top, sel=sel, n_bins=50, cluster_cutoff=4.0)
        m = len(sel)
        assert out["js_dist"].shape == (m, m) and bool((out["js_dist"] == 0).all()) and bool((out["w1_dist"] == 0).all())
        assert float(out["js_dist_mean"]) == 0.0 and float(out["js_dist_median"]) == 0.0
        assert float(out["js_rg"]) == 0.0 and float(out["w1_rg"]) == 0.0 and int(out["overflow"]) == 0
        jt = out["js_torsion"].cpu().numpy()
        assert jt.shape == (top.n_residues, 7) and (jt[~np.isnan(jt)] == 0.0).all() and (~np.isnan(jt)).sum() >= top.n_residues
        assert np.isnan(jt[2, 3:]).all()                              # GLY has no chi
        assert (out["js_torsion_mean"].cpu().numpy()[:4] == 0.0).all()
        assert float(out["js_cluster"]) == 0.0 and out["n_clusters"] >= 1 and out["n_a"] == 40 and out["n_b"] == b.shape[0]


def test_planted_two_state_pools_give_the_hand_value():
    a, b = cr.hinge_pools()
    m = a.shape[1]
    out = metrics.ensemble_compare(dev(a), dev(b), n_bins=50)
    js = out["js_dist"].cpu().numpy()
    assert int(out["overflow"]) == 0 and out["r_max"] == 19.0        # the box is 15.2 x 9 A: diagonal 17.7, plus 1, rounded up
    assert abs(js[0, m - 1] - cr.HAND_JS) <= cr.bounds(52)[0] and js[0, m - 1] == js[m - 1, 0]
    assert abs(cr.HAND_JS - 0.311278) < 1e-6
    assert (js[:m - 1, :m - 1] == 0.0).all()                          # pairs the states do not move
    assert (np.diag(js) == 0.0).all() and (js >= 0).all() and (js <= 1.0 + cr.bounds(52)[0]).all()
    w1 = out["w1_dist"].cpu().numpy()
    assert abs(w1[0, m - 1] - 0.5 * (23 - 13) * (19.0 / 50)) < 1e-12   # half the mass moves from bin 13 (5 A) to bin 23 (9 A)
    assert float(out["js_rg"]) > 0.0
    # disjoint states: every cluster belongs to one pool alone
    rng = np.random.default_rng(8)
    base = rng.uniform(-5, 5, (12, 3))
    other = base.copy()
    other[:4] += 6.0
    pa = (base[None] + rng.normal(0, 0.01, (30, 12, 3))).astype(np.float32)
    pb = (other[None] + rng.normal(0, 0.01, (20, 12, 3))).astype(np.float32)
    out = metrics.ensemble_compare(dev(pa), dev(pb), n_bins=20, cluster_cutoff=1.0)
    assert float(out["js_cluster"]) == 1.0 and out["n_clusters"] == 2
    with pytest.raises(ValueError, match="no finite structure"):
        metrics.ensemble_compare(dev(pa), dev(np.full((3, 12, 3), np.nan, dtype=np.float32)))
    with pytest.raises(ValueError, match="no finite structure"):
        metrics.distance_histogram(dev(np.full((3, 12, 3), np.inf, dtype=np.float32)))


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around the three entry points: the same bits under the three fills of every buffer the package
    allocates, every element of every output written, no zone byte changed.  One bin and 256 of them are among the calls."""
    from tests.test_buffer_discipline import hold
    c = cr.pool(65, 17, "mixed")
    x = c["x"].copy()
    x[3, c["sel"][1], 2] = np.nan
    rng = np.random.default_rng(6)
    v = rng.uniform(-200, 200, (65, 7))
    v[4, 2] = np.nan
    A, B = cr.count_tables(9, 52, 7, sparse=True)
    A[3] = 0                                                         # a NaN row is a written row too

    def case(g):
        out = {}
        for n_bins, dr in ((1, 40.0), (50, 0.5), (256, 0.125)):
            h = metrics.distance_histogram(g(torch.from_numpy(x), "x"), sel=c["sel"].tolist(), dr=dr, n_bins=n_bins)
            out.update({f"B{n_bins}_{k}": h[k] for k in ("H", "finite", "n_counted")})
            for periodic in (False, True):
                ch = metrics.column_histogram(g(torch.from_numpy(v), "values"), -180.0, 180.0, n_bins, periodic=periodic)
                out.update({f"B{n_bins}_p{int(periodic)}_{k}": t for k, t in ch.items()})
        d = metrics.histogram_divergence(g(torch.from_numpy(A), "HA"), g(torch.from_numpy(B), "HB"))
        out.update({f"div_{k}": t for k, t in d.items()})
        return out, []
    hold("compare", case)


def test_cli_compare_end_to_end(tmp_path):
    for d in ("latent", "recon"):
        (tmp_path / d).mkdir()
    files, stdout = _cli(tmp_path / "latent", "--compare", "20")
    js = sorted(f for f in files if f.endswith("_compare_js_dist.npy"))
    assert len(js) == 4 and "generated against true ensemble" in stdout and stdout.count("compare_js_dist_mean") == 4
    assert stdout.count("distance JS mean") == 4 and stdout.count("Rg JS") == 4
    for f in js:
        M = np.load(files[f])
        assert M.ndim == 2 and M.shape[0] == M.shape[1] >= 2 and M.dtype == np.float64
        assert (np.diag(M) == 0).all() and (M >= 0).all() and (M <= 1.0 + cr.bounds(22)[0]).all() and (M == M.T).all()
    for f in (f for f in files if f.endswith("_compare_js_torsion.npy")):
        T = np.load(files[f])
        assert T.ndim == 2 and T.shape[1] == 7 and ((T[~np.isnan(T)] >= 0) & (T[~np.isnan(T)] <= 1.0 + 1e-12)).all()
    files, stdout = _cli(tmp_path / "recon", "--experiment", "recon", "--compare")
    js = sorted(f for f in files if f.endswith("_compare_js_dist.npy"))
    assert len(js) == 4 and stdout.count("distance JS mean") == 4
    for f in js:
        M = np.load(files[f])
        assert np.isfinite(M).all() and (M >= 0).all() and (M <= 1.0 + cr.bounds(52)[0]).all()
    print("\n".join(line for line in stdout.splitlines() if line.startswith("compare ")))
