"""The chain-statistics kernels on the device against tests/polymer_ref.py: every element of sep_r2, sep_inv and inv_sum
within the header's bound of the longdouble reference (the bounds come from the operation counts of the header; none is
fitted), the gyration tensor within its bound and its eigenvalues within the bound of eigvalsh of the device's own tensor,
the rod and the cube by hand, the same bits from call to call, for a structure alone or inside a batch, and on both sides
of the split threshold, defined results for non-finite input and coincident atoms, weighted ensemble values, and
tests/memcheck.py around the launches.  Largest measured fraction of a bound on an MI355X (printed by every accuracy
test): sep_r2 0.11, sep_inv 0.10, inv_sum 0.07, tensor 0.07, eig 0.47, ree 0.14, weighted r_rms and 1 / rh_mean 0.003."""
import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import memcheck as mc
from tests import polymer_ref as pr
from tests.test_saxs import dev

pytestmark = pytest.mark.gpu
LD = pr.LD


def _sel(c):
    return None if c["sel"] is None else c["sel"].tolist()


def _np(t):
    return t.detach().cpu().numpy()


def _check_sums(out, c, label):
    """Every element against the longdouble reference -> the largest fractions of the three bounds."""
    m = c["m"]
    assert out["sep_r2"].dtype == torch.float64 and tuple(out["sep_r2"].shape) == tuple(out["sep_inv"].shape) == (c["N"], m - 1)
    assert tuple(out["inv_sum"].shape) == (c["N"],) and out["finite"].dtype == torch.bool and _np(out["finite"]).all()
    f2 = pr.worst(_np(out["sep_r2"]), c["sep_r2"], pr.sum_bound(m))
    fi = pr.worst(_np(out["sep_inv"]), c["sep_inv"], pr.sum_bound(m))
    fs = pr.worst(_np(out["inv_sum"]), c["inv_sum"], pr.inv_sum_bound(m))
    print(f"{label}: largest fraction of the bound: sep_r2 {f2:.3f}, sep_inv {fi:.3f}, inv_sum {fs:.3f}")
    assert f2 <= 1.0 and fi <= 1.0 and fs <= 1.0, (label, f2, fi, fs)


def _check_gyration(g, c, label):
    m = c["m"]
    T, e, ree = _np(g["tensor"]), _np(g["eig"]), _np(g["ree"])
    assert T.shape == (c["N"], 6) and e.shape == (c["N"], 3) and _np(g["finite"]).all()
    trace = c["tensor"][:, :3].sum(1)
    ft = float(np.max(np.abs(T.astype(LD) - c["tensor"]) / (LD(pr.tensor_bound(m)) * trace[:, None])))
    own = pr.eigvalsh6(T)                                # of the device's own tensor
    fe = float(np.max(np.abs(e - np.maximum(own, 0.0)) / (pr.eig_bound(m) * T[:, :3].sum(1)[:, None])))
    fr = pr.worst(ree, c["ree"], pr.TERM_OPS * pr.EPS)   # the per-pair sequence and one square root
    print(f"{label}: largest fraction of the bound: tensor {ft:.3f}, eig {fe:.3f}, ree {fr:.3f}")
    assert ft <= 1.0 and fe <= 1.0 and fr <= 1.0, (label, ft, fe, fr)
    assert (e[:, 0] <= e[:, 1]).all() and (e[:, 1] <= e[:, 2]).all() and (e >= 0).all()
    return T, e


@pytest.mark.parametrize("m", pr.SHAPE_M)
@pytest.mark.parametrize("N", pr.SHAPE_N)
def test_every_sum_lies_within_the_header_bound_of_longdouble(N, m):
    c = pr.case(N, m)
    x = dev(c["x"])
    out = metrics.chain_sums(x)
    _check_sums(out, c, f"N{N}-m{m}")
    g = metrics.gyration_tensor(x)
    T, e = _check_gyration(g, c, f"N{N}-m{m}")
    # rg2 three ways: the eigenvalues' sum, radius_of_gyration squared (codlad_ens_moments: a 256-lane deal, fewer additions
    # than SUM_BOUND counts, a division, a root and this square: 3 roundings more), and Lagrange's sum of sep_r2 / m^2
    trace = c["tensor"][:, :3].sum(1)
    rg2 = _np(g["rg2"]).astype(LD)
    own = (3 * pr.eig_bound(m) + 3 * pr.tensor_bound(m) + 2 * pr.EPS) * trace
    rog = _np(metrics.radius_of_gyration(x)).astype(LD) ** 2
    lagrange = _np(out["sep_r2"]).astype(LD).sum(1) / LD(m * m)
    assert (np.abs(rg2 - rog) <= own + (pr.sum_bound(m) + 3 * pr.EPS) * trace).all()
    assert (np.abs(rg2 - lagrange) <= own + pr.sum_bound(m) * trace).all()
    # the shape numbers are float64 torch from eig: the same formulas in numpy from the device's eig
    for name, want in zip(("asphericity", "acylindricity", "kappa2", "prolateness"), pr.shape_numbers(e)):
        assert np.abs(_np(g[name]) - want).max() <= 8 * pr.EPS * max(1.0, float(np.abs(want).max())), name
    k2, pl = _np(g["kappa2"]), _np(g["prolateness"])
    assert ((k2 >= -8 * pr.EPS) & (k2 <= 1 + 8 * pr.EPS)).all() and ((pl >= -0.25 - 8 * pr.EPS) & (pl <= 2 + 8 * pr.EPS)).all()


@pytest.mark.parametrize("N,m,kind", [(3, 65, "subset"), (3, 129, "descending")])
def test_a_subset_and_a_descending_selection(N, m, kind):
    c = pr.case(N, m, kind)
    x = dev(c["x"])
    out = metrics.chain_sums(x, sel=_sel(c))
    _check_sums(out, c, f"{kind}-N{N}-m{m}")
    _check_gyration(metrics.gyration_tensor(x, sel=_sel(c)), c, f"{kind}-N{N}-m{m}")
    if kind == "descending":                             # the reversed chain's sums are the chain's, each within its bound
        fwd = metrics.chain_sums(x)
        for k, b in (("sep_r2", pr.sum_bound(m)), ("sep_inv", pr.sum_bound(m)), ("inv_sum", pr.inv_sum_bound(m))):
            assert pr.worst(_np(out[k]), _np(fwd[k]), 2 * b) <= 1.0, k


@pytest.mark.parametrize("m", [pr.SPLIT_MIN_SEL - 1, pr.SPLIT_MIN_SEL])
def test_both_sides_of_the_split_threshold_at_one_structure(m):
    groups = _lib.lib().codlad_chain_sums_groups(1, m)
    assert (groups > 1) == (m >= pr.SPLIT_MIN_SEL)
    c = pr.case(1, m)
    _check_sums(metrics.chain_sums(dev(c["x"])), c, f"N1-m{m}-groups{groups}")
    _check_gyration(metrics.gyration_tensor(dev(c["x"])), c, f"N1-m{m}")


def test_the_selection_limit_and_one_more():
    m = pr.MAX_SEL
    c = pr.case(1, m)
    _check_sums(metrics.chain_sums(dev(c["x"])), c, f"N1-m{m}")
    _check_gyration(metrics.gyration_tensor(dev(c["x"])), c, f"N1-m{m}")
    big = torch.zeros(1, m + 1, 3, device="cuda")
    for call in (metrics.chain_sums, metrics.gyration_tensor, metrics.hydrodynamic_radius, metrics.distance_scaling):
        with pytest.raises(ValueError, match=f"{m} selected atoms, got {m + 1}"):
            call(big)
    assert metrics.chain_sums(big, sel=list(range(m)))["sep_r2"].shape == (1, m - 1)      # a selection within the limit runs


def test_rod_and_cube_by_hand():
    for m in (2, 17, 64, 600):                           # 600: the split path
        x = dev(pr.rod(m))
        out = metrics.chain_sums(x)
        want2, wanti = pr.rod_sums(m)
        assert (_np(out["sep_r2"])[0] == want2).all()    # integers: exact in any order
        assert pr.worst(_np(out["sep_inv"])[0], (LD(m) - np.arange(1, m)) / (LD(4) * np.arange(1, m)), pr.sum_bound(m)) <= 1.0
        g = metrics.gyration_tensor(x)
        lam = LD(16 * (m * m - 1)) / LD(12)
        e = _np(g["eig"])[0]
        assert e[0] == 0.0 and e[1] == 0.0 and abs(e[2] - lam) <= pr.eig_bound(m) * lam and float(g["ree"][0]) == 4.0 * (m - 1)
        assert float(g["kappa2"][0]) == 1.0 and abs(float(g["prolateness"][0]) - 2.0) <= 4 * pr.EPS
        assert float(g["acylindricity"][0]) == 0.0 and float(g["asphericity"][0]) == e[2] and float(g["rg2"][0]) == e[2]
        rh = metrics.hydrodynamic_radius(x)
        want = LD(m * m) / (2 * ((LD(m) - np.arange(1, m)) / (LD(4) * np.arange(1, m))).sum())
        assert abs(float(rh["rh"][0]) - want) <= (pr.inv_sum_bound(m) + 3 * pr.EPS) * want and float(rh["rh_mean"]) == float(rh["rh"][0])
        sc = metrics.distance_scaling(x)
        assert _np(sc["sep"]).tolist() == list(range(1, m)) and (_np(sc["r_rms"]) == 4.0 * np.arange(1, m)).all() and sc["n_struct"] == 1
        if m >= 17:
            fit = metrics.flory_fit(sc["sep"], sc["r_rms"], s_min=2)
            assert abs(fit["nu"] - 1.0) <= 1e-12 and abs(fit["r0"] - 4.0) <= 1e-12
    g = metrics.gyration_tensor(dev(pr.cube()))
    assert _np(g["eig"])[0].tolist() == [0.25, 0.25, 0.25] and float(g["kappa2"][0]) == 0.0 and float(g["prolateness"][0]) == 0.0
    assert float(g["asphericity"][0]) == 0.0 and abs(float(g["ree"][0]) - np.sqrt(3.0)) <= pr.TERM_OPS * pr.EPS * 2
    # every atom in one place: rg2 is 0 and the shape numbers are not numbers; 1 / r is +inf throughout and Rh is 0
    one = dev(np.ones((1, 5, 3), dtype=np.float32))
    g = metrics.gyration_tensor(one)
    assert float(g["rg2"][0]) == 0.0 and bool(g["finite"][0]) and float(g["ree"][0]) == 0.0
    assert all(np.isnan(float(g[k][0])) for k in ("asphericity", "acylindricity", "kappa2", "prolateness"))
    assert float(metrics.hydrodynamic_radius(one)["rh"][0]) == 0.0


def _bits(out, keys=("sep_r2", "sep_inv", "inv_sum")):
    return {k: out[k].detach().cpu().clone() for k in keys}


def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    return all(mc.same_bits(a[k][rows_a].contiguous(), b[k][rows_b].contiguous()) for k in a)


GYR_KEYS = ("tensor", "eig", "ree", "rg2", "kappa2")


def test_the_bits_repeat_and_do_not_depend_on_the_batch():
    c = pr.case(70, 129)
    x = dev(c["x"])
    a, b = _bits(metrics.chain_sums(x)), _bits(metrics.chain_sums(x))
    assert _same(a, b)
    ga, gb = _bits(metrics.gyration_tensor(x), GYR_KEYS), _bits(metrics.gyration_tensor(x), GYR_KEYS)
    assert _same(ga, gb)
    for s in (0, 17, 69):                                # alone, and in another place of another batch
        alone = _bits(metrics.chain_sums(x[s:s + 1]))
        assert _same(alone, a, slice(0, 1), slice(s, s + 1))
        galone = _bits(metrics.gyration_tensor(x[s:s + 1]), GYR_KEYS)
        assert _same(galone, ga, slice(0, 1), slice(s, s + 1))
    perm = torch.arange(69, -1, -1, device=x.device)
    moved = _bits(metrics.chain_sums(x[perm].contiguous()))
    assert _same(moved, a, slice(None), perm.cpu())
    gmoved = _bits(metrics.gyration_tensor(x[perm].contiguous()), GYR_KEYS)
    assert _same(gmoved, ga, slice(None), perm.cpu())


def test_the_split_changes_no_bit():
    """One structure of SPLIT_MIN_SEL atoms is split across workgroups; SPLIT_MAX_N copies of it are not."""
    m, n = pr.SPLIT_MIN_SEL + 45, pr.SPLIT_MAX_N         # 557: an odd count, and no multiple of 64
    groups = _lib.lib().codlad_chain_sums_groups
    assert groups(1, m) > groups(32, m) > groups(n - 1, m) > 1 and groups(n, m) == 1      # 70, 32, 5 and 1 workgroups a structure
    x = dev(pr.case(1, m)["x"])
    split = _bits(metrics.chain_sums(x))
    for copies in (32, n - 1, n):
        many = _bits(metrics.chain_sums(x.expand(copies, m, 3).contiguous()))
        for s in (0, 17, copies - 1):
            assert _same(split, many, slice(0, 1), slice(s, s + 1)), (copies, s)
    m = pr.SPLIT_MIN_SEL                                 # an even count: the middle separation stands alone
    x = dev(pr.case(1, m)["x"])
    assert _same(_bits(metrics.chain_sums(x)), _bits(metrics.chain_sums(x.expand(n, m, 3).contiguous())), slice(0, 1), slice(5, 6))


@pytest.mark.parametrize("m", [65, 2 * pr.SPLIT_MIN_SEL + 1])
def test_non_finite_input_and_coincident_atoms_have_defined_results(m):
    """33 selected atoms (a workgroup per structure) and SPLIT_MIN_SEL + 1 of them (the split path)."""
    x3 = pr.walk(3, m)
    x0 = np.concatenate([x3, x3[:2]], 0)                 # five structures
    sel = list(range(0, m, 2))                           # every other atom, both ends (m is odd)
    ms = len(sel)
    assert (_lib.lib().codlad_chain_sums_groups(5, ms) > 1) == (m > 65)
    clean = metrics.chain_sums(dev(x0), sel=sel)
    gclean = metrics.gyration_tensor(dev(x0), sel=sel)
    for bad in (np.nan, np.inf, -np.inf):
        x = x0.copy()
        x[1, sel[3], 1] = bad
        x[3, sel[-1], 0] = bad
        x[2, 1, 2] = bad                                 # an unselected atom: changes nothing
        out, g = metrics.chain_sums(dev(x), sel=sel), metrics.gyration_tensor(dev(x), sel=sel)
        assert _np(out["finite"]).tolist() == [True, False, True, False, True] == _np(g["finite"]).tolist()
        for k in ("sep_r2", "sep_inv", "inv_sum"):
            assert torch.isnan(out[k][[1, 3]]).all(), k
            assert mc.same_bits(out[k][[0, 2, 4]].contiguous(), clean[k][[0, 2, 4]].contiguous()), k
        for k in ("tensor", "eig", "ree", "rg2", "asphericity", "acylindricity", "kappa2", "prolateness"):
            assert torch.isnan(g[k][[1, 3]]).all(), k
            assert mc.same_bits(g[k][[0, 2, 4]].contiguous(), gclean[k][[0, 2, 4]].contiguous()), k
        rh = metrics.hydrodynamic_radius(dev(x), sel=sel)
        assert torch.isnan(rh["rh"][[1, 3]]).all() and _np(rh["finite"]).tolist() == [True, False, True, False, True]
        ref = metrics.hydrodynamic_radius(dev(x0[[0, 2, 4]]), sel=sel)
        assert mc.same_bits(rh["rh"][[0, 2, 4]].contiguous(), ref["rh"])
        assert abs(float(rh["rh_mean"]) - float(ref["rh_mean"])) <= 8 * pr.EPS * float(ref["rh_mean"])     # three terms, any order
    # two coincident selected atoms, three chain positions apart: +inf in that one separation, Rh = 0, still finite
    x = x0.copy()
    x[2, sel[10]] = x[2, sel[7]]
    out = metrics.chain_sums(dev(x), sel=sel)
    inf = torch.isinf(out["sep_inv"])
    assert inf.sum() == 1 and bool(inf[2, 2]) and float(out["sep_inv"][2, 2]) == float("inf") and float(out["inv_sum"][2]) == float("inf")
    assert _np(out["finite"]).all() and torch.isfinite(out["sep_r2"]).all() and tuple(out["sep_r2"].shape) == (5, ms - 1)
    assert mc.same_bits(out["sep_inv"][[0, 1, 3, 4]].contiguous(), clean["sep_inv"][[0, 1, 3, 4]].contiguous())
    rh = metrics.hydrodynamic_radius(dev(x), sel=sel)
    assert float(rh["rh"][2]) == 0.0 and bool(rh["finite"][2]) and float(rh["rh_mean"]) == 0.0


def test_weighted_ensemble_values():
    N, m = 70, 129
    c = pr.case(N, m)
    rng = np.random.default_rng(3)
    w = rng.uniform(0.1, 2.0, N)
    w[[4, 9]] = 0.0
    for weights in (None, w):
        r_rms, inv_rh, n = pr.scaling_ld(c["x"], None, weights)
        sc = metrics.distance_scaling(dev(c["x"]), weights=weights)
        rh = metrics.hydrodynamic_radius(dev(c["x"]), weights=weights)
        fr = pr.worst(_np(sc["r_rms"]), r_rms, pr.ensemble_bound(m, N))
        fh = pr.worst(1.0 / _np(rh["rh_mean"]).astype(LD), inv_rh, pr.ensemble_bound(m, N))
        print(f"weights {'given' if weights is not None else 'none'}: largest fraction of the bound: r_rms {fr:.3f}, 1 / rh_mean {fh:.3f}")
        assert fr <= 1.0 and fh <= 1.0 and sc["n_struct"] == n == (N if weights is None else N - 2)
        assert pr.worst(_np(rh["inv_rh"]), 2 * c["inv_sum"] / LD(m * m), pr.inv_sum_bound(m) + pr.EPS) <= 1.0
        assert pr.worst(_np(rh["rh"]), LD(m * m) / (2 * c["inv_sum"]), pr.inv_sum_bound(m) + 2 * pr.EPS) <= 1.0
    # a random walk of 129 steps is an ideal chain: the exponent is near 1/2 (70 chains: a loose statement)
    fit = metrics.flory_fit(sc["sep"], sc["r_rms"])
    assert 0.4 < fit["nu"] < 0.6 and fit["n_points"] == m // 2 - 5 + 1
    # a structure of weight 0 that holds a NaN leaves the result as it is
    x = c["x"].copy()
    x[4, 7, 0] = np.nan
    sc2, rh2 = metrics.distance_scaling(dev(x), weights=w), metrics.hydrodynamic_radius(dev(x), weights=w)
    assert mc.same_bits(sc2["r_rms"], sc["r_rms"]) and mc.same_bits(rh2["rh_mean"], rh["rh_mean"]) and sc2["n_struct"] == N - 2
    # ... and without weights it is left out, as the reference leaves it out
    r_rms, inv_rh, n = pr.scaling_ld(x)
    sc3, rh3 = metrics.distance_scaling(dev(x)), metrics.hydrodynamic_radius(dev(x))
    assert sc3["n_struct"] == n == N - 1 and pr.worst(_np(sc3["r_rms"]), r_rms, pr.ensemble_bound(m, N)) <= 1.0
    assert pr.worst(1.0 / _np(rh3["rh_mean"]).astype(LD), inv_rh, pr.ensemble_bound(m, N)) <= 1.0
    with pytest.raises(ValueError, match="no finite structure of positive weight"):
        metrics.distance_scaling(dev(np.full((3, 5, 3), np.nan, dtype=np.float32)))


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around chain_sums on both sides of the split threshold and around gyration_tensor: the same bits
    under the three fills of every buffer the package allocates, every element of every output written (a structure
    that is not finite among them), no zone byte changed."""
    from tests.test_buffer_discipline import hold
    pools = {}
    for m in (65, pr.SPLIT_MIN_SEL + 1):
        x = pr.case(3, m)["x"].copy()
        x[1, 4, 2] = np.nan
        pools[m] = x
    sel = list(range(1, 60, 2))

    def case(g):
        out = {}
        for m, x in pools.items():
            for tag, s in (("all", None), ("sel", sel)):
                cs = metrics.chain_sums(g(torch.from_numpy(x), "x"), sel=s)
                gy = metrics.gyration_tensor(g(torch.from_numpy(x), "x"), sel=s)
                out.update({f"m{m}_{tag}_{k}": t for k, t in cs.items()})
                out.update({f"m{m}_{tag}_gyr_{k}": t for k, t in gy.items()})
        return out, []
    hold("polymer", case)
