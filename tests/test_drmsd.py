"""The dRMSD kernels on the device against tests/drmsd_ref.py: every element of the matrix within the header's bound of the
longdouble DIRECT sum over the float32 distances (the bound comes from the operation count of the header; it is not
fitted), rods by hand to the bit, exactly 0 for a duplicate, a mirror image and an fp32-exact translate, symmetry, repeats,
permutations and the split to the bit, the bitmap on EVERY pair of cases whose cut-off the CPU suite has shown to leave no
pair undecided, defined results for non-finite input, the pair route and its per-position rows, the clustering, and
tests/memcheck.py around the launches.  Largest measured fraction of a bound on an MI355X (printed by every accuracy
test): matrix 0.10 (at P = 1; 0.06 from P = 3, 0.00001 at 9.35 M pairs), pair route 0.035, per-position rows 0.14."""
import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import cluster_ref as cr
from tests import drmsd_ref as dr
from tests import memcheck as mc
from tests.polymer_ref import walk
from tests.test_saxs import dev

pytestmark = pytest.mark.gpu
LD = dr.LD

POOL_SIZES = (1, 2, 63, 64, 65, 130)
SEL_SIZES = (2, 3, 5, 17, 33, 87, 129)
ACCURACY_CASES = tuple(dict.fromkeys(
    [(N, 87, 1) for N in POOL_SIZES] +
    [(65, m, s) for m in SEL_SIZES for s in (1, 2, 3, m - 1) if 1 <= s < m] +
    [(2, 129, 1), (2, 129, 3), (130, 129, 1)]))


def _np(t):
    return t.detach().cpu().numpy()


def _sel(c):
    return None if c["sel"] is None else c["sel"].tolist()


def _check_matrix(got, c, label, msd=None, scale=None):
    """Every element of the msd table against the longdouble reference -> the largest fraction of the bound."""
    msd, scale = (c["msd"], c["scale"]) if msd is None else (msd, scale)
    assert got.dtype == torch.float64 and tuple(got.shape) == msd.shape
    f = dr.worst(_np(got), msd, scale, dr.matrix_bound(c["P"]))
    print(f"{label}: largest fraction of the matrix bound: {f:.4f}")
    assert f <= 1.0, (label, f)
    assert bool((torch.isnan(got).cpu() == torch.from_numpy(np.isnan(msd.astype(np.float64)))).all())
    return f


@pytest.mark.parametrize("N,m,min_sep", ACCURACY_CASES)
def test_every_element_lies_within_the_header_bound_of_the_direct_sum(N, m, min_sep):
    c = dr.case(N, m, min_sep)
    x = dev(c["x"])
    sq = metrics.drmsd_matrix(x, min_sep=min_sep, squared=True)
    _check_matrix(sq, c, f"N{N}-m{m}-sep{min_sep}")
    assert mc.same_bits(sq, sq.T.contiguous()) and bool((sq.diagonal() == 0).all())
    root = metrics.drmsd_matrix(x, min_sep=min_sep)
    assert mc.same_bits(root, torch.sqrt(sq))
    assert mc.same_bits(sq, metrics.drmsd_matrix(x, min_sep=min_sep, squared=True))          # a repeat


@pytest.mark.parametrize("N,m,min_sep,kind", [(65, 33, 2, "subset"), (3, 129, 1, "descending"), (64, 17, 3, "subset")])
def test_a_subset_and_a_descending_selection(N, m, min_sep, kind):
    c = dr.case(N, m, min_sep, kind)
    x = dev(c["x"])
    sq = metrics.drmsd_matrix(x, sel=_sel(c), min_sep=min_sep, squared=True)
    _check_matrix(sq, c, f"{kind}-N{N}-m{m}-sep{min_sep}")
    if kind == "descending":                             # the reversed chain has the same pairs in another order
        fwd = metrics.drmsd_matrix(x, min_sep=min_sep, squared=True)
        assert dr.worst(_np(fwd), c["msd"], c["scale"], dr.matrix_bound(c["P"])) <= 1.0
    else:                                                # the selected atoms as a pool of their own: the same bits
        own = dev(np.ascontiguousarray(c["x"][:, c["sel"]]))
        assert mc.same_bits(sq, metrics.drmsd_matrix(own, min_sep=min_sep, squared=True))
    with pytest.raises(ValueError, match="names an atom twice"):
        metrics.drmsd_matrix(x, sel=[0, 3, 3, 5])


@pytest.mark.parametrize("Na,Nb", [(65, 3), (3, 130)])
def test_two_pools(Na, Nb):
    m, min_sep = 87, 2
    a, b = dr.case(Na, m, min_sep), dr.case(Nb, m, min_sep)
    xa, xb = dev(a["x"]), dev(b["x"])
    msd, scale = dr.msd_cross(a["D"], b["D"])
    got = metrics.drmsd_matrix(xa, xb, min_sep=min_sep, squared=True)
    _check_matrix(got, a, f"cross-{Na}x{Nb}", msd, scale)
    # which pool is the row does not matter, and neither does the call: the element of the joined pool has the same bits
    assert mc.same_bits(got, metrics.drmsd_matrix(xb, xa, min_sep=min_sep, squared=True).T.contiguous())
    joined = metrics.drmsd_matrix(torch.cat((xa, xb)), min_sep=min_sep, squared=True)
    assert mc.same_bits(got, joined[:Na, Na:].contiguous())
    assert mc.same_bits(metrics.drmsd_matrix(xa, xb, min_sep=min_sep), torch.sqrt(got))
    # a generated pool against itself as the "true" one: every structure is at exactly 0 of its own frame
    own = metrics.drmsd_matrix(xa, xa.clone(), min_sep=min_sep)
    assert bool((own.diagonal() == 0).all()) and bool((own.min(1).values == 0).all())
    bad = b["x"].copy()
    bad[1, 4, 0] = np.nan
    got = metrics.drmsd_matrix(xa, dev(bad), min_sep=min_sep, squared=True)
    assert torch.isnan(got[:, 1]).all() and mc.same_bits(got[:, [0, 2]].contiguous(), metrics.drmsd_matrix(xa, xb, min_sep=min_sep, squared=True)[:, [0, 2]].contiguous())


def test_rods_by_hand_to_the_bit():
    for m, min_sep in ((2, 1), (3, 1), (17, 1), (17, 3), (129, 2), (200, 1), (200, 199)):      # 200: two slabs, the split
        got = _np(metrics.drmsd_matrix(dev(dr.rods(m)), min_sep=min_sep, squared=True))
        assert (got == dr.rods_msd(m, min_sep)).all(), (m, min_sep)
    assert _lib.lib().codlad_drmsd_groups(3, 0, 200, 1) == 2 and _lib.lib().codlad_drmsd_groups(3, 0, 129, 1) == 1
    many = np.concatenate([dr.rods(129)] * 30)           # 90 structures: the same three values across two blocks
    got = _np(metrics.drmsd_matrix(dev(many), min_sep=2, squared=True))
    assert (got == np.tile(dr.rods_msd(129, 2), (30, 30))).all()


def test_equal_distance_vectors_are_at_exactly_zero_and_bits_do_not_depend_on_the_pool():
    N, m = 130, 87
    x = dr.case(N, m)["x"].copy()
    q, moved = dr.translated(walk(4, m, seed=7))
    x[0:4], x[64:68], x[126:130] = q, moved, dr.mirrored(q)
    x[100] = x[31]                                       # a duplicate in another block
    xd = dev(x)
    sq = metrics.drmsd_matrix(xd, squared=True)
    for i in range(4):
        assert float(sq[i, 64 + i]) == 0.0 and float(sq[i, 126 + i]) == 0.0 and float(sq[64 + i, 126 + i]) == 0.0
        assert float(sq[i, (i + 1) % 4]) > 0.0
    assert float(sq[31, 100]) == 0.0 and float(sq[100, 31]) == 0.0
    assert mc.same_bits(sq[31].contiguous(), sq[100].contiguous())                            # and the same row of everything else
    assert mc.same_bits(sq, sq.T.contiguous())
    # a permuted pool gives the permuted matrix
    perm = torch.from_numpy(np.random.default_rng(5).permutation(N)).to(xd.device)
    moved_sq = metrics.drmsd_matrix(xd[perm].contiguous(), squared=True)
    assert mc.same_bits(moved_sq, sq[perm][:, perm].contiguous())
    # two structures alone, in either order, and inside the pool
    for i, j in ((5, 77), (64, 129), (63, 64)):
        two = metrics.drmsd_matrix(xd[[i, j]].contiguous(), squared=True)
        assert mc.same_bits(two[0, 1], sq[i, j]) and mc.same_bits(two[1, 0], sq[i, j])
        assert mc.same_bits(metrics.drmsd_matrix(xd[[j, i]].contiguous(), squared=True)[0, 1], sq[i, j])


def test_the_split_changes_no_bit():
    """Two structures of 1100 atoms are one block of 38 slabs: a workgroup per slab.  Inside a pool of 23 x 23 blocks
    every workgroup runs its 38 slabs itself."""
    m, big = 1100, 64 * 22 + 1
    groups = _lib.lib().codlad_drmsd_groups
    assert groups(2, 0, m, 1) == 38 == dr.n_slabs(m) and groups(big, 0, m, 1) == 1
    x2 = walk(2, m, seed=3)
    D = dr.distances(x2)
    msd, scale = dr.msd_cross(D, D)
    split = metrics.drmsd_matrix(dev(x2), squared=True)
    f = dr.worst(_np(split), msd, scale, dr.matrix_bound(D.shape[1]))
    print(f"N2-m{m} (split): largest fraction of the matrix bound: {f:.4f}")
    assert f <= 1.0
    pool = walk(big, m, seed=4)
    pool[5], pool[big - 3] = x2[0], x2[1]
    whole = metrics.drmsd_matrix(dev(pool), squared=True)
    assert mc.same_bits(whole[5, big - 3], split[0, 1]) and mc.same_bits(whole[big - 3, 5], split[0, 1])
    # cross mode on both sides of the rule, too
    cross = metrics.drmsd_matrix(dev(x2[:1]), dev(x2[1:]), squared=True)
    assert groups(1, 1, m, 1) == 38 and mc.same_bits(cross[0, 0], split[0, 1])


def test_the_limit_sized_selection():
    m = 4325                                             # the project's large all-atom shape: 9.35 M pairs, 576 slabs
    x = walk(3, m, seed=1)
    D = dr.distances(x)
    assert D.shape[1] == 9350650 and _lib.lib().codlad_drmsd_groups(3, 0, m, 1) == 576
    msd, scale = dr.msd_cross(D, D)
    got = metrics.drmsd_matrix(dev(x), squared=True)
    f = dr.worst(_np(got), msd, scale, dr.matrix_bound(D.shape[1]))
    print(f"N3-m{m}: largest fraction of the matrix bound: {f:.5f}")
    assert f <= 1.0 and mc.same_bits(got, got.T.contiguous())
    pairs = torch.tensor([[0, 1], [2, 0]])
    direct = metrics.drmsd_pairs(dev(x), dev(x), pairs, squared=True)
    fp = max(float(abs(LD(float(direct[k])) - msd[i, j]) / (LD(dr.pairs_bound(m)) * msd[i, j])) for k, (i, j) in enumerate(pairs.tolist()))
    print(f"N3-m{m}: largest fraction of the pair bound: {fp:.4f}")
    assert fp <= 1.0


@pytest.mark.parametrize("N,m,min_sep", dr.BITMAP_CASES)
def test_the_bitmap_is_the_reference_decision_on_every_pair(N, m, min_sep):
    c = dr.case(N, m, min_sep)
    cutoff = dr.cutoff_of(c)
    assert not dr.undecided(c, cutoff * cutoff)[~np.eye(N, dtype=bool)].any()                 # what the CPU suite has shown
    want = np.array(c["msd"] <= cutoff * cutoff)
    np.fill_diagonal(want, True)
    x = dev(c["x"])
    for return_matrix in (False, True):
        out = metrics.drmsd_neighbours(x, cutoff, min_sep=min_sep, return_matrix=return_matrix)
        got = cr.unpack(_np(out["bits"]), N)
        assert out["bits"].dtype == torch.int64 and tuple(out["bits"].shape) == (N, (N + 63) // 64) and out["n"] == N
        assert (got[:, :N] == want).all() and not got[:, N:].any() and _np(out["finite"]).all()
        assert ("drmsd" in out) == return_matrix
    assert mc.same_bits(out["drmsd"], metrics.drmsd_matrix(x, min_sep=min_sep))
    res = metrics.cluster_drmsd(x, cutoff, min_sep=min_sep)
    ref = cr.daura(got[:, :N])
    assert (_np(res["labels"]) == ref["labels"]).all() and (_np(res["centres"]) == ref["centres"]).all()
    assert (_np(res["sizes"]) == ref["sizes"]).all() and res["n_clusters"] == ref["n_clusters"]


def test_non_finite_input_has_a_defined_result():
    N, m = 70, 43
    x0 = walk(N, m, seed=2)
    sel = list(range(0, m, 2)) + [1]                     # 23 positions; atom 3 is not among them
    ms = len(sel)
    c0 = metrics.cluster_drmsd(dev(x0), 6.0, sel=sel, min_sep=2, return_matrix=True)
    keep = [i for i in range(N) if i not in (1, 66)]
    for bad in (np.nan, np.inf, -np.inf):
        x = x0.copy()
        x[1, sel[3], 1] = bad
        x[66, sel[-1], 0] = bad
        x[2, 3, 2] = bad                                 # an unselected atom: changes nothing
        out = metrics.cluster_drmsd(dev(x), 6.0, sel=sel, min_sep=2, return_matrix=True)
        fin = np.ones(N, dtype=bool)
        fin[[1, 66]] = False
        assert (_np(out["finite"]) == fin).all()
        d = out["drmsd"]
        assert torch.isnan(d[[1, 66]]).all() and torch.isnan(d[:, [1, 66]]).all()
        assert mc.same_bits(d[keep][:, keep].contiguous(), c0["drmsd"][keep][:, keep].contiguous())
        bits, bits0 = cr.unpack(_np(out["bits"]), N), cr.unpack(_np(c0["bits"]), N)
        assert not bits[[1, 66]].any() and not bits[:, [1, 66]].any() and not bits[:, N:].any()
        assert (bits[keep][:, keep] == bits0[keep][:, keep]).all() and bits[keep, keep].all()
        lab = _np(out["labels"])
        assert lab[1] == -1 and lab[66] == -1 and (lab[keep] >= 0).all()
        ref = cr.daura(bits[:, :N], finite=fin)
        assert (lab == ref["labels"]).all() and np.isnan(_np(out["centre_drmsd"])[[1, 66]]).all()
        pairs = torch.tensor([[0, 1], [2, 3], [66, 5]])
        direct, pos = metrics.drmsd_pairs(dev(x), dev(x), pairs, sel=sel, min_sep=2, per_position=True)
        assert np.isnan(_np(direct)).tolist() == [True, False, True] and torch.isnan(pos[[0, 2]]).all() and tuple(pos.shape) == (3, ms)
        assert torch.isfinite(pos[1]).all()
    assert _np(c0["finite"]).all()


@pytest.mark.parametrize("m,min_sep", [(87, 1), (87, 3), (5, 4), (2, 1), (129, 2)])
def test_the_pair_route_and_its_per_position_rows(m, min_sep):
    a, b = walk(9, m, seed=11), walk(7, m, seed=12)
    rng = np.random.default_rng(m)
    pairs = np.stack((rng.integers(0, 9, 12), rng.integers(0, 7, 12)), 1)
    msd, _ = dr.msd_cross(dr.distances(a, None, min_sep), dr.distances(b, None, min_sep))
    got, pos = metrics.drmsd_pairs(dev(a), dev(b), torch.from_numpy(pairs), min_sep=min_sep, per_position=True, squared=True)
    only = metrics.drmsd_pairs(dev(a), dev(b), torch.from_numpy(pairs), min_sep=min_sep, squared=True)
    assert mc.same_bits(got, only) and mc.same_bits(torch.sqrt(got), metrics.drmsd_pairs(dev(a), dev(b), torch.from_numpy(pairs), min_sep=min_sep))
    want = np.array([msd[i, j] for i, j in pairs])
    f = float(np.max(np.abs(_np(got).astype(LD) - want) / (LD(dr.pairs_bound(m)) * want)))
    fp = 0.0
    for k, (i, j) in enumerate(pairs):
        ref = dr.position_ld(dr.table32(a[i]), dr.table32(b[j]), m, min_sep)
        has = np.isfinite(ref)                           # a position without partners is 0 / 0
        assert (np.isnan(_np(pos[k])) == ~has).all()
        fp = max(fp, float(np.max(np.abs(_np(pos[k]).astype(LD)[has] - ref[has]) / (LD(dr.position_bound(m)) * ref[has]))))
    print(f"m{m}-sep{min_sep}: largest fraction of the bound: pairs {f:.3f}, per position {fp:.3f}")
    assert f <= 1.0 and fp <= 1.0
    # the matrix route agrees within the two bounds
    tab = metrics.drmsd_matrix(dev(a), dev(b), min_sep=min_sep, squared=True)
    _, scale = dr.msd_cross(dr.distances(a, None, min_sep), dr.distances(b, None, min_sep))
    for k, (i, j) in enumerate(pairs):
        lim = LD(dr.matrix_bound(dr.n_pairs(m, min_sep))) * scale[i, j] + LD(dr.pairs_bound(m)) * msd[i, j]
        assert abs(LD(float(tab[i, j])) - LD(float(got[k]))) <= lim


def test_clustering_of_a_planted_pool_whatever_the_orientation():
    for rotate in (False, True):
        x, member = dr.planted(rotate=rotate)
        N, m = x.shape[:2]
        P = dr.n_pairs(m)
        D = dr.distances(x)
        msd, scale = dr.msd_cross(D, D)
        out = {rm: metrics.cluster_drmsd(dev(x), 1.0, return_matrix=rm) for rm in (False, True)}
        for rm, res in out.items():
            lab = _np(res["labels"])
            assert res["n_clusters"] == 3 and sorted(_np(res["sizes"]).tolist()) == [5, 7, 9] and ("drmsd" in res) == rm
            for k in range(3):
                assert len(set(member[lab == k])) == 1   # the planted membership
            ref = cr.daura(cr.unpack(_np(res["bits"]), N)[:, :N])
            assert (lab == ref["labels"]).all() and (_np(res["centres"]) == ref["centres"]).all()
            assert abs(float(res["populations"].sum()) - 1.0) <= 1e-15
        assert (_np(out[False]["labels"]) == _np(out[True]["labels"])).all()
        # centre_drmsd by the pair route and read from the matrix: each within its bound of the reference
        lab, centres = _np(out[True]["labels"]), _np(out[True]["centres"])
        for i in range(N):
            j = centres[lab[i]]
            direct, table = LD(float(out[False]["centre_drmsd"][i])) ** 2, LD(float(out[True]["centre_drmsd"][i])) ** 2
            slack = 4 * dr.EPS * msd[i, j]               # the root and this square
            assert abs(direct - msd[i, j]) <= dr.pairs_bound(m) * msd[i, j] + slack
            assert abs(table - msd[i, j]) <= dr.matrix_bound(P) * scale[i, j] + slack
        w = np.random.default_rng(1).uniform(0.5, 2.0, N)
        res = metrics.cluster_drmsd(dev(x), 1.0, weights=w)
        want = np.array([w[lab == k].sum() for k in range(3)]) / w.sum()
        assert np.abs(_np(res["populations"]) - want).max() <= 1e-14


def test_buffers_are_written_before_they_are_read_and_only_inside():
    """tests/memcheck.py around one one-pool call, one cross call and one split call, the pair route and the clustering:
    the same bits under the three fills of every buffer the package allocates, no zone byte changed."""
    from tests.test_buffer_discipline import hold
    one = dr.case(65, 33, 2)["x"].copy()
    one[7, 4, 2] = np.nan
    other = dr.case(3, 33, 2)["x"].copy()
    long2 = walk(2, 200, seed=9)                         # two slabs: the split path
    sel = list(range(1, 30, 2))
    pairs = torch.tensor([[0, 1], [7, 2], [64, 0]])

    def case(g):
        out = {}
        a = metrics.cluster_drmsd(g(torch.from_numpy(one), "x"), 5.0, min_sep=2, return_matrix=True)
        out.update({f"one_{k}": v for k, v in a.items() if torch.is_tensor(v)})
        b = metrics.cluster_drmsd(g(torch.from_numpy(one), "x"), 5.0, sel=sel)
        out.update({f"sel_{k}": v for k, v in b.items() if torch.is_tensor(v)})
        out["cross"] = metrics.drmsd_matrix(g(torch.from_numpy(one), "x"), g(torch.from_numpy(other), "y"), min_sep=2)
        out["split"] = metrics.drmsd_matrix(g(torch.from_numpy(long2), "x"), squared=True)
        out["split_cross"] = metrics.drmsd_matrix(g(torch.from_numpy(long2), "x"), g(torch.from_numpy(long2[:1]), "y"))
        out["pairs"], out["pos"] = metrics.drmsd_pairs(g(torch.from_numpy(one), "a"), g(torch.from_numpy(other), "b"), pairs, sel=sel,
                                                       per_position=True)
        return out, []
    hold("drmsd", case)
