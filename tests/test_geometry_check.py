"""Reference-free geometry check (codlad_geometry_check, csrc/geometry_kernels.hip; metrics.geometry_check).

The kernel is held to a float64 all-pairs reference written here in numpy, on inputs whose every pair distance keeps
1e-4 A away from every threshold it is compared with (asserted): a distance computed in fp32 from fp32 coordinates is off
by a few 1e-7 A relative at most, the fp32 thresholds (1.3f, (r_i + r_j) in fp32, the 1e-7 under the clash root) by less
than 1e-6 A, so no decision can differ and the five counts must be EXACTLY equal.  Sizes: 2 and 4 atoms, one below / at /
one above the kernel's row block (256) and column tile (1024), and 2100 atoms (three column tiles), for 1 and 3 structures.
The inputs and their references are built once per size on the CPU and shared."""
import functools

import numpy as np
import pytest
import torch

from codlad_amd import metrics
from codlad_amd.utils import dataset_builder as db
from codlad_amd.utils.cg_input import template_topology

SCALE, CLASH, NEAR, ORDER, MARGIN = 1.3, 1.2, 9.0, 2, 1e-4
SIZES = (2, 4, 255, 256, 257, 1023, 1024, 1025, 2100)
R_C = 0.68


# ------------------------------------------------------------------------------------------------- float64 reference
_EXCLUDED = {}


def excluded_matrix(bonds, order, n):
    """bool [n, n]: within `order` bonds (dataset_builder.high_order_edges, the dense construction of the reference)."""
    key = (np.asarray(bonds).tobytes(), order, n)
    if key not in _EXCLUDED:
        _EXCLUDED[key] = _excluded_matrix(np.asarray(bonds, dtype=np.int64).reshape(-1, 2), order, n)
    return _EXCLUDED[key]


def _excluded_matrix(bonds, order, n):
    m = np.zeros((n, n), dtype=bool)
    if len(bonds):
        e = db.high_order_edges(torch.as_tensor(bonds, dtype=torch.int64), order, n).numpy()
        m[e[:, 0], e[:, 1]] = True
    return m | m.T


def pair_table(x, radius, bonds, order=ORDER, scale=SCALE):
    """All pairs i < j of one structure in float64: (i, j, d, cut, is_bond, is_excluded)."""
    n = x.shape[0]
    i, j = np.triu_indices(n, 1)
    x = x.astype(np.float64)
    d = np.sqrt(((x[i] - x[j]) ** 2).sum(-1))
    cut = (radius.astype(np.float64)[i] + radius.astype(np.float64)[j]) * scale
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    bond = np.zeros((n, n), dtype=bool)
    bond[bonds[:, 0], bonds[:, 1]] = True
    return i, j, d, cut, bond[i, j], excluded_matrix(bonds, order, n)[i, j]


def reference(x, radius, bonds, order=ORDER, scale=SCALE, clash=CLASH, near=NEAR):
    _i, _j, d, cut, bond, excl = pair_table(x, radius, bonds, order, scale)
    free = ~excl
    counts = [int((bond & (d >= cut)).sum()), int((~bond & (d < cut)).sum()), int((d < cut).sum()),
              int((free & (d <= near)).sum()), int((free & (np.sqrt(d * d + 1e-7) < clash)).sum())]
    return counts, float(d[free].min()) if free.any() else float("inf")


def too_close_to_a_threshold(x, radius, bonds):
    """Pairs (i, j) whose distance lies within MARGIN of a threshold it is compared with."""
    i, j, d, cut, _bond, _excl = pair_table(x, radius, bonds)
    bad = (np.abs(d - cut) < MARGIN) | (np.abs(d - CLASH) < MARGIN) | (np.abs(d - NEAR) < MARGIN)
    return i[bad], j[bad]


@functools.lru_cache(maxsize=None)
def case(n):
    """A generic topology of n atoms and 3 structures of it, with their float64 references.  Bonds are local in index (a
    random tree over the 3 preceding atoms plus a few ring closures); coordinates are a straight chain (1.2 A apart) plus
    N(0, 1 A) offsets, so that bonds break, non-bonded atoms bond and clash.  Pairs that land within MARGIN of a threshold
    are moved off it here, on the CPU."""
    rng = np.random.default_rng(1000 + n)
    radius = rng.choice(np.array([0.68, 0.68, 0.64, 1.02, 0.35], dtype=np.float32), n).astype(np.float32)
    bonds = {(k - int(rng.integers(1, min(k, 3) + 1)), k) for k in range(1, n)}
    bonds |= {(k, k + int(rng.integers(2, 6))) for k in range(0, max(n - 6, 0)) if rng.random() < 0.1}
    bonds = np.array(sorted(bonds), dtype=np.int64).reshape(-1, 2)
    chain = np.stack([1.2 * np.arange(n), np.zeros(n), np.zeros(n)], 1)
    xyz = (chain[None] + rng.normal(0, 1.0, (3, n, 3))).astype(np.float32)
    for s in range(3):
        for _ in range(50):
            _i, j = too_close_to_a_threshold(xyz[s], radius, bonds)
            if not len(j):
                break
            xyz[s, np.unique(j)] += rng.normal(0, 0.01, (len(np.unique(j)), 3)).astype(np.float32)
    refs = [reference(xyz[s], radius, bonds) for s in range(3)]
    return radius, bonds, xyz, refs


def run(xyz, radius, bonds, **kw):
    out = metrics.geometry_check_lists(torch.from_numpy(np.ascontiguousarray(xyz)).cuda(), torch.from_numpy(radius), bonds,
                                       **kw)
    return out["counts"].cpu().numpy(), out["min_dist"].cpu().numpy(), out


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("order", [1, 2, 3])
def test_exclusion_csr_is_the_pair_set_of_high_order_edges(order):
    top = template_topology(["MET", "TRP", "PRO", "GLY", "HIS", "ARG", "TPO", "PHE"], chain_ids=[0] * 5 + [1] * 3)
    bonds, n = db.standard_bonds(top), top.n_atoms
    ptr, words = metrics.exclusion_csr(bonds, order, n)
    assert ptr.dtype == torch.int32 and words.dtype == torch.int32 and ptr.shape == (n + 1,) and int(ptr[-1]) == len(words)
    flag = metrics._lib.GEOM_BOND_FLAG
    rows = [[int(w) for w in words[int(ptr[i]):int(ptr[i + 1])]] for i in range(n)]
    partners = [[w & ~flag for w in row] for row in rows]
    pairs = {(i, j) for i, row in enumerate(partners) for j in row}
    want = {tuple(e) for e in db.high_order_edges(bonds, order, n).tolist()}
    assert {p for p in pairs if p[0] < p[1]} == want and len(want) > n
    assert all(row == sorted(set(row)) and i not in row for i, row in enumerate(partners))          # sorted, no self, no repeats
    assert all((j, i) in pairs for i, j in pairs)                                                   # symmetric
    bonded = {(i, w & ~flag) for i, row in enumerate(rows) for w in row if w & flag}
    both_ways = {tuple(b) for b in bonds.tolist()} | {(j, i) for i, j in bonds.tolist()}
    assert bonded == both_ways                                                                       # order-1 partners flagged
    with pytest.raises(ValueError):
        metrics.exclusion_csr(torch.tensor([[0, n]]), order, n)


def test_generated_inputs_exercise_every_category_and_keep_their_margin():
    seen = np.zeros(5, dtype=bool)
    for n in SIZES:
        radius, bonds, xyz, refs = case(n)
        for s in range(3):
            assert not len(too_close_to_a_threshold(xyz[s], radius, bonds)[0]), (n, s)
            seen |= np.array(refs[s][0]) > 0
        if n >= 255:                                   # every size beyond the toy ones shows every category by itself
            got = np.array([r[0] for r in refs])
            assert (got[:, 0] > 0).any() and (got[:, 1] > 0).any() and (got[:, 4] > 0).any(), (n, got)
            assert all(r[0][2] == len(bonds) - r[0][0] + r[0][1] for r in refs)
    assert seen.all()


def test_cpu_tensors_raise_and_the_tables_live_on_the_topology():
    top = template_topology(["ALA", "GLY", "SER"])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        metrics.geometry_check(torch.zeros(1, top.n_atoms, 3), top)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        metrics.geometry_check_lists(torch.zeros(1, 2, 3), [R_C, R_C], [[0, 1]])


# ------------------------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n_struct", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_against_float64_all_pairs(n, n_struct):
    radius, bonds, xyz, refs = case(n)
    counts, dmin, _ = run(xyz[:n_struct], radius, bonds)
    for s in range(n_struct):
        print(f"n={n} S={n_struct} s={s}: kernel {counts[s].tolist()} min {dmin[s]:.7g}  reference {refs[s][0]} min {refs[s][1]:.7g}")
    for s in range(n_struct):
        assert not len(too_close_to_a_threshold(xyz[s], radius, bonds)[0])
        assert counts[s].tolist() == refs[s][0], (s, counts[s].tolist(), refs[s][0])
        want = refs[s][1]
        assert (np.isinf(want) and np.isinf(dmin[s]) and dmin[s] > 0) or abs(dmin[s] - want) <= 1e-5 * want, (s, dmin[s], want)
        assert counts[s][2] == len(bonds) - counts[s][0] + counts[s][1]


@pytest.mark.gpu
def test_hand_made_cases():
    r2 = np.array([R_C, R_C], dtype=np.float32)
    cut = (R_C + R_C) * 1.3                                                    # 1.768
    pair = lambda d: np.array([[[0, 0, 0], [d, 0, 0]]], dtype=np.float32)      # noqa: E731
    inf = float("inf")
    # a bonded pair just inside / outside (r_i + r_j) * 1.3: intact, then broken and no longer in the graph
    c, m, out = run(pair(cut - 1e-3), r2, [[0, 1]])
    assert c[0].tolist() == [0, 0, 1, 0, 0] and m[0] == inf and bool(out["valid"][0])
    c, m, out = run(pair(cut + 1e-3), r2, [[0, 1]])
    assert c[0].tolist() == [1, 0, 0, 0, 0] and m[0] == inf and not bool(out["valid"][0])
    # a non-excluded pair at 1.19 A clashes (and bonds spuriously), at 1.21 A it does not clash
    none = np.zeros((0, 2), dtype=np.int64)
    c, m, out = run(pair(1.19), r2, none)
    assert c[0].tolist() == [0, 1, 1, 1, 1] and abs(m[0] - 1.19) < 1e-6 and not bool(out["valid"][0])
    c, m, _ = run(pair(1.21), r2, none)
    assert c[0].tolist() == [0, 1, 1, 1, 0] and abs(m[0] - 1.21) < 1e-6
    c, m, out = run(pair(9.5), r2, none)
    assert c[0].tolist() == [0, 0, 0, 0, 0] and abs(m[0] - 9.5) < 1e-5 and bool(out["valid"][0])
    # 0 - 1 - 2 with the order-2 pair (0, 2) at 1.0 A: not a clash (within 2 bonds), but a bond the template does not have;
    # and no pair is more than 2 bonds apart: min_dist = inf, near = clash = 0
    tri = np.array([[[0, 0, 0], [0.5, 1.4, 0], [1.0, 0, 0]]], dtype=np.float32)
    r3 = np.array([R_C] * 3, dtype=np.float32)
    c, m, out = run(tri, r3, [[0, 1], [1, 2]])
    assert c[0].tolist() == [0, 1, 3, 0, 0] and m[0] == inf and not bool(out["valid"][0])
    # the same atoms with order 1: (0, 2) is now a free pair, near and clashing
    c, m, _ = run(tri, r3, [[0, 1], [1, 2]], order=1)
    assert c[0].tolist() == [0, 1, 3, 1, 1] and abs(m[0] - 1.0) < 1e-6
    # a single atom has no pairs
    c, m, _ = run(np.zeros((2, 1, 3), dtype=np.float32), r2[:1], none)
    assert not c.any() and (m == inf).all()


def protein_case():
    """The golden N6_L46_B3 coordinates (reference-generated), three frames as they are and three with 0.3 A noise, and the
    template topology of their interior residues."""
    from tests.test_dataset_builder import golden_frames
    top, full, _og, _info, _g5 = golden_frames("N6_L46_B3")
    inner = template_topology(top.res_names).subset_residues(1, top.n_residues - 1)
    x = full[:, 1:-1]
    noisy = x + np.random.default_rng(5).normal(0, 0.3, x.shape).astype(np.float32)
    return inner, np.concatenate([x, noisy]).astype(np.float32)


@pytest.mark.gpu
def test_bonded_count_equals_the_pinned_bond_graph_kernel():
    top, x = protein_case()
    xyz = torch.from_numpy(x).cuda()
    geo = metrics.geometry_check(xyz, top)
    flat = xyz.reshape(-1, 3)
    pinned = metrics.bond_graph_counts(flat, flat, [top.n_atoms] * x.shape[0], np.tile(top.atomic_nums(), x.shape[0]))
    assert torch.equal(geo["bonded"], pinned[:, 4]) and torch.equal(geo["bonded"], pinned[:, 1])
    n_bonds = db.standard_bonds(top).shape[0]
    assert torch.equal(geo["bonded"], n_bonds - geo["broken"] + geo["spurious"])
    counts = geo["counts"].cpu().numpy()
    print(counts.tolist(), geo["min_dist"].tolist())
    assert counts[3:, 0].max() > 0 and (counts[:, 3] > 1000).all()              # the noisy frames break bonds
    assert torch.equal(geo["valid"], (geo["broken"] == 0) & (geo["spurious"] == 0)) and geo["valid"].dtype == torch.bool
    # the float64 reference on real residue templates (no margin is asserted here: compare the order-independent parts)
    radius = np.array(metrics.COV_CUTOFF, dtype=np.float32)[top.atomic_nums() - 1]
    for s in (0, 3):
        want, dmin = reference(x[s], radius, db.standard_bonds(top).numpy())
        if not len(too_close_to_a_threshold(x[s], radius, db.standard_bonds(top).numpy())[0]):
            assert counts[s].tolist() == want and abs(float(geo["min_dist"][s]) - dmin) <= 1e-5 * dmin


@pytest.mark.gpu
def test_results_are_bit_identical_and_independent_of_the_batch():
    radius, bonds, xyz, _refs = case(1025)
    c1, m1, _ = run(xyz, radius, bonds)
    c2, m2, _ = run(xyz, radius, bonds)
    assert c1.tobytes() == c2.tobytes() and m1.tobytes() == m2.tobytes()
    for s in range(3):
        cs, ms, _ = run(xyz[s:s + 1], radius, bonds)
        assert cs[0].tobytes() == c1[s].tobytes() and ms[0].tobytes() == m1[s].tobytes()
    top, x = protein_case()
    a = metrics.geometry_check(torch.from_numpy(x).cuda(), top)
    assert set(top._geometry_tables) == {(2, "cuda:0")}                       # cached on the topology, per order and device
    tables = top._geometry_tables[(2, "cuda:0")]
    b = metrics.geometry_check(torch.from_numpy(x).cuda(), top)
    assert top._geometry_tables[(2, "cuda:0")] is tables
    assert torch.equal(a["counts"], b["counts"]) and torch.equal(a["min_dist"], b["min_dist"])
    metrics.geometry_check(torch.from_numpy(x).cuda(), top, order=3)
    assert set(top._geometry_tables) == {(2, "cuda:0"), (3, "cuda:0")}
    with pytest.raises(ValueError, match="atoms"):
        metrics.geometry_check(torch.from_numpy(x[:, :-1].copy()).cuda(), top)


@pytest.mark.gpu
def test_c_abi_rejects_bad_arguments_before_any_launch():
    from codlad_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(1, 2, 3, device="cuda")
    r = torch.full((2,), R_C, device="cuda")
    ptr = torch.zeros(3, dtype=torch.int32, device="cuda")
    counts = torch.zeros(1, 5, dtype=torch.int32, device="cuda")
    dmin = torch.zeros(1, device="cuda")
    p = _lib.ptr
    import ctypes as C
    f = C.c_float
    ok = (p(x), 1, 2, p(r), p(ptr), None, None, 0, f(1.3), f(1.2), f(9.0), p(counts), p(dmin), None)
    for k, bad in ((0, None), (1, 0), (2, 0), (2, 1 << 30), (2, 70000), (7, -1), (7, 1), (8, f(0.0)), (11, None), (12, None)):
        args = list(ok)
        args[k] = bad
        assert lib.codlad_geometry_check(*args) != 0, k
        assert b"codlad_geometry_check" in lib.codlad_last_error()
