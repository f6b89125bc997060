"""CPU: the host side of the restrained clash relaxation (metrics.relax_tables) against tests/relax_ref.py, the reference
itself against central differences, the C ABI's declaration, and the conditions the planted inputs of tests/test_relax.py
must meet - all decided by the float64 reference, before the device sees anything."""
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from codlad_amd.utils import dataset_builder as db
from codlad_amd.utils.cg_input import template_topology
from tests import relax_ref as rr
from tests import stereo_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def eight_residues():
    return template_topology(["MET", "TRP", "PRO", "GLY", "HIS", "ARG", "TPO", "PHE"], chain_ids=[0] * 5 + [1] * 3)


def csr_rows(ptr, words):
    flag = _lib.GEOM_BOND_FLAG
    return [[int(w) & ~flag for w in words[int(ptr[i]):int(ptr[i + 1])]] for i in range(len(ptr) - 1)]


def test_pair_set_is_high_order_edges_of_order_2():
    top = eight_residues()
    tab = metrics.relax_tables(top)
    n, bonds = top.n_atoms, db.standard_bonds(top)
    rows = csr_rows(tab["pair_ptr"], tab["pair_j"])
    pairs = {(i, j) for i, row in enumerate(rows) for j in row}
    want = {tuple(e) for e in db.high_order_edges(bonds, 2, n).tolist()}
    assert {p for p in pairs if p[0] < p[1]} == want and len(want) > n
    assert all(row == sorted(set(row)) and i not in row for i, row in enumerate(rows))
    assert all((j, i) in pairs for i, j in pairs)
    assert tab["pair_ptr"].dtype == torch.int32 and tab["pair_j"].dtype == torch.int32
    # the repulsion's exclusion follows `order`; the restrained pairs do not
    tab3 = metrics.relax_tables(top, order=3)
    assert torch.equal(tab3["pair_j"], tab["pair_j"]) and tab3["excl"].numel() > tab["excl"].numel()
    assert torch.equal(tab["excl"], tab["pair_j"])
    assert metrics.relax_tables(top) is tab and set(top._relax_tables) == {(2, "host"), (3, "host")}      # kept on the topology
    assert tab["fixed"].dtype == torch.bool and tab["fixed"].tolist() == (top.name == "CA").tolist()
    want_r = np.array(metrics.COV_CUTOFF, dtype=np.float32)[top.atomic_nums() - 1]
    assert np.array_equal(tab["radius"].numpy(), want_r)


def test_ring_bonds_are_the_ones_expected_by_residue_name():
    top = eight_residues()
    tab = metrics.relax_tables(top)
    ring, peptide, arg = rr.expected_rigid_bonds(top)
    assert len(ring) == 5 + 10 + 5 + 6 and len(peptide) == 4 + 2 and len(arg) == 1          # PRO, TRP, HIS, PHE; two chains
    got = set(metrics.ring_bonds(db.standard_bonds(top), top.n_atoms))
    assert got == ring
    assert {tuple(b) for b in tab["rigid"].tolist()} == ring | peptide | arg
    # generic graphs: a triangle with a tail, two fused squares
    assert metrics.ring_bonds([[0, 1], [1, 2], [0, 2], [2, 3]], 4) == [(0, 1), (0, 2), (1, 2)]
    assert metrics.ring_bonds([[0, 1], [1, 2], [2, 3], [0, 3], [2, 4], [4, 5], [3, 5], [5, 6]], 7) == \
        [(0, 1), (0, 3), (1, 2), (2, 3), (2, 4), (3, 5), (4, 5)]


def test_quad_set_is_the_brute_force_enumeration():
    top = eight_residues()
    tab = metrics.relax_tables(top)
    n, bonds = top.n_atoms, db.standard_bonds(top).numpy()
    ring, peptide, arg = rr.expected_rigid_bonds(top)
    want = rr.brute_quads(bonds, ring | peptide | arg, n)
    got = tab["quads"].numpy().astype(np.int64)
    assert tab["quads"].dtype == torch.int32 and got.shape[1] == 4
    assert len(got) == len(want) and {tuple(q) for q in got} == {tuple(q) for q in want} and len(want) > 50
    assert len({tuple(q) for q in got}) == len(got)
    # the per-atom CSR lists exactly the quads an atom is part of, with its position, in ascending order
    ptr, ref = tab["quad_ptr"].tolist(), tab["quad_ref"].tolist()
    assert len(ptr) == n + 1 and ptr[-1] == len(ref) == 4 * len(got)
    for i in range(n):
        row = ref[ptr[i]:ptr[i + 1]]
        assert row == sorted(row) and all(got[r >> 2, r & 3] == i for r in row)
        assert len(row) == int((got == i).sum())
    with pytest.raises(ValueError):
        metrics.quad_csr([[0, 1, 2, n]], n)


@pytest.fixture(scope="module")
def thirty():
    """A 30-residue chain through all 22 templates, displaced by N(0, 0.15 A) from its start structure, with two atoms
    pushed to 0.9 A of each other: all three terms are active."""
    rng = np.random.default_rng(11)
    pl = sr.planted(30, 3)
    pl.update(omega=np.full(30, 180.0), d_ca=None, d_side=None)
    top, x0 = sr.build_chain(**pl)
    tab, T = rr.case_tables(top)
    x = x0 + rng.normal(0, 0.15, x0.shape)
    return top, tab, T, x0, x


def test_reference_gradient_agrees_with_central_differences_on_every_coordinate(thirty):
    top, _tab, T, x0, x = thirty
    e, g, gmax = rr.energy(x, x0, T)
    assert (e > 1.0).all() and gmax == np.abs(g).max()                     # all three terms are active
    h, worst = 1e-5, 0.0
    for a in range(top.n_atoms):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[a, c] += h
            xm[a, c] -= h
            fd = (rr.energy(xp, x0, T)[0].sum() - rr.energy(xm, x0, T)[0].sum()) / (2 * h)
            worst = max(worst, abs(fd - g[a, c]) / (1.0 + abs(fd)))
    print(f"largest |central difference - analytic| / (1 + |gradient|) over {3 * top.n_atoms} coordinates: {worst:.2e}")
    assert worst < 1e-6
    # fixed atoms: gradient 0, energy unchanged; the start structure against itself: no restraint energy
    fixed = top.name == "CA"
    e_f, g_f, _ = rr.energy(x, x0, T, fixed)
    assert np.array_equal(e_f, e) and not g_f[fixed].any() and np.array_equal(g_f[~fixed], g[~fixed])
    e0 = rr.energy(x0, x0, T)[0]
    assert e0[0] == 0.0 and e0[1] == 0.0


def test_float32_evaluation_is_close_to_float64(thirty):
    _top, _tab, T, x0, x = thirty
    x32, x032 = x.astype(np.float32), x0.astype(np.float32)
    e64, g64, _ = rr.energy(x32, x032, T)
    e32, g32, _ = rr.energy(x32, x032, T, dtype=np.float32)
    assert g32.dtype == np.float32 and np.abs(e32 - e64).max() < 1e-2 and 0 < np.abs(g32 - g64).max() < 1e-2


def test_header_and_binding_agree_on_the_new_symbols():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    declared = set(re.findall(r"\b(codlad_[a-z0-9_]+)\s*\(", header))
    new = {"codlad_relax", "codlad_relax_energy", "codlad_relax_scratch_bytes"}
    assert new <= declared and new <= set(_lib.exported_symbols())
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19
    assert len(_lib._SIGS["codlad_relax"][1]) == len(re.search(r"int codlad_relax\(([^;]*)\);", header).group(1).split(","))
    assert len(_lib._SIGS["codlad_relax_energy"][1]) == \
        len(re.search(r"int codlad_relax_energy\(([^;]*)\);", header).group(1).split(","))


def test_cpu_tensors_raise():
    top = template_topology(["ALA", "GLY", "SER"])
    x = torch.zeros(1, top.n_atoms, 3)
    for call in (lambda: metrics.relax(x, top), lambda: metrics.relax_energy(x, top),
                 lambda: metrics.relax_lists(torch.zeros(1, 2, 3), [0.68, 0.68], [[0, 1]], []),
                 lambda: metrics.relax_energy_lists(torch.zeros(1, 2, 3), [0.68, 0.68], [[0, 1]], [])):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()


# ------------------------------------------------------------------------------------------------ the planted inputs
@pytest.mark.parametrize("key", list(rr.PLANTED))
def test_planted_case_meets_its_conditions(key):
    """What tests/test_relax.py relies on, by the float64 reference: the clean chain has NO free pair under sigma and the
    reference leaves it alone; the planted chain has clashes; the reference run ends with every free pair at >= 1.2 + 0.2 A,
    keeps every quad bond angle in [60, 150] degrees along the whole trajectory, and leaves every stereo flag as planted
    (none), with stereo_ref's margins (|omega| 0.5 degrees from 30 and 150, |v| >= 0.1 A^3)."""
    c = rr.planted_case(key)
    top, T = c["top"], c["T"]
    n_res = rr.PLANTED[key][0]
    assert top.n_residues == n_res and len(c["residues"]) == rr.PLANTED[key][2]
    if key == "r140":
        assert top.n_atoms > 1024
    sig = (T["radius"][T["free_i"]] + T["radius"][T["free_j"]]) * rr.DEFAULTS["contact_scale"]
    assert (rr.free_pair_distances(c["xyz0"], T) >= sig).all()
    assert rr.clashes(c["xyz"], T) >= len(c["residues"]) and rr.clashes(c["xyz0"], T) == 0
    moved = np.nonzero(np.abs(c["xyz"] - c["xyz0"]).max(1) > 0)[0]
    assert set(top.residue_of_atom[moved].tolist()) == set(c["residues"])            # only the planted side chains differ
    angles = [180.0, 0.0]

    def watch(x):
        a = rr.quad_angles(x, T["quads"])
        angles[0], angles[1] = min(angles[0], float(a.min())), max(angles[1], float(a.max()))
    out = rr.minimise(c["xyz"], T, c["n_iter"], c["fixed"], watch=watch)
    d_min = float(rr.free_pair_distances(out["xyz"], T).min())
    print(f"{key}: {top.n_atoms} atoms, {len(T['quads'])} quads, clashes {rr.clashes(c['xyz'], T)} -> {rr.clashes(out['xyz'], T)}, "
          f"E {out['energy'][0]:.2f} -> {out['energy'][-1]:.4f}, {int(out['accepted'].sum())} accepted, closest free pair "
          f"{d_min:.3f} A, quad angles {angles[0]:.1f} .. {angles[1]:.1f}")
    assert d_min >= rr.CLEAN and rr.clashes(out["xyz"], T) == 0
    assert 60.0 <= angles[0] and angles[1] <= 150.0
    assert np.array_equal(out["xyz"][c["fixed"]], c["xyz"][c["fixed"]].astype(np.float64))
    assert (np.diff(out["energy"]) <= 0).all() and out["energy"][-1] < out["energy"][0]
    for x in (c["xyz"], out["xyz"]):
        v, flags, counts = sr.reference(x, top)
        assert not flags.any() and not counts.any()
        w = np.abs(v[..., 2])
        assert np.nanmin(np.minimum(np.abs(w - 30.0), np.abs(w - 150.0))) >= 0.5 and np.nanmin(np.abs(v[..., 7:])) >= 0.1
    # the clean chain: energy 0, gradient 0, nothing to do
    e, g, gmax = rr.energy(c["xyz0"], c["xyz0"], T, c["fixed"])
    assert not e.any() and not g.any() and gmax == 0.0
