"""CPU: the lDDT reference (tests/lddt_ref.py) against cases derived by hand, the cap on the decisions its float64 sandwich
leaves open, the symmetry table against the residue templates, and what metrics.lddt decides without a device."""
import importlib
import os

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from codlad_amd.utils.cg_input import template_topology
from tests import lddt_ref as lr
from tests import stereo_ref as sr

ml = importlib.import_module("codlad_amd.metrics.lddt")          # metrics.lddt is the function
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def line(xs, res):
    """Atoms on the x axis at `xs`, residue numbers `res`."""
    x = np.zeros((len(xs), 3), dtype=np.float32)
    x[:, 0] = xs
    return x, np.asarray(res)


@pytest.mark.parametrize("dtype", (np.float64, np.float32))
def test_reference_on_the_hand_derived_cases(dtype):
    model, ref, res_ptr, kept_sums, score = lr.toy()
    res = np.repeat(np.arange(2), np.diff(res_ptr))
    same = lr.evaluate(ref, ref, res, dtype)
    assert same["score"] == 1.0 and (same["residue"] == 1.0).all() and same["atom_total"].tolist() == [5, 1, 1, 1, 1, 1]
    out = lr.evaluate(model, ref, res, dtype)
    assert out["atom_preserved"].sum(1).tolist() == kept_sums and out["atom_preserved"][0].tolist() == [1, 2, 3, 4]
    assert out["score"] == score == 0.5 and out["residue"].tolist() == [0.5, 0.5]
    # a displacement of exactly 0.5 is not preserved at 0.5; 0.4375 is
    for shift, want in ((0.5, [0, 1, 1, 1]), (0.4375, [1, 1, 1, 1])):
        ref2, res2 = line([0.0, 2.0], [0, 1])
        mod2 = ref2.copy()
        mod2[1, 0] += shift
        assert lr.evaluate(mod2, ref2, res2, dtype)["atom_preserved"].tolist() == [want, want]
    # a reference distance of exactly 15 is not included; the next float below is
    for far, total in ((15.0, 0), (np.nextafter(np.float32(15.0), np.float32(0.0)), 1)):
        ref2, res2 = line([0.0, far], [0, 1])
        got = lr.evaluate(ref2, ref2, res2, dtype)
        assert got["atom_total"].tolist() == [total, total] and (np.isnan(got["score"]) if total == 0 else got["score"] == 1.0)
    # one residue: no pair at all
    one = lr.evaluate(*(line([0.0, 1.0, 2.0], [0, 0, 0])[0],) * 2, np.zeros(3, dtype=int), dtype)
    assert one["atom_total"].tolist() == [0, 0, 0] and np.isnan(one["residue"]).all() and np.isnan(one["score"])
    # seq_sep = 2 takes the neighbours' pairs away and only those
    ref4, res4 = line([0.0, 1.0, 2.0, 3.0], [0, 1, 2, 3])
    assert lr.evaluate(ref4, ref4, res4, dtype)["atom_total"].tolist() == [3, 3, 3, 3]
    assert lr.evaluate(ref4, ref4, res4, dtype, seq_sep=2)["atom_total"].tolist() == [2, 1, 1, 2]


@pytest.mark.parametrize("n,sigma", lr.CASES)
def test_the_sandwich_leaves_few_decisions_open_and_holds_the_restatement(n, sigma):
    """The cap is a condition on the test cases, asserted on the reference alone: at most CAP of the (T + 1) * sum(total)
    decisions lie between the bounds.  The float32 restatement lies between them everywhere."""
    top, xyz = lr.chain(n)
    model = lr.noisy(xyz, sigma, seed=n)[0]
    res = lr.residues(top)
    lo, hi, share = lr.sandwich(model, xyz, res)
    assert share <= lr.CAP, share
    t32, k32 = lr.counts(model, xyz, res, np.float32)
    t64, k64 = lr.counts(model, xyz, res, np.float64)
    assert (lo[0] <= t32).all() and (t32 <= hi[0]).all() and (lo[1] <= k32).all() and (k32 <= hi[1]).all()
    assert (lo[0] <= t64).all() and (t64 <= hi[0]).all() and (lo[1] <= k64).all() and (k64 <= hi[1]).all()
    print(f"n={n} sigma={sigma}: undecided share {share:.1e}; float32 differs from float64 in "
          f"{int((t32 != t64).sum() + (k32 != k64).sum())} of {5 * t64.shape[0]} counts, sum(total) {int(t64.sum())}")


def test_symmetry_table_against_the_templates():
    """Every named atom exists in the template of its residue type; the package's table and the reference's name the same
    exchanges; lddt_symmetry is an involution within residues and moves exactly the named atoms."""
    names = sorted(metrics.LDDT_SYMMETRIC)
    assert names == sorted(lr.FLIPS) == ["ARG", "ASP", "GLU", "LEU", "PHE", "TYR", "VAL"]
    top = template_topology(sr.RES22)
    for r, nm in enumerate(top.res_names):
        pairs = metrics.LDDT_SYMMETRIC.get(nm, ())
        assert {frozenset(p) for p in pairs} == {frozenset(p.split("=")) for p in lr.FLIPS.get(nm, "").split()}
        for a, b in pairs:
            assert top.atom(r, a) >= 0 and top.atom(r, b) >= 0, (nm, a, b)
    partner = metrics.lddt_symmetry(top)
    assert partner is metrics.lddt_symmetry(top) and partner.dtype == np.int32
    assert (partner[partner] == np.arange(top.n_atoms)).all() and (top.residue_of_atom[partner] == top.residue_of_atom).all()
    moved = {(int(top.residue_of_atom[a]), str(top.name[a])) for a in np.nonzero(partner != np.arange(top.n_atoms))[0]}
    assert moved == {(r, a) for r, nm in enumerate(top.res_names) for p in metrics.LDDT_SYMMETRIC.get(nm, ()) for a in p}
    ref_pairs = {frozenset(p) for pairs in lr.flips(top).values() for p in pairs}
    assert ref_pairs == {frozenset((a, int(partner[a]))) for a in np.nonzero(partner != np.arange(top.n_atoms))[0]}
    # a residue that lacks a named atom is not symmetric
    short = template_topology(["PHE", "ASP"])
    short.atom_names[0].remove("CE2")
    cut = type(short)(short.res_names, short.atom_names)
    p2 = metrics.lddt_symmetry(cut)
    assert (p2[:cut.first_atom[1]] == np.arange(cut.first_atom[1])).all() and (p2 != np.arange(cut.n_atoms)).sum() == 2


def test_position_tables_and_unselected_symmetric_atoms():
    top = template_topology(["PHE", "GLY", "ASP"])
    partner = metrics.lddt_symmetry(top)
    tab = ml._tables(top.first_atom, top.n_atoms, None, partner)
    assert tab["res"].tolist() == top.residue_of_atom.tolist() and tab["res_ptr"].tolist() == top.first_atom.tolist()
    assert tab["partner"].tolist() == partner.tolist() and tab["moved"].shape[0] == 6
    # reversed selection without PHE's CE1: PHE is not symmetric any more, ASP still is
    sel = [a for a in range(top.n_atoms - 1, -1, -1) if a != top.atom(0, "CE1")]
    tab = ml._tables(top.first_atom, top.n_atoms, sel, partner)
    m = len(sel)
    assert tab["res"].tolist() == [int(top.residue_of_atom[a]) for a in sel]
    assert sorted(tab["res_pos"].tolist()) == list(range(m)) and (np.diff(tab["res"][tab["res_pos"]]) >= 0).all()
    assert tab["res_ptr"].tolist() == [0, top.first_atom[1] - 1, top.first_atom[2] - 1, m]
    moved = {sel[p] for p in tab["moved"]}
    assert moved == {top.atom(2, "OD1"), top.atom(2, "OD2")}
    assert sel[tab["partner"][sel.index(top.atom(2, "OD1"))]] == top.atom(2, "OD2")
    for bad, msg in (((sel + sel[:1]), "twice"),):
        with pytest.raises(ValueError, match=msg):
            ml._tables(top.first_atom, top.n_atoms, bad, partner)
    with pytest.raises(ValueError, match="res_ptr must rise from 0 to n_atoms"):
        ml._tables([0, 3], top.n_atoms, None, None)
    wrong = partner.copy()
    wrong[0] = top.n_atoms - 1
    with pytest.raises(ValueError, match="in pairs within a residue"):
        ml._tables(top.first_atom, top.n_atoms, None, wrong)


def test_ref_index_defaults_and_refusals():
    assert metrics.lddt_ref_index(3, 3).tolist() == [0, 1, 2] and metrics.lddt_ref_index(4, 1).tolist() == [0, 0, 0, 0]
    assert metrics.lddt_ref_index(3, 2, (1, 0, 1)).tolist() == [1, 0, 1]
    assert metrics.lddt_ref_index(2, 5, torch.tensor([4, 0])).dtype == np.int32
    with pytest.raises(ValueError, match="need a ref_index"):
        metrics.lddt_ref_index(3, 2)
    for bad in ((0, 2, 1), (0, -1, 1)):
        with pytest.raises(ValueError, match=r"ref_index has an entry outside \[0, 2\)"):
            metrics.lddt_ref_index(3, 2, bad)
    with pytest.raises(ValueError, match="2 entries for 3 structures"):
        metrics.lddt_ref_index(3, 2, (0, 1))


def test_refusals_that_need_no_device():
    top = template_topology(["ALA", "GLY"])
    x = torch.zeros(1, top.n_atoms, 3)
    with pytest.raises(ValueError, match="1 .. 8 thresholds .CODLAD_LDDT_MAX_THRESHOLDS."):
        metrics.lddt(x, x, top, thresholds=[0.5] * 9)
    with pytest.raises(ValueError, match="1 .. 8 thresholds"):
        metrics.lddt(x, x, top, thresholds=[])
    for bad in ([0.5, -1.0], [0.0], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="thresholds must be positive finite numbers"):
            metrics.lddt(x, x, top, thresholds=bad)
    for bad in (-15.0, 0.0, float("inf")):
        with pytest.raises(ValueError, match="cutoff must be positive finite numbers"):
            metrics.lddt(x, x, top, cutoff=bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="seq_sep must be an integer >= 1"):
            metrics.lddt_lists(x, x, [0, 5, 9], seq_sep=bad)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.lddt(x, x, top)
    with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
        metrics.lddt_lists(x, x, [0, 5, 9])


def test_binding_header_and_build_agree():
    from codlad_amd import build
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    assert "codlad_lddt" in _lib.exported_symbols() and hasattr(_lib.lib(), "codlad_lddt")
    assert f"#define CODLAD_LDDT_MAX_THRESHOLDS {_lib.LDDT_MAX_THRESHOLDS}\n" in header
    assert f"#define CODLAD_LDDT_MAX_ATOMS {_lib.LDDT_MAX_ATOMS}\n" in header
    n = _lib.LDDT_MAX_ATOMS
    assert n * n < 2 ** 31 <= (n + 1) ** 2                           # m (m - 1) < m^2: every residue sum fits an int32
    assert "lddt_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["lddt_kernels.hip"] == ["-ffp-contract=off"]
    assert set(ml.__all__) <= set(dir(metrics))
