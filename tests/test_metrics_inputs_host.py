"""CPU checks of what the structure-analysis entry points of codlad_amd/metrics/ share (metrics/_inputs.py): the package
keeps every public name the single-file module had, every entry point that takes structures refuses a CPU tensor, the
geometry check and the relaxation read ONE set of template tables per topology, and the bond-graph tables are what they
were - tests/golden/bond_graph_tables.json holds the outputs of the functions as they stood before the split, on seeded
random bond graphs of 2 .. 12 atoms (the inputs are in the file)."""
import json
import os

import pytest
import torch

from codlad_amd import metrics
from codlad_amd.metrics import _inputs
from codlad_amd.utils import dataset_builder
from codlad_amd.utils.cg_input import template_topology

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every name without a leading underscore in the namespace of the former codlad_amd/metrics.py (C and torch are its imports)
PUBLIC_NAMES = (
    "C", "CHI_PATH", "COV_CUTOFF", "DSSP_CODES", "DSSP_MAX_RES", "DSSP_NAMES", "GEOMETRY_COUNTS", "NAMES", "RELAX_DEFAULTS",
    "RELAX_ENERGIES", "SASA_MAX_POINTS", "SIDE_CENTRE", "STEREO_COLUMNS", "STEREO_COUNTS", "STEREO_FLAGS", "VDW_RADII",
    "all_results", "bond_graph_counts", "clash_list", "clash_result", "compute_div", "contact_map", "diversity_terms", "dssp",
    "dssp_assign", "dssp_tables", "evaluate", "exclusion_csr", "ged_result", "geometry_check", "geometry_check_lists", "hbonds",
    "inter_result", "pairwise_rmsd", "quad_csr", "radius_of_gyration", "recon_result", "relax", "relax_energy",
    "relax_energy_lists", "relax_lists", "relax_tables", "ring_bonds", "sasa", "sasa_lists", "sphere_points", "ss_propensity",
    "ss_strings", "stereo_check", "stereo_tables", "superpose", "superposed_rmsd", "superposed_rmsd_batch", "torch",
    "torsion_quads", "valid_ratio_and_cut_off_result", "vdw_radii", "xyz_result")
# entry points whose structures are held to no atom count: there is no topology, list or second tensor to differ from
NO_COUNT = ("pairwise_rmsd", "radius_of_gyration", "contact_map")


def topology():
    return template_topology(["ALA", "CYS", "GLY"])


def entry_points(top):
    """name -> f(x, ref) for every entry point that takes structures: x [S, n_atoms, 3] is the batch under test; ref (a
    batch of the topology's atom count) and the lists of the *_lists forms come from the topology."""
    m = metrics
    tab = m.relax_tables(top)
    lists = (tab["radius"], _inputs.template_tables(top, 2)[3], tab["quads"])
    return {
        "superposed_rmsd_batch": lambda x, ref: m.superposed_rmsd_batch(x, ref),
        "superpose": lambda x, ref: m.superpose(x, ref),
        "pairwise_rmsd": lambda x, ref: m.pairwise_rmsd(x[None]),
        "diversity_terms": lambda x, ref: m.diversity_terms(x[None], ref),
        "geometry_check": lambda x, ref: m.geometry_check(x, top),
        "geometry_check_lists": lambda x, ref: m.geometry_check_lists(x, *lists[:2]),
        "stereo_check": lambda x, ref: m.stereo_check(x, top),
        "relax": lambda x, ref: m.relax(x, top, n_iter=1),
        "relax_energy": lambda x, ref: m.relax_energy(x, top),
        "relax_lists": lambda x, ref: m.relax_lists(x, *lists, n_iter=1),
        "relax_energy_lists": lambda x, ref: m.relax_energy_lists(x, *lists),
        "sasa": lambda x, ref: m.sasa(x, top, n_points=96),
        "sasa_lists": lambda x, ref: m.sasa_lists(x, m.vdw_radii(top.element), n_points=96),
        "radius_of_gyration": lambda x, ref: m.radius_of_gyration(x),
        "contact_map": lambda x, ref: m.contact_map(x),
        "hbonds": lambda x, ref: m.hbonds(x, top),
        "dssp": lambda x, ref: m.dssp(x, top),
    }


def test_the_package_keeps_every_public_name():
    missing = [name for name in PUBLIC_NAMES if not hasattr(metrics, name)]
    assert not missing, missing
    from codlad_amd.metrics import COV_CUTOFF                                  # tools/gen_golden.py's import
    assert len(COV_CUTOFF) == 107 and callable(metrics.relax) and callable(metrics.dssp)


def test_every_entry_point_refuses_a_cpu_tensor():
    top = topology()
    x = torch.zeros(2, top.n_atoms, 3)
    calls = entry_points(top)
    assert len(calls) == 17
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call(x, x)
    assert "_sasa_tables" not in top.__dict__ and "_stereo_tables" not in top.__dict__       # refused before any table


def test_geometry_and_relaxation_read_one_set_of_template_tables(monkeypatch):
    top = topology()
    built = []
    real = dataset_builder.standard_bonds
    monkeypatch.setattr(dataset_builder, "standard_bonds", lambda t: built.append("bonds") or real(t))
    # the geometry check's tables at order 2 (what geometry_check uploads) and the relaxation's
    radius, ptr, words, bonds = _inputs.template_tables(top, 2)
    tab = metrics.relax_tables(top, 2)
    assert tab["radius"] is radius and tab["excl_ptr"] is ptr and tab["excl"] is words
    assert tab["pair_ptr"] is ptr and tab["pair_j"] is words
    assert built == ["bonds"] and _inputs.template_tables(top, 2)[3] is bonds                      # one bond list, built once
    assert torch.equal(bonds, real(top))
    for a, b in zip((ptr, words), metrics.exclusion_csr(bonds, 2, top.n_atoms)):
        assert torch.equal(a, b)
    # a second request returns the cached objects
    assert metrics.relax_tables(top, 2) is tab and _inputs.template_tables(top, 2)[2] is words
    # order 3: another exclusion CSR, the same restrained pairs, radii and bonds
    tab3 = metrics.relax_tables(top, 3)
    radius3, ptr3, words3, bonds3 = _inputs.template_tables(top, 3)
    assert radius3 is radius and bonds3 is bonds
    assert tab3["excl"] is words3 and words3 is not words and words3.numel() > words.numel()
    assert tab3["pair_j"] is words and tab3["radius"] is radius and built == ["bonds"]
    assert set(top._relax_tables) == {(2, "host"), (3, "host")}


def test_bond_graph_tables_are_what_they_were():
    with open(os.path.join(ROOT, "tests", "golden", "bond_graph_tables.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 12 and max(c["n_atoms"] for c in cases) == 12
    assert sum(len(c["torsion_quads"]) for c in cases) > 0 and sum(len(c["ring_bonds"]) for c in cases) > 0
    for c in cases:
        n, bonds = c["n_atoms"], c["bonds"]
        for order, (ptr, words) in c["exclusion_csr"].items():
            got = metrics.exclusion_csr(bonds, int(order), n)
            assert got[0].dtype == got[1].dtype == torch.int32 and got[0].tolist() == ptr and got[1].tolist() == words
        assert [list(b) for b in metrics.ring_bonds(bonds, n)] == c["ring_bonds"]
        quads = metrics.torsion_quads(bonds, [tuple(b) for b in c["rigid"]], n)
        assert quads.dtype == torch.int32 and tuple(quads.shape) == (len(c["torsion_quads"]), 4)
        assert quads.tolist() == c["torsion_quads"]
        qp, qr = metrics.quad_csr(quads, n)
        assert qp.dtype == qr.dtype == torch.int32 and [qp.tolist(), qr.tolist()] == c["quad_csr"]
    # exclusion_csr still refuses a self-bond and an index outside the atoms
    for bad in ([(1, 1)], [(0, 3)], [(-1, 2)]):
        with pytest.raises(ValueError, match="not a pair of different atoms"):
            metrics.exclusion_csr(bad, 2, 3)
