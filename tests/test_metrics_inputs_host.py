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
NO_COUNT = ("pairwise_rmsd", "radius_of_gyration", "contact_map", "rmsd_matrix", "rmsd_neighbours", "cluster", "mean_structure",
            "rmsf", "covariance", "pca", "distance_histogram")


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
        # the eight newer modules (reweight takes no structures; the *_lists forms of saxs need form-factor tables)
        "saxs_profile": lambda x, ref: m.saxs_profile(x, top),
        "saxs_partials": lambda x, ref: m.saxs_partials(x, top),
        "pair_histogram": lambda x, ref: m.pair_histogram(x, top),
        "pair_histogram_lists": lambda x, ref: m.pair_histogram_lists(x, [0] * top.n_atoms, 1),
        "pair_distribution": lambda x, ref: m.pair_distribution(x, top),
        "saxs_profile_hist": lambda x, ref: m.saxs_profile_hist(x, top),
        "rmsd_matrix": lambda x, ref: m.rmsd_matrix(x),
        "rmsd_neighbours": lambda x, ref: m.rmsd_neighbours(x, 1.0),
        "cluster": lambda x, ref: m.cluster(x, 1.0),
        "mean_structure": lambda x, ref: m.mean_structure(x),
        "rmsf": lambda x, ref: m.rmsf(x),
        "covariance": lambda x, ref: m.covariance(x),
        "pca": lambda x, ref: m.pca(x, n_components=2),
        "pca_project": lambda x, ref: m.pca_project(x, dict(mean=ref[0].double(), components=ref[:1].double())),
        "distance_histogram": lambda x, ref: m.distance_histogram(x),
        "ensemble_compare": lambda x, ref: m.ensemble_compare(x, ref),
        "lddt": lambda x, ref: m.lddt(x, ref, top),
        "lddt_lists": lambda x, ref: m.lddt_lists(x, ref, [0, top.n_atoms]),
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
    assert len(calls) == 35
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call(x, x)
    assert "_sasa_tables" not in top.__dict__ and "_stereo_tables" not in top.__dict__       # refused before any table


def test_the_selection_is_one_object_with_its_two_errors():
    from codlad_amd.metrics import ensemble
    assert ensemble._selection is _inputs.selection and metrics._selection is _inputs.selection
    assert _inputs.selection(None, 5, "cpu") == (None, 0)
    sel, n_sel = _inputs.selection([3, 0], 5, "cpu")
    assert sel.dtype == torch.int32 and sel.tolist() == [3, 0] and n_sel == 2
    with pytest.raises(ValueError, match=r"^sel is empty$"):
        _inputs.selection([], 5, "cpu")
    for bad in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError, match=r"^sel has an index outside \[0, 5\)$"):
            _inputs.selection(bad, 5, "cpu")


# the callers of _inputs.pool: (what, the limit each passes)
POOLS = (("pca", "PCA_MAX_N"), ("mean_structure", "PCA_MAX_N"), ("pca_project", "PCA_MAX_N"), ("rmsd_matrix", "CLUSTER_MAX_N"),
         ("cluster", "CLUSTER_MAX_N"), ("distance_histogram", "COMPARE_MAX_ROWS"), ("ensemble_compare", "COMPARE_MAX_ROWS"))


@pytest.mark.parametrize("what,limit", POOLS)
def test_pool_refuses_a_cpu_tensor_then_too_many_structures(what, limit, monkeypatch):
    max_n = getattr(metrics, limit)
    assert max_n == {"PCA_MAX_N": 65536, "CLUSTER_MAX_N": 65536, "COMPARE_MAX_ROWS": 1048576}[limit]
    big = torch.zeros(1, 4, 3).expand(max_n + 1, 4, 3)                          # zero stride: 48 bytes
    # as it stands the CUDA refusal comes first, for a pool of any size
    with pytest.raises(RuntimeError, match=f"^{what}: x must be a CUDA tensor"):
        _inputs.pool(big, None, what, max_n)
    # past it, the size refusal comes before the selection's
    monkeypatch.setattr(_inputs, "need_cuda", lambda t, w: None)
    monkeypatch.setattr(_inputs, "structures", lambda x, w, n_atoms=None, dims=3: x)     # (no copy of 10^6 structures)
    with pytest.raises(ValueError, match=f"^{what}: at most {max_n} structures in one pool, got {max_n + 1}$"):
        _inputs.pool(big, [], what, max_n)
    with pytest.raises(ValueError, match="^sel is empty$"):
        _inputs.pool(big[:max_n], [], what, max_n)
    x, sel, n_sel = _inputs.pool(big[:2], [1, 2], what, max_n)
    assert x.shape == (2, 4, 3) and sel.tolist() == [1, 2] and n_sel == 2


def test_the_modules_pass_their_own_limit_to_pool(monkeypatch):
    """Each caller's limit and prefix reach pool: the over-size message through the public entry points."""
    monkeypatch.setattr(_inputs, "need_cuda", lambda t, w: None)
    monkeypatch.setattr(_inputs, "structures", lambda x, w, n_atoms=None, dims=3: x)
    one = torch.zeros(1, 4, 3)
    for call, what, max_n in ((lambda x: metrics.mean_structure(x), "mean_structure", metrics.PCA_MAX_N),
                              (lambda x: metrics.pca(x), "pca", metrics.PCA_MAX_N),
                              (lambda x: metrics.rmsd_matrix(x), "rmsd_matrix", metrics.CLUSTER_MAX_N),
                              (lambda x: metrics.cluster(x, 1.0), "cluster", metrics.CLUSTER_MAX_N),
                              (lambda x: metrics.distance_histogram(x), "distance_histogram", metrics.COMPARE_MAX_ROWS)):
        with pytest.raises(ValueError, match=f"^{what}: at most {max_n} structures in one pool, got {max_n + 1}$"):
            call(one.expand(max_n + 1, 4, 3))
    # compare's own check of the selected atoms stays on top of the shared one
    with pytest.raises(ValueError, match="^distance_histogram: 2 .. 2048 selected atoms, got 1$"):
        metrics.distance_histogram(one, sel=[0])


@pytest.mark.parametrize("what", ("pca", "rmsd_neighbours", "cluster", "distance_histogram", "ensemble_compare"))
def test_positive_and_count_messages(what):
    assert _inputs.positive(2, "tol", what) == 2.0 and _inputs.positive("0.5", "tol", what) == 0.5
    assert _inputs.positive(True, "tol", what) == 1.0                           # float(True): a bool is the number it is
    for bad in (0, -1.0, float("nan"), float("inf"), None, "x", [1.0], False):
        with pytest.raises(ValueError) as e:
            _inputs.positive(bad, "cutoff", what)
        assert str(e.value) == f"{what}: cutoff must be a positive finite number, got {bad!r}"
    assert _inputs.count(1, "max_iter", 7, what) == 1 and _inputs.count(7, "max_iter", 7, what) == 7
    import numpy as np
    for bad in (0, 8, True, False, 2.0, float("nan"), None, "3", np.int64(3)):
        with pytest.raises(ValueError) as e:
            _inputs.count(bad, "max_iter", 7, what)
        assert str(e.value) == f"{what}: max_iter must be an integer in 1 .. 7, got {bad!r}"
    # numpy integers only where the caller says so (compare's bin counts), and never a bool
    got = _inputs.count(np.int64(3), "n_bins", 7, what, types=(int, np.integer))
    assert got == 3 and type(got) is int
    for bad in (True, np.bool_(True), np.int64(8), np.float64(3.0)):
        with pytest.raises(ValueError, match=f"^{what}: n_bins must be an integer in 1 .. 7, got "):
            _inputs.count(bad, "n_bins", 7, what, types=(int, np.integer))


def test_each_module_keeps_its_own_acceptance_of_counts(monkeypatch):
    import numpy as np
    from codlad_amd.metrics import compare
    assert compare._n_bins(np.int32(5), "distance_histogram") == 5
    with pytest.raises(ValueError, match="^column_histogram: rg_bins must be an integer in 1 .. 256, got 257$"):
        compare._n_bins(257, "column_histogram", "rg_bins")
    with pytest.raises(ValueError, match="^ensemble_compare: n_bins must be an integer in 1 .. 256, got True$"):
        compare._n_bins(True, "ensemble_compare")
    monkeypatch.setattr(_inputs, "need_cuda", lambda t, w: None)
    x = torch.zeros(3, 4, 3)
    with pytest.raises(ValueError) as e:
        metrics.pca(x, n_components=2, max_iter=np.int64(5))                    # pca takes no numpy integer
    assert str(e.value) == f"pca: max_iter must be an integer in 1 .. {metrics._lib.PCA_MAX_ITER}, got {np.int64(5)!r}"
    with pytest.raises(ValueError, match="^rmsd_neighbours: cutoff must be a positive finite number, got nan$"):
        metrics.rmsd_neighbours(x, float("nan"))                                # the cut-off is refused before the pool


@pytest.mark.parametrize("what", ("pca", "rmsf", "cluster"))
def test_weights_in_both_modes(what):
    for need_positive in (True, False):
        w = _inputs.weights([0, 2, 0.5], 3, "cpu", what, need_positive)
        assert w.dtype == torch.float64 and w.tolist() == [0.0, 2.0, 0.5]
        with pytest.raises(ValueError, match=f"^{what}: weights must have one value per structure \\(3\\), got 2$"):
            _inputs.weights([1, 1], 3, "cpu", what, need_positive)
        for bad in ([1, -1, 1], [1, float("nan"), 1], [1, float("inf"), 1]):
            with pytest.raises(ValueError, match=f"^{what}: weights must be finite and >= 0$"):
                _inputs.weights(bad, 3, "cpu", what, need_positive)
    # pca's mode: None is "no weights", and one weight at least is positive; cluster's: all zero passes
    assert _inputs.weights(None, 3, "cpu", what, True) is None
    with pytest.raises(ValueError, match=f"^{what}: every weight is 0$"):
        _inputs.weights([0, 0, 0], 3, "cpu", what, True)
    assert _inputs.weights([0, 0, 0], 3, "cpu", what, False).tolist() == [0.0, 0.0, 0.0]


def test_flags_hold_two_elements_or_more():
    for N in (1, 2, 5):
        f = _inputs.flags(N, "cpu")
        assert f.dtype == torch.uint8 and f.shape == (N,) and f.untyped_storage().nbytes() == max(N, 2)


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
