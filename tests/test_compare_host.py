"""CPU checks of the ensemble-comparison feature: the C ABI of codlad_dist_hist, codlad_column_hist and
codlad_hist_divergence (declared once, exported, counted in _SIGS, bad arguments refused before any HIP call, the table
sizes), the kernels' registers, what the Python layer and the CLI refuse, and the references of tests/compare_ref.py
against answers derived by hand."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import compare_ref as cr
from tests.test_cluster_host import _FakeCuda
from tests.cli_script import load_cli, option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("codlad_dist_hist_bytes", "long long", 2), ("codlad_column_hist_bytes", "long long", 2),
                ("codlad_dist_hist", "int", 11), ("codlad_column_hist", "int", 10), ("codlad_hist_divergence", "int", 8))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, ret, n_args in ENTRY_POINTS:
        decl = re.findall(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
        assert not name.startswith(("codlad_pca_", "codlad_ens_", "codlad_stereo_"))
    for macro, value, mine in (("COMPARE_MAX_ROWS", 1048576, _lib.COMPARE_MAX_ROWS), ("COMPARE_MAX_BINS", 256, _lib.COMPARE_MAX_BINS),
                               ("DIST_HIST_MAX_SEL", 2048, _lib.DIST_HIST_MAX_SEL),
                               ("DIVERGENCE_MAX_COLS", 4098, _lib.DIVERGENCE_MAX_COLS)):
        assert f"#define CODLAD_{macro} {value}\n" in header and mine == value == getattr(metrics, macro)
    assert (cr.MAX_ROWS, cr.MAX_BINS, cr.MAX_SEL, cr.MAX_COLS) == (1048576, 256, 2048, 4098)
    assert "#define CODLAD_DIST_HIST_PAIR(i, j, m) ((i) * (m) - (i) * ((i) + 1) / 2 + ((j) - (i) - 1))\n" in header
    for name, expr in (("JS", "(4.0 * (cols) + 8.0)"), ("TV", "((cols) + 2.0)"), ("W1", "(2.0 * (cols) * (cols) + 2.0 * (cols))")):
        assert f"#define CODLAD_DIVERGENCE_{name}_BOUND(cols) ({expr} * 2.220446049250313e-16)\n" in header
    assert cr.EPS == 2.220446049250313e-16 and cr.bounds(52) == ((4 * 52 + 8) * cr.EPS, 54 * cr.EPS, (2 * 52 * 52 + 104) * cr.EPS)
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "compare_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["compare_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("distance_histogram", "column_histogram", "histogram_divergence", "pair_matrix", "ensemble_compare"):
        assert callable(getattr(metrics, name))


def test_compare_kernels_use_no_scratch_and_spill_nothing():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "compare_kernels.hip"}
    for kernel in ("compare_fill_kernel", "compare_finite_kernel", "dist_hist_kernel", "column_hist_kernel", "hist_divergence_kernel"):
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    assert len(mine) == 5, sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced
    p = buf.ctypes.data
    nan, inf = float("nan"), float("inf")

    def refuses(fn, ok, cases):
        for k, bad in cases:
            args = list(ok)
            args[k] = bad
            assert getattr(lib, fn)(*args) < 0, (fn, k, bad)
            assert fn.encode() in lib.codlad_last_error(), (fn, k, bad)

    for fn, bads in (("codlad_dist_hist_bytes", ((1, 50), (0, 50), (-1, 50), (2049, 50), (5, 0), (5, 257), (5, -1), (2048, 256 * 4))),
                     ("codlad_column_hist_bytes", ((0, 50), (-1, 50), (1048577, 50), (5, 0), (5, 257)))):
        for bad in bads:
            assert getattr(lib, fn)(*bad) < 0 and fn.encode() in lib.codlad_last_error(), (fn, bad)
    # the table H a caller allocates: int32 [P][n_bins + 2] and [C][n_bins + 2]
    assert lib.codlad_dist_hist_bytes(2, 1) == 4 * 1 * 3
    assert lib.codlad_dist_hist_bytes(505, 50) == 4 * 127260 * 52
    assert lib.codlad_dist_hist_bytes(2048, 256) == 4 * 2096128 * 258
    assert lib.codlad_column_hist_bytes(1, 1) == 4 * 3
    assert lib.codlad_column_hist_bytes(903, 36) == 4 * 903 * 38
    assert lib.codlad_column_hist_bytes(1048576, 256) == 4 * 1048576 * 258
    #     x  N  n_atoms sel n_sel inv_dr n_bins H finite n_counted stream
    ok = [p, 4, 5, None, 0, 2.0, 50, p, p, p, None]
    refuses("codlad_dist_hist", ok, [(k, None) for k in (0, 7, 8, 9)] +
            [(1, 0), (1, -1), (1, 1048577), (2, 0), (2, 1), (2, 2049), (4, 3), (4, -1), (5, 0.0), (5, -1.0), (5, nan), (5, inf),
             (6, 0), (6, -1), (6, 257)])
    args = list(ok)
    args[3] = p                                          # sel without n_sel
    assert lib.codlad_dist_hist(*args) < 0 and b"disagree" in lib.codlad_last_error()
    args[4] = 1                                          # one selected atom has no pair
    assert lib.codlad_dist_hist(*args) < 0 and b"codlad_dist_hist" in lib.codlad_last_error()
    args[4] = 2049
    assert lib.codlad_dist_hist(*args) < 0 and b"codlad_dist_hist" in lib.codlad_last_error()
    #     values N  C  lo    inv_width n_bins periodic H n_valid stream
    ok = [p, 4, 7, -180.0, 0.1, 36, 1, p, p, None]
    refuses("codlad_column_hist", ok, [(k, None) for k in (0, 7, 8)] +
            [(1, 0), (1, -1), (1, 1048577), (2, 0), (2, 1048577), (3, nan), (3, inf), (3, -inf), (4, 0.0), (4, -1.0), (4, nan),
             (4, inf), (5, 0), (5, 257), (6, 2), (6, -1)])
    #     HA HB rows cols js tv w1 stream
    ok = [p, p, 3, 52, p, p, p, None]
    refuses("codlad_hist_divergence", ok, [(k, None) for k in (0, 1, 4, 5, 6)] +
            [(2, 0), (2, -1), (2, (1 << 31) // 52 + 1), (3, 1), (3, 0), (3, 4099), (3, -1)])


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 5, 3)
    cnt = torch.zeros(3, 5, dtype=torch.int32)
    for call in (lambda: metrics.distance_histogram(x), lambda: metrics.column_histogram(torch.zeros(4, 2), 0.0, 1.0, 5),
                 lambda: metrics.histogram_divergence(cnt, cnt), lambda: metrics.ensemble_compare(x, x)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    F = _FakeCuda(x)
    for call in (metrics.distance_histogram, lambda a, **k: metrics.ensemble_compare(a, a, **k)):
        with pytest.raises(ValueError, match="non-empty"):
            call(_FakeCuda(torch.zeros(4, 5)))
        with pytest.raises(ValueError, match="outside"):
            call(F, sel=[0, 5])
        with pytest.raises(ValueError, match="sel is empty"):
            call(F, sel=[])
        with pytest.raises(ValueError, match="2 .. 2048 selected atoms, got 1"):
            call(F, sel=[3])
        with pytest.raises(ValueError, match="2 .. 2048 selected atoms, got 2049"):
            call(_FakeCuda(torch.zeros(2, 2049, 3)))
        with pytest.raises(ValueError, match="2 .. 2048 selected atoms, got 1"):
            call(_FakeCuda(torch.zeros(2, 1, 3)))
        for bad in (0, -1, 257, 2.0, None, True):
            with pytest.raises(ValueError, match="n_bins must be an integer in 1 .. 256"):
                call(F, n_bins=bad, r_max=10.0)
        for bad in (0.0, -1.0, float("nan"), float("inf"), "wide"):
            with pytest.raises(ValueError, match="r_max must be a positive finite number"):
                call(F, r_max=bad)
    with pytest.raises(ValueError, match="at most 1048576 structures"):
        metrics.distance_histogram(_FakeCuda(torch.zeros(1048577, 2, 3)), r_max=5.0)
    for bad in (0.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="dr must be a positive finite number"):
            metrics.distance_histogram(F, dr=bad)
    with pytest.raises(ValueError, match="at most 256 bins"):
        metrics.distance_histogram(F, dr=0.1, r_max=30.0)
    with pytest.raises(ValueError, match="have 5 and 6 atoms"):
        metrics.ensemble_compare(F, _FakeCuda(torch.zeros(4, 6, 3)))
    for name in ("torsion_bins", "rg_bins"):
        with pytest.raises(ValueError, match=f"{name} must be an integer in 1 .. 256"):
            metrics.ensemble_compare(F, F, r_max=5.0, **{name: 0})
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="min_separation must be a positive integer"):
            metrics.ensemble_compare(F, F, r_max=5.0, min_separation=bad)
    V = _FakeCuda(torch.zeros(4, 2))
    for lo, hi in ((0.0, 0.0), (1.0, 0.0), (float("nan"), 1.0), (0.0, float("inf")), ("a", 1.0)):
        with pytest.raises(ValueError, match="lo and hi must be finite numbers with lo < hi"):
            metrics.column_histogram(V, lo, hi, 5)
    for bad in (0, 257, 1.0):
        with pytest.raises(ValueError, match="n_bins must be an integer in 1 .. 256"):
            metrics.column_histogram(V, 0.0, 1.0, bad)
    with pytest.raises(ValueError, match="non-empty"):
        metrics.column_histogram(_FakeCuda(torch.zeros(4, 2, 2)), 0.0, 1.0, 5)
    K = _FakeCuda(cnt)
    with pytest.raises(ValueError, match="one shape"):
        metrics.histogram_divergence(K, _FakeCuda(torch.zeros(3, 6, dtype=torch.int32)))
    with pytest.raises(ValueError, match="integer counts"):
        metrics.histogram_divergence(_FakeCuda(torch.zeros(3, 5)), _FakeCuda(torch.zeros(3, 5)))
    for cols in (1, 4099):
        with pytest.raises(ValueError, match="2 .. 4098 columns"):
            metrics.histogram_divergence(_FakeCuda(torch.zeros(2, cols, dtype=torch.int32)), _FakeCuda(torch.zeros(2, cols, dtype=torch.int32)))
    with pytest.raises(ValueError, match="3 atoms have 3 pairs"):
        metrics.pair_matrix(torch.zeros(4), 3)
    M = metrics.pair_matrix(torch.tensor([1.0, 2.0, 3.0]), 3)
    assert M.tolist() == [[0.0, 1.0, 2.0], [1.0, 0.0, 3.0], [2.0, 3.0, 0.0]]


def test_cli_refuses_what_compare_cannot_run():
    cli = load_cli("codlad_cli")
    a = argparse.Namespace(compare=None, compare_cluster=None, experiment="latent")
    assert cli.check_compare(a) == 0 and a.compare == 0
    assert cli.check_compare(argparse.Namespace(compare=20, compare_cluster=None, experiment="latent")) == 20
    assert cli.check_compare(argparse.Namespace(compare=50, compare_cluster=2.5, experiment="recon")) == 50
    for bad in (0, -1, 257):
        with pytest.raises(SystemExit, match="--compare takes the number of distance bins, 1 .. 256"):
            cli.check_compare(argparse.Namespace(compare=bad, compare_cluster=None, experiment="latent"))
    for exp in ("bpd", "fmloss"):
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_compare(argparse.Namespace(compare=20, compare_cluster=None, experiment=exp))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SystemExit, match="--compare_cluster takes an RMSD cut-off in A"):
            cli.check_compare(argparse.Namespace(compare=20, compare_cluster=bad, experiment="latent"))
    with pytest.raises(SystemExit, match="--compare_cluster needs --compare"):
        cli.check_compare(argparse.Namespace(compare=None, compare_cluster=2.0, experiment="latent"))
    with pytest.raises(SystemExit, match="has no true frames"):
        cli.compare_truth("p", {"x": 1})
    flag, cut = option(cli, "--compare"), option(cli, "--compare_cluster")
    assert flag.type is int and flag.nargs == "?" and flag.const == 50 and flag.default is None
    assert cut.type is float and cut.nargs is None and cut.default is None
    parse = cli.build_parser().parse_args
    assert parse(["--compare"]).compare == 50 and parse([]).compare is None
    assert parse(["--compare", "20", "--compare_cluster", "2.5"]).compare_cluster == 2.5


def test_reference_divergences_by_hand():
    js, tv, w1 = cr.divergence_ref([[1, 0]], [[0, 1]])
    assert js[0] == 1.0 and tv[0] == 1.0 and w1[0] == 1.0
    js, tv, w1 = cr.divergence_ref([[7, 7]], [[0, 5]])                # p = (1/2, 1/2), q = (0, 1)
    assert abs(js[0] - cr.HAND_JS) <= cr.bounds(2)[0] and abs(cr.HAND_JS - 0.31127812445913283) < 1e-15
    assert tv[0] == 0.5 and w1[0] == 0.5
    js, tv, w1 = cr.divergence_ref([[3, 1, 0, 6], [1, 1, 1, 1]], [[21, 7, 0, 42], [5, 5, 5, 5]])      # equal proportions
    assert (js == 0.0).all() and (tv == 0.0).all() and (w1 == 0.0).all()
    for k in (1, 3, 17):                                              # two point masses k columns apart
        a, b = np.zeros((1, 20), dtype=np.int64), np.zeros((1, 20), dtype=np.int64)
        a[0, 1], b[0, 1 + k] = 9, 4
        js, tv, w1 = cr.divergence_ref(a, b)
        assert w1[0] == float(k) and js[0] == 1.0 and tv[0] == 1.0
    js, tv, w1 = cr.divergence_ref([[0, 0], [1, -1], [2, 2]], [[1, 1], [1, 1], [0, 0]])
    assert np.isnan(js).all() and np.isnan(tv).all() and np.isnan(w1).all()
    A, B = cr.count_tables(40, 52, 3, sparse=True)
    a, b = cr.divergence_ref(A, B), cr.divergence_ref(B, A)           # the swap: same bits
    ld = cr.divergence_ld(A, B)
    for got, back, want, bound in zip(a, b, ld, cr.bounds(52)):
        assert (got.view(np.int64) == back.view(np.int64)).all()
        assert float(np.abs(got.astype(np.longdouble) - want).max()) <= bound


def test_pair_index_round_trips_and_the_histogram_references_agree():
    for m in (2, 3, 17):
        i, j = cr.pairs(m)
        tab = metrics.pair_table(m)
        assert tab.shape == (m * (m - 1) // 2, 2) and (tab[:, 0] == i).all() and (tab[:, 1] == j).all()
        for p, (a, b) in enumerate(tab.tolist()):
            assert a < b and cr.pair_index(a, b, m) == p == metrics.pair_index(a, b, m)
    # the closed form of the lattice is what the float32 restatement gives, edge for edge
    for dr, n_bins in ((0.5, 50), (1.0, 20), (2.0, 256)):
        x = cr.lattice_pool(7, 17)
        H, fin, n = cr.hist32(x, None, np.float32(1.0 / dr), n_bins)
        assert fin.all() and n == 7 and (H == cr.lattice_hist(7, 17, dr, n_bins)).all() and (H.sum(1) == 7).all()
    # a structure that is not finite among its selected atoms takes no part; an unselected NaN changes nothing
    c = cr.pool(63, 15, "sel")
    x = c["x"].copy()
    unsel = [a for a in range(x.shape[1]) if a not in set(c["sel"].tolist())]
    x[5, unsel[0], 1] = np.nan
    H0, _f, _n = cr.hist32(c["x"], c["sel"], 2.0, 50)
    H1, f1, n1 = cr.hist32(x, c["sel"], 2.0, 50)
    assert (H0 == H1).all() and f1.all() and n1 == 63
    x[9, c["sel"][2], 0] = np.inf
    H2, f2, n2 = cr.hist32(x, c["sel"], 2.0, 50)
    assert not f2[9] and f2.sum() == 62 == n2 and (H2.sum(1) == 62).all() and (H2[:, 0] == 0).all()
    # the float64 decision of a column: edges, both ends, the wrap of a torsion
    v = np.array([[-180.0], [180.0], [179.999], [-170.0], [0.0], [np.nan], [np.inf], [540.0], [-190.0]])
    H, n = cr.column_hist_ref(v, -180.0, 36 / 360.0, 36, True)
    assert n[0] == 7 and H[0, 0] == 0 and H[0, -1] == 0 and H[0, 1] == 3 and H[0, 36] == 2 and H[0, 2] == 1 and H[0, 19] == 1
    H, n = cr.column_hist_ref(v, -180.0, 36 / 360.0, 36, False)
    assert n[0] == 7 and H[0, 0] == 1 and H[0, -1] == 2 and H[0, 1] == 1 and H[0, 36] == 1
    assert {k[0] for k in cr.SHAPES} == {1, 2, 63, 64, 65, 300} and {k[1] for k in cr.SHAPES} == {2, 3, 15, 16, 17, 33, 129}
    assert {k[2] for k in cr.SHAPES} >= {1, 50, 255, 256} and cr.LIMITS == ((2, 2048, 1, 64.0), (65, 3, 256, 0.125))
