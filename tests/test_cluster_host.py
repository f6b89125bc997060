"""CPU checks of the clustering feature: the C ABI of codlad_rmsd_matrix and codlad_cluster_* (declared, exported, bad
arguments refused before any HIP call, no scratch memory in the kernels), what the Python layer and the CLI refuse, and
the references of tests/cluster_ref.py against what they restate: all_pairs against ensemble_ref.kabsch, the Daura loop
against answers derived by hand, and the condition under which the GPU comparison of the bitmaps is exact - no pair of
the planted and continuum cases lies within msd_bound of its cut-off."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import cluster_ref as cr
from tests import ensemble_ref as er
from tests.cli_script import load_cli, option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("codlad_rmsd_matrix_scratch_bytes", "long long", 2), ("codlad_rmsd_matrix", "int", 13),
                ("codlad_cluster_scratch_bytes", "long long", 1), ("codlad_cluster_daura", "int", 10),
                ("codlad_cluster_populations", "int", 6))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, ret, n_args in ENTRY_POINTS:
        decl = re.findall(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value in (("MAX_N", 65536), ("MAX_ROUNDS", 4096), ("STATE_WORDS", 8), ("ST_PHASE", 0), ("ST_ACTIVE", 1),
                         ("ST_CLUSTERS", 2), ("ST_ROUNDS", 3)):
        assert f"#define CODLAD_CLUSTER_{macro} {value}\n" in header and getattr(_lib, f"CLUSTER_{macro}") == value
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "cluster_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["cluster_kernels.hip"] == ["-ffp-contract=off"]
    assert metrics.CLUSTER_MAX_N == 65536
    for name in ("rmsd_matrix", "rmsd_neighbours", "cluster_neighbours", "cluster"):
        assert callable(getattr(metrics, name))


def test_cluster_kernels_use_no_scratch():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "cluster_kernels.hip"}
    for kernel in ("operand_kernel", "matrix_kernel", "init_kernel", "count_kernel", "pick_kernel", "populations_kernel"):
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    matrix = [r for k, r in mine.items() if "matrix_kernel" in k][0]
    assert matrix["VGPRs"] <= 256 and matrix["Occupancy"] >= 2, matrix          # two 8-wave workgroups' worth per SIMD


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced
    p = buf.ctypes.data
    for bad in ((0, 4), (-1, 4), (65537, 4), (4, 0), (4, -1)):
        assert lib.codlad_rmsd_matrix_scratch_bytes(*bad) < 0, bad
        assert b"codlad_rmsd_matrix_scratch_bytes" in lib.codlad_last_error(), bad
    assert lib.codlad_rmsd_matrix_scratch_bytes(1, 1) == 8 * 4 * 3 * 64
    assert lib.codlad_rmsd_matrix_scratch_bytes(65, 65) == 8 * 68 * 3 * 128
    assert lib.codlad_rmsd_matrix_scratch_bytes(65536, 129) == 8 * 132 * 3 * 65536
    #     x  mom N  n_atoms sel n_sel cut2 squared msd bits finite scratch stream
    ok = [p, p, 4, 5, None, 0, 1.0, 0, p, p, p, p, None]
    cases = [(0, None), (1, None), (10, None), (11, None), (2, 0), (2, -1), (2, 65537), (3, 0), (3, -1), (5, -1), (5, 3),
             (6, -1.0), (6, float("nan")), (6, float("inf"))]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_rmsd_matrix(*args) < 0, (k, bad)
        assert b"codlad_rmsd_matrix" in lib.codlad_last_error(), (k, bad)
    args = list(ok)
    args[8] = args[9] = None                             # neither output
    assert lib.codlad_rmsd_matrix(*args) < 0 and b"neither" in lib.codlad_last_error()
    args = list(ok)
    args[4] = p                                          # sel without n_sel
    assert lib.codlad_rmsd_matrix(*args) < 0 and b"disagree" in lib.codlad_last_error()
    for bad in (0, -1, 65537):
        assert lib.codlad_cluster_scratch_bytes(bad) < 0 and b"codlad_cluster_scratch_bytes" in lib.codlad_last_error()
    assert lib.codlad_cluster_scratch_bytes(1) == 20 and lib.codlad_cluster_scratch_bytes(65) == 16 * 2 + 4 * 65
    #     bits finite N rounds state labels centres sizes scratch stream
    ok = [p, None, 4, 64, p, p, p, p, p, None]
    for k, bad in [(0, None), (4, None), (5, None), (6, None), (7, None), (8, None), (2, 0), (2, -1), (2, 65537), (3, -1), (3, 4097)]:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_cluster_daura(*args) < 0, (k, bad)
        assert b"codlad_cluster_daura" in lib.codlad_last_error(), (k, bad)
    #     labels w N K pop stream
    ok = [p, p, 4, 2, p, None]
    for k, bad in [(0, None), (1, None), (4, None), (2, 0), (2, 65537), (3, 0), (3, -1), (3, 5)]:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_cluster_populations(*args) < 0, (k, bad)
        assert b"codlad_cluster_populations" in lib.codlad_last_error(), (k, bad)


class _FakeCuda:
    """A CPU tensor that says it is on the device: what the refusals that precede every launch read (none reaches one)."""
    is_cuda, device = True, "cpu"

    def __init__(self, t):
        self.t, self.shape, self.dtype = t, t.shape, t.dtype

    def dim(self):
        return self.t.dim()

    def numel(self):
        return self.t.numel()

    def detach(self):
        return self

    def to(self, *_a, **_k):
        return self

    def contiguous(self):
        return self


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 5, 3)
    bits = torch.zeros(4, 1, dtype=torch.int64)
    for call in (lambda: metrics.rmsd_matrix(x), lambda: metrics.rmsd_neighbours(x, 1.0), lambda: metrics.cluster(x, 1.0),
                 lambda: metrics.cluster_neighbours(bits, 4)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    F = _FakeCuda(x)
    for bad in (0.0, -1.0, float("nan"), float("inf"), None, "wide"):
        for call in (metrics.rmsd_neighbours, metrics.cluster):
            with pytest.raises(ValueError, match="cutoff must be a positive finite number"):
                call(F, bad)
    big = _FakeCuda(torch.zeros(65537, 1, 3))
    for call in (lambda: metrics.rmsd_matrix(big), lambda: metrics.rmsd_neighbours(big, 1.0), lambda: metrics.cluster(big, 1.0)):
        with pytest.raises(ValueError, match="at most 65536 structures"):
            call()
    with pytest.raises(ValueError, match="non-empty"):
        metrics.rmsd_matrix(_FakeCuda(torch.zeros(4, 5)))
    with pytest.raises(ValueError, match="outside"):
        metrics.rmsd_matrix(F, sel=[0, 5])
    for bad in (torch.zeros(4, 1, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int64), torch.zeros(5, 1, dtype=torch.int64),
                torch.zeros(4, dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"bits must be int64 \[4, 1\]"):
            metrics.cluster_neighbours(_FakeCuda(bad), 4)
    for bad_n in (0, -1, 65537, 4.0):
        with pytest.raises(ValueError, match="n must be an integer"):
            metrics.cluster_neighbours(_FakeCuda(bits), bad_n)
    with pytest.raises(ValueError, match="finite must have one entry"):
        metrics.cluster_neighbours(_FakeCuda(bits), 4, finite=torch.ones(3, dtype=torch.bool))
    for bad, what in ((np.ones(3), "one value per structure"), (np.array([1, -1, 1, 1.0]), "finite and >= 0"),
                      (np.array([1, np.nan, 1, 1.0]), "finite and >= 0"), (np.array([1, np.inf, 1, 1.0]), "finite and >= 0")):
        with pytest.raises(ValueError, match=what):
            metrics.cluster_neighbours(_FakeCuda(bits), 4, weights=bad)
        with pytest.raises(ValueError, match=what):
            metrics.cluster(F, 1.0, weights=bad)


def test_all_pairs_is_kabsch_for_every_pair():
    """The stacked arithmetic against ensemble_ref.kabsch itself: two float64 evaluations of the same formula whose
    covariances are summed in another order, so they differ by at most the bound's own worst case, msd_bound(n, e0 / n)."""
    for x in (cr.pool(17, 65), cr.pool(17, 3), cr.degenerate()):
        msd, e0n = cr.all_pairs(x)
        for i in range(x.shape[0]):
            for j in range(x.shape[0]):
                k = er.kabsch(x[i], x[j])
                lim = er.msd_bound(x.shape[1], k["e0n"])
                assert abs(k["msd"] - msd[i, j]) <= lim and abs(k["e0n"] - e0n[i, j]) <= lim


def test_cases_are_the_shapes_the_issue_names():
    assert cr.POOL_SIZES == (1, 2, 15, 16, 17, 63, 64, 65, 130) and cr.ATOM_COUNTS == (1, 2, 3, 4, 5, 63, 64, 65, 257, 1000)
    assert cr.LARGE == (1025, 5) and len(cr.SHAPES) == 9 + 9 + 1 and len(set(cr.SHAPES)) == 19
    assert cr.PLANTED_CASES == ((130, 65, 5), (65, 4, 3), (17, 257, 2)) and len(cr.SUB_POOL) == 17
    for N, n in cr.SHAPES:
        x = cr.pool(N, n)
        assert x.shape == (N, n, 3) and x.dtype == np.float32 and not x.flags.writeable
    assert cr.continuum().shape == (130, 65, 3) and cr.degenerate().shape == (16, 65, 3)
    far = np.abs(cr.continuum()).max(axis=(1, 2)) > 400
    assert far[1::2].all() and not far[::2].any()                    # every odd member is 1000 A away


def test_no_pair_of_the_separated_cases_is_undecided():
    """The GPU comparison of the bitmaps is exact because no reference msd lies within msd_bound of the cut-off: zero
    undecided pairs in the three planted cases at 1.0 A and in the continuum case at 2.0 A, on the reference alone."""
    for key in cr.PLANTED_CASES:
        x, blob = cr.planted(*key)
        msd, bound = cr.reference("planted", *key)
        same = blob[:, None] == blob[None, :]
        off = ~np.eye(key[0], dtype=bool)
        within, between = float(np.sqrt(msd[same & off].max())), float(np.sqrt(msd[~same].min()))
        print(f"planted {key}: largest within-cluster RMSD {within:.3f}, smallest between {between:.3f}")
        assert within < 0.8 < 1.0 < 2.0 < between
        assert int(cr.undecided(msd, bound, cr.PLANTED_CUTOFF ** 2).sum()) == 0
        d = cr.daura(msd <= cr.PLANTED_CUTOFF ** 2)
        assert d["n_clusters"] == len(set(blob.tolist())) and all(len(set(blob[d["labels"] == k].tolist())) == 1 for k in range(d["n_clusters"]))
    msd, bound = cr.reference("continuum")
    cut2 = cr.CONTINUUM_CUTOFF ** 2
    off = ~np.eye(130, dtype=bool)
    inside = msd <= cut2
    print(f"continuum: {inside[off].mean():.3f} of the pairs inside {cr.CONTINUUM_CUTOFF} A, the nearest {np.abs(msd[off] - cut2).min():.1e} A^2 "
          f"from the cut, bound {bound.max():.1e}")
    assert 0.05 < inside[off].mean() < 0.25 and int(cr.undecided(msd, bound, cut2).sum()) == 0
    # not transitive: some A ~ B ~ C with A and C apart, so the centre rule decides the clusters
    assert ((inside.astype(np.int64) @ inside.astype(np.int64)) > 0)[~inside].any()
    d = cr.daura(inside)
    assert d["centres"][0] != 0 and d["sizes"][0] > 1 and (d["sizes"] == 1).sum() > 10      # a centre the rule picks; a tail of singletons


@pytest.mark.parametrize("name", list(cr.HAND), ids=lambda s: s.split(":")[0])
def test_reference_loop_gives_the_hand_derived_answers(name):
    N, edges, labels, centres, sizes = cr.HAND[name]
    nb = cr.from_edges(N, edges)
    d = cr.daura(nb)
    assert d["labels"].tolist() == list(labels) and d["centres"].tolist() == list(centres) and d["sizes"].tolist() == list(sizes)
    assert d["n_clusters"] == len(centres) and sum(sizes) == N
    for garbage in (False, True):
        back = cr.unpack(cr.pack(nb, garbage), N)
        assert (back[:, :N] == nb).all() and (back[:, N:] == garbage).all()
    fin = np.ones(N, dtype=bool)
    fin[centres[0]] = False                                          # without the first centre nobody carries its label
    d2 = cr.daura(nb, fin)
    assert d2["labels"][centres[0]] == -1 and (d2["labels"][fin] >= 0).all() and d2["sizes"].sum() == N - 1


def test_cli_refuses_a_cluster_cutoff_that_is_not_positive():
    cli = load_cli("codlad_cli")
    a = argparse.Namespace(cluster=None, experiment="latent")
    assert cli.check_cluster(a) == 0.0 and a.cluster == 0.0
    assert cli.check_cluster(argparse.Namespace(cluster=1.5, experiment="latent")) == 1.5
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SystemExit, match="--cluster takes an RMSD cut-off in A, a positive number"):
            cli.check_cluster(argparse.Namespace(cluster=bad, experiment="latent"))
    with pytest.raises(SystemExit, match="generates none"):
        cli.check_cluster(argparse.Namespace(cluster=1.0, experiment="bpd"))
    flag, atoms = option(cli, "--cluster"), option(cli, "--cluster_atoms")
    assert flag.type is float and flag.nargs is None and flag.default is None
    assert tuple(atoms.choices) == ("ca", "all") and atoms.default == "ca"
    parsed = cli.build_parser().parse_args(["--cluster", "1.5", "--cluster_atoms", "all"])
    assert parsed.cluster == 1.5 and parsed.cluster_atoms == "all"
