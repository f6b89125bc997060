"""CPU checks of the essential-dynamics feature: the C ABI of codlad_pca_* (declared once, exported, counted in _SIGS, bad
arguments refused before any HIP call, the scratch sizes), the kernels' registers, what the Python layer and the CLI refuse,
and the reference of tests/pca_ref.py against answers derived by hand and against the planted truth."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import pca_ref as pr
from tests.test_cluster_host import _FakeCuda
from tests.cli_script import load_cli, option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("codlad_pca_fit_scratch_bytes", "long long", 2), ("codlad_pca_fit", "int", 19), ("codlad_pca_align", "int", 11),
                ("codlad_pca_deviations", "int", 13), ("codlad_pca_covariance_scratch_bytes", "long long", 2),
                ("codlad_pca_covariance", "int", 11), ("codlad_pca_eigen_scratch_bytes", "long long", 2),
                ("codlad_pca_eigen", "int", 12), ("codlad_pca_project", "int", 7))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, ret, n_args in ENTRY_POINTS:
        decl = re.findall(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    assert sorted(n for n in _lib._SIGS if n.startswith("codlad_pca_")) == sorted(n for n, _r, _a in ENTRY_POINTS)
    for macro, value in (("MAX_N", 65536), ("MAX_DIM", 4096), ("MAX_COMPONENTS", 64), ("MAX_ITER", 4096), ("STATE_WORDS", 8),
                         ("ST_PHASE", 0), ("ST_ITER", 1), ("ST_STATUS", 2), ("ST_START", 3), ("SCALARS", 4), ("SC_W", 0), ("SC_STEP", 1)):
        assert f"#define CODLAD_PCA_{macro} {value}\n" in header and getattr(_lib, f"PCA_{macro}") == value
    for k, status in enumerate(("CONVERGED", "LIMIT", "NO_WEIGHT")):
        assert f"#define CODLAD_PCA_{status} {k}\n" in header and _lib.PCA_STATUS[k] == status.lower()
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "pca_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["pca_kernels.hip"] == ["-ffp-contract=off"]
    assert (metrics.PCA_MAX_N, metrics.PCA_MAX_DIM, metrics.PCA_MAX_COMPONENTS) == (65536, 4096, 64)
    for name in ("mean_structure", "rmsf", "covariance", "pca", "pca_project"):
        assert callable(getattr(metrics, name))


def test_pca_kernels_use_no_scratch_and_the_covariance_keeps_two_waves():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "pca_kernels.hip"}
    for kernel in ("pca_init_kernel", "pca_align_kernel", "pca_mean_kernel", "pca_step_kernel", "pca_dev_kernel", "pca_rmsf_kernel",
                   "pca_cov_kernel", "pca_cov_reduce_kernel", "pca_corr_kernel", "pca_orth_kernel", "pca_cq_kernel", "pca_h_kernel",
                   "pca_jacobi_kernel", "pca_rot_kernel", "pca_status_kernel", "pca_project_kernel", "pca_tmom_kernel"):
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
    cov = [r for k, r in mine.items() if "pca_cov_kernel" in k][0]
    assert cov["VGPRs"] <= 256 and cov["Occupancy"] >= 2, cov


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

    for fn, bads in (("codlad_pca_fit_scratch_bytes", ((0, 4), (-1, 4), (65537, 4), (4, 0), (4, -1))),
                     ("codlad_pca_covariance_scratch_bytes", ((0, 6), (65537, 6), (4, 0), (4, 4097), (4, 4099), (4, 7), (4, -3))),
                     ("codlad_pca_eigen_scratch_bytes", ((0, 1), (4097, 1), (6, 0), (6, 7), (300, 65), (6, -1)))):
        for bad in bads:
            assert getattr(lib, fn)(*bad) < 0 and fn.encode() in lib.codlad_last_error(), (fn, bad)
    # the chunk partials [chunks][m][3] and the target's four moments; chunks of 1, 65 and 65 536 structures: 1, 1, 32
    assert lib.codlad_pca_fit_scratch_bytes(1, 1) == 8 * (3 + 4)
    assert lib.codlad_pca_fit_scratch_bytes(65, 65) == 8 * (3 * 65 + 4)
    assert lib.codlad_pca_fit_scratch_bytes(65536, 129) == 8 * (3 * 129 * 32 + 4)
    # one 64 x 64 tile of doubles per (tile of the lower triangle, chunk)
    assert lib.codlad_pca_covariance_scratch_bytes(1, 3) == 8 * 4096
    assert lib.codlad_pca_covariance_scratch_bytes(1030, 195) == 8 * 4096 * 10 * 3
    assert lib.codlad_pca_covariance_scratch_bytes(16400, 4095) == 8 * 4096 * 2080 * 32
    # four blocks [b][d], three [b][b], three [b], b = min(k + 8, d)
    assert lib.codlad_pca_eigen_scratch_bytes(3, 3) == 8 * (4 * 9 + 3 * 9 + 9)
    assert lib.codlad_pca_eigen_scratch_bytes(195, 4) == 8 * (4 * 12 * 195 + 3 * 144 + 36)
    assert lib.codlad_pca_eigen_scratch_bytes(4096, 64) == 8 * (4 * 72 * 4096 + 3 * 72 * 72 + 3 * 72)
    #     x  mom N  n_atoms sel n_sel w start tol  max_iter iters state scal target mean Rt finite scratch stream
    ok = [p, p, 4, 5, None, 0, None, -1, 1e-6, 100, 8, p, p, p, p, p, p, p, None]
    refuses("codlad_pca_fit", ok, [(k, None) for k in (0, 1, 11, 12, 13, 14, 15, 16, 17)] +
            [(2, 0), (2, -1), (2, 65537), (3, 0), (5, -1), (5, 3), (7, -2), (7, 4), (8, 0.0), (8, -1.0), (8, nan), (8, inf),
             (9, 0), (9, 4097), (10, -1), (10, 4097)])
    args = list(ok)
    args[4] = p                                          # sel without n_sel
    assert lib.codlad_pca_fit(*args) < 0 and b"disagree" in lib.codlad_last_error()
    #     x  mom N  n_atoms sel n_sel target tmom Rt finite stream
    ok = [p, p, 4, 5, None, 0, p, p, p, p, None]
    refuses("codlad_pca_align", ok, [(k, None) for k in (0, 1, 6, 7, 8, 9)] + [(2, 0), (2, 65537), (3, 0), (5, 2), (5, -1)])
    #     x  Rt finite w N  n_atoms sel n_sel mean scal D  rmsf stream
    ok = [p, p, p, None, 4, 5, None, 0, p, p, p, p, None]
    refuses("codlad_pca_deviations", ok, [(k, None) for k in (0, 1, 2, 8)] + [(4, 0), (4, 65537), (5, 0), (7, 1), (7, -1)])
    args = list(ok)
    args[10] = args[11] = None                           # neither output
    assert lib.codlad_pca_deviations(*args) < 0
    args = list(ok)
    args[9] = None                                       # the RMSF divides by W
    assert lib.codlad_pca_deviations(*args) < 0 and b"scal" in lib.codlad_last_error()
    #     D  w  finite N  d  scal cov corr total scratch stream
    ok = [p, None, p, 4, 6, p, p, p, p, p, None]
    refuses("codlad_pca_covariance", ok, [(k, None) for k in (0, 2, 5, 6, 7, 8, 9)] +
            [(3, 0), (3, 65537), (4, 0), (4, 7), (4, 4097), (4, 4098), (4, -3)])
    #     cov d  k  rtol max_iter iters state evals comps resid scratch stream
    ok = [p, 6, 2, 1e-10, 1000, 16, p, p, p, p, p, None]
    refuses("codlad_pca_eigen", ok, [(k, None) for k in (0, 6, 7, 8, 9, 10)] +
            [(1, 0), (1, 4097), (2, 0), (2, 7), (2, 65), (2, -1), (3, 0.0), (3, -1e-10), (3, nan), (3, inf), (4, 0), (4, 4097),
             (5, -1), (5, 4097)])
    #     D  comps N  d  k  P  stream
    ok = [p, p, 4, 6, 2, p, None]
    refuses("codlad_pca_project", ok, [(k, None) for k in (0, 1, 5)] + [(2, 0), (2, 65537), (3, 0), (3, 4097), (4, 0), (4, 7), (4, 65)])


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 5, 3)
    for call in (lambda: metrics.mean_structure(x), lambda: metrics.rmsf(x), lambda: metrics.covariance(x), lambda: metrics.pca(x, 2),
                 lambda: metrics.pca_project(x, {"mean": torch.zeros(5, 3), "components": torch.zeros(2, 5, 3)})):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    F = _FakeCuda(x)
    calls = (metrics.mean_structure, metrics.rmsf, metrics.covariance, lambda *a, **k: metrics.pca(*a, n_components=2, **k))
    big = _FakeCuda(torch.zeros(65537, 1, 3))
    for call in calls:
        with pytest.raises(ValueError, match="at most 65536 structures"):
            call(big)
        with pytest.raises(ValueError, match="non-empty"):
            call(_FakeCuda(torch.zeros(4, 5)))
        with pytest.raises(ValueError, match="outside"):
            call(F, sel=[0, 5])
        with pytest.raises(ValueError, match="sel is empty"):
            call(F, sel=[])
        for bad, what in ((np.ones(3), "one value per structure"), (np.array([1, -1, 1, 1.0]), "finite and >= 0"),
                          (np.array([1, np.nan, 1, 1.0]), "finite and >= 0"), (np.array([1, np.inf, 1, 1.0]), "finite and >= 0"),
                          (np.zeros(4), "every weight is 0")):
            with pytest.raises(ValueError, match=what):
                call(F, weights=bad)
        for bad in (0.0, -1e-6, float("nan"), float("inf"), None, "tight"):
            with pytest.raises(ValueError, match="tol must be a positive finite number"):
                call(F, tol=bad)
        for bad in (-1, 4, 1.0, True):
            with pytest.raises(ValueError, match="start must be the index of a structure"):
                call(F, start=bad)
        with pytest.raises(ValueError, match="the start structure 2 has weight 0"):
            call(F, start=2, weights=np.array([1, 1, 0, 1.0]))
    for call in (metrics.mean_structure, metrics.rmsf, metrics.covariance):
        for bad in (0, -1, 4097, 2.0):
            with pytest.raises(ValueError, match="max_iter must be an integer in 1 .. 4096"):
                call(F, max_iter=bad)
    wide = _FakeCuda(torch.zeros(2, 1366, 3))                            # d = 4 098
    for call in (metrics.covariance, lambda a: metrics.pca(a, 2)):
        with pytest.raises(ValueError, match="4098 coordinates, at most 4096"):
            call(wide)
    for bad in (0, -1, 65, 16, 2.0, None, True):                         # d = 15 here
        with pytest.raises(ValueError, match="n_components must be an integer in 1 .. 15"):
            metrics.pca(F, n_components=bad)
    with pytest.raises(ValueError, match="n_components must be an integer in 1 .. 64"):
        metrics.pca(_FakeCuda(torch.zeros(4, 30, 3)), n_components=65)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rtol must be a positive finite number"):
            metrics.pca(F, 2, rtol=bad)
    with pytest.raises(ValueError, match="max_iter must be an integer"):
        metrics.pca(F, 2, max_iter=0)
    with pytest.raises(ValueError, match="model must be the dict pca returns"):
        metrics.pca_project(F, {"mean": torch.zeros(5, 3)})
    with pytest.raises(ValueError, match="do not match"):
        metrics.pca_project(F, {"mean": torch.zeros(4, 3), "components": torch.zeros(2, 4, 3)})


def test_cli_refuses_what_pca_cannot_run():
    cli = load_cli("codlad_cli")
    a = argparse.Namespace(pca=None, experiment="latent")
    assert cli.check_pca(a) == 0 and a.pca == 0
    assert cli.check_pca(argparse.Namespace(pca=10, experiment="latent")) == 10
    for bad in (0, -1, 65):
        with pytest.raises(SystemExit, match="--pca takes the number of components, 1 .. 64"):
            cli.check_pca(argparse.Namespace(pca=bad, experiment="latent"))
    with pytest.raises(SystemExit, match="generates none"):
        cli.check_pca(argparse.Namespace(pca=3, experiment="bpd"))
    assert cli.pca_selection("p", 500, "ca", [1, 5, 9]) == [1, 5, 9] and cli.pca_selection("p", 1365, "all", [1]) is None
    with pytest.raises(SystemExit, match="3 x 1366 = 4098 coordinates over the chosen atoms, at most 4096"):
        cli.pca_selection("p", 1366, "all", [1, 5])
    with pytest.raises(SystemExit, match="the CA atoms of p are not known"):
        cli.pca_selection("p", 100, "ca", None)
    flag, atoms = option(cli, "--pca"), option(cli, "--pca_atoms")
    assert flag.type is int and flag.nargs == "?" and flag.const == 10 and flag.default is None
    assert tuple(atoms.choices) == ("ca", "all") and atoms.default == "ca"
    parse = cli.build_parser().parse_args
    assert parse(["--pca"]).pca == 10 and parse(["--pca", "3", "--pca_atoms", "all"]).pca == 3 and parse([]).pca is None


def test_cases_are_the_shapes_the_issue_names():
    assert {N for N, _m, _k in pr.SHAPES} == {1, 2, 3, 15, 16, 17, 65, 130, 1030}
    assert {m for _N, m, _k in pr.SHAPES} == {1, 2, 21, 22, 43, 65} and 10 <= len(pr.SHAPES) <= 14
    assert pr.LARGE_DIM[:2] == (20, 1365) and pr.MANY[:2] == (16400, 2)
    assert (130, 65, "walk") in pr.SHAPES and (1030, 43, "walk") in pr.SHAPES
    for N, m, kind in pr.SHAPES:
        x = pr.pool(N, m, kind)
        assert x.shape == (N, m, 3) and x.dtype == np.float32 and not x.flags.writeable
    far = np.abs(pr.pool(65, 21, "far")).max(axis=(1, 2)) > 400
    assert far[1::2].all() and not far[::2].any()


def test_reference_two_structures_by_hand():
    """Two structures base +- delta, delta a stretch of one atom pair along its own axis (orthogonal to every rigid motion, so
    they are superposed as they stand): the mean is base, the deviations are +-delta, the covariance is delta delta^T."""
    base = np.array([[0.0, 0, 0], [4, 0, 0], [0, 3, 0], [0, 0, 5], [4, 3, 0], [4, 0, 5]])
    base -= base.mean(0)
    delta = np.zeros((6, 3))
    delta[0, 0], delta[1, 0] = 0.25, -0.25         # atoms 0 and 1 lie on one line along x: a stretch of it, no net force or torque
    x = np.stack((base + delta, base - delta))
    f = pr.procrustes(x)
    assert f["status"] == "converged" and f["W"] == 2.0
    assert np.abs(f["mean"] - base).max() < 1e-12
    r = pr.reference_pca(x, 2)
    want = np.outer(delta.reshape(-1), delta.reshape(-1))
    assert np.abs(r["C"] - want).max() < 1e-12
    assert abs(r["lam"][0] - 2 * 0.25 ** 2) < 1e-12 and abs(r["lam"][1]) < 1e-12
    v = delta.reshape(-1) / np.linalg.norm(delta)
    assert abs(abs(r["vec"][0] @ v) - 1.0) < 1e-12
    # weights 3 : 1 move the mean to base + delta / 2 and give the variance 4 p (1 - p) a^2 per displaced coordinate
    fw = pr.procrustes(x, w=np.array([3.0, 1.0]))
    assert np.abs(fw["mean"] - (base + 0.5 * delta)).max() < 1e-12
    rw = pr.reference_pca(x, 1, w=np.array([3.0, 1.0]))
    assert abs(rw["lam"][0] - 2 * 4 * 0.75 * 0.25 * 0.25 ** 2) < 1e-12


def test_reference_rigid_copies_have_no_variance():
    rng = np.random.default_rng(11)
    base = rng.standard_normal((21, 3)) * 5
    x = np.stack([base @ pr._rotation(rng).T + rng.standard_normal(3) * 10 for _ in range(7)])
    f = pr.procrustes(x)
    assert f["status"] == "converged" and f["n_iter"] <= 2
    r = pr.reference_pca(x, 3)
    assert np.abs(r["D"]).max() < 1e-12 and np.abs(r["C"]).max() < 1e-24 and np.abs(r["lam"]).max() < 1e-24
    nan = x.copy()
    nan[2, 3, 1] = np.nan                                               # a structure that is not finite takes no part
    fn = pr.procrustes(nan)
    assert not fn["finite"][2] and fn["W"] == 6.0 and np.isnan(fn["A"][2]).all() and np.abs(fn["mean"] - f["mean"]).max() < 1e-12


def test_reference_recovers_a_single_planted_mode_and_the_planted_spectra():
    rng = np.random.default_rng(12)
    m, N = 22, 40
    base = rng.standard_normal((m, 3)) * 5
    base -= base.mean(0)
    rigid = pr.rigid_basis(base)
    assert rigid.shape == (6, 3 * m) and np.abs(rigid @ rigid.T - np.eye(6)).max() < 1e-12
    u = rng.standard_normal(3 * m)
    u -= rigid.T @ (rigid @ u)
    u /= np.linalg.norm(u)
    c = rng.standard_normal(N)
    c -= c.mean()
    c *= np.sqrt(N) / np.linalg.norm(c)
    sigma = 1e-3                                                        # small: the superposition is exact to second order
    x = np.stack([(base + sigma * ci * u.reshape(m, 3)) @ pr._rotation(rng).T + rng.standard_normal(3) for ci in c])
    r = pr.reference_pca(x, 2)
    back = pr.align(r["fit"]["mean"][None], base)[1][0]                 # the frame of the mean against the base's
    v = (r["vec"][0].reshape(m, 3) @ back.T).reshape(-1)
    assert abs(r["lam"][0] - sigma ** 2) <= 1e-6 * sigma ** 2 and r["lam"][1] <= 1e-6 * sigma ** 2
    assert abs(abs(v @ u) - 1.0) <= 1e-6
    worst = 0.0
    for name in pr.PLANTED:
        xs, _modes, lam = pr.planted(name)
        got = pr.reference_pca(xs, len(lam))["lam"]
        worst = max(worst, float(np.abs(got - lam).max() / lam[0]))
        print(f"planted {name}: reference eigenvalues off by {np.abs(got - lam).max() / lam[0]:.2e} of the largest")
    assert worst <= pr.PLANTED_RECOVERY / 2 * 1.05 and pr.PLANTED_RECOVERY <= 4 * worst      # the constant is twice the measured
