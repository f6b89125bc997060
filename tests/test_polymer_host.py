"""CPU checks of the chain-statistics feature: the C ABI of codlad_chain_sums and codlad_gyration (declared once, exported,
counted in _SIGS, bad arguments refused before any HIP call, the split rule on both sides of its thresholds), the kernels'
registers, what the Python layer refuses, the references of tests/polymer_ref.py against answers derived by hand, and the
Flory fit."""
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import polymer_ref as pr
from tests.test_cluster_host import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = (("codlad_chain_sums_groups", 2), ("codlad_chain_sums", 10), ("codlad_gyration", 11))
KERNELS = ("chain_sums_kernel", "chain_finish_kernel", "gyration_kernel")


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, n_args in ENTRY_POINTS:
        decl = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value, mine in (("MAX_SEL", 8192, _lib.POLYMER_MAX_SEL), ("SPLIT_MAX_N", 256, _lib.POLYMER_SPLIT_MAX_N),
                               ("SPLIT_MIN_SEL", 512, _lib.POLYMER_SPLIT_MIN_SEL)):
        assert f"#define CODLAD_POLYMER_{macro} {value}\n" in header and mine == value == getattr(metrics, "POLYMER_" + macro)
        assert pr.macro(macro) == value
    assert pr.MAX_SEL >= 4325                            # the project's large all-atom shape
    assert (pr.LANES, pr.TERM_OPS, pr.TREE_ADDS) == (64, 5, 6) and pr.JACOBI_STOP == 2.0 ** -60 and pr.EPS == 2.0 ** -52
    for name, expr in (("SUM", "(((m) + 63) / 64 + 11.0)"), ("INV_SUM", "(((m) + 63) / 64 + 11.0 + ((m) - 2.0))"),
                       ("TENSOR", "(((m) + 63) / 64 + 10.0)")):
        assert f"#define CODLAD_POLYMER_{name}_BOUND(m) ({expr} * 2.220446049250313e-16)\n" in header
    assert pr.sum_bound(129) == 14 * pr.EPS and pr.inv_sum_bound(129) == 141 * pr.EPS and pr.tensor_bound(64) == 11 * pr.EPS
    assert pr.sum_bound(8192) == 139 * pr.EPS and pr.eig_bound(2) == 11 * pr.EPS + 2.0 ** -60
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19 and lib.codlad_abi_version() == 19
    assert "polymer_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["polymer_kernels.hip"] == ["-ffp-contract=off"]
    for name in ("chain_sums", "hydrodynamic_radius", "gyration_tensor", "distance_scaling", "flory_fit"):
        assert callable(getattr(metrics, name)) and name in metrics.polymer.__all__


def test_polymer_kernels_use_no_scratch_and_spill_nothing():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "polymer_kernels.hip"}
    for kernel in KERNELS:
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    assert len(mine) == len(KERNELS), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced
    p = buf.ctypes.data

    def refuses(fn, ok, cases):
        for k, bad in cases:
            args = list(ok)
            args[k] = bad
            assert getattr(lib, fn)(*args) < 0, (fn, k, bad)
            assert fn.encode() in lib.codlad_last_error(), (fn, k, bad)

    #     x  N  n_atoms sel n_sel sep_r2 sep_inv inv_sum finite stream
    ok = [p, 4, 87, None, 0, p, p, p, p, None]
    refuses("codlad_chain_sums", ok, [(k, None) for k in (0, 5, 6, 7, 8)] +
            [(1, 0), (1, -1), (2, 0), (2, -1), (2, 1), (2, pr.MAX_SEL + 1), (4, 3), (4, -1)])
    args = list(ok)
    args[3] = p                                          # sel without n_sel
    assert lib.codlad_chain_sums(*args) < 0 and b"disagree" in lib.codlad_last_error()
    for n_sel in (1, pr.MAX_SEL + 1):                    # one selected atom has no pair; one more than the limit
        args[4] = n_sel
        assert lib.codlad_chain_sums(*args) < 0 and b"codlad_chain_sums" in lib.codlad_last_error()
    #     x  N  n_atoms sel n_sel mom tensor eig ree finite stream
    ok = [p, 4, 87, None, 0, p, p, p, p, p, None]
    refuses("codlad_gyration", ok, [(k, None) for k in (0, 5, 6, 7, 8, 9)] +
            [(1, 0), (1, -1), (2, 0), (2, -1), (2, pr.MAX_SEL + 1), (4, 3), (4, -1)])
    args = list(ok)
    args[3] = p
    assert lib.codlad_gyration(*args) < 0 and b"disagree" in lib.codlad_last_error()
    args[4] = pr.MAX_SEL + 1
    assert lib.codlad_gyration(*args) < 0 and b"codlad_gyration" in lib.codlad_last_error()


def test_the_split_rule_stands_on_both_sides_of_its_thresholds():
    groups = _lib.lib().codlad_chain_sums_groups
    for bad in ((0, 87), (-1, 87), (1, 1), (1, 0), (1, pr.MAX_SEL + 1)):
        assert groups(*bad) < 0 and b"codlad_chain_sums_groups" in _lib.lib().codlad_last_error(), bad
    assert groups(1, pr.SPLIT_MIN_SEL - 1) == 1 and groups(1, pr.SPLIT_MIN_SEL) == pr.SPLIT_MIN_SEL // 8   # four pairs of separations each
    assert groups(pr.SPLIT_MAX_N - 1, pr.SPLIT_MIN_SEL) > 1 and groups(pr.SPLIT_MAX_N, pr.SPLIT_MIN_SEL) == 1
    # many small structures: a workgroup each; few large ones: about a thousand workgroups in all
    assert groups(400, 87) == groups(65536, 129) == groups(65536, 4325) == 1
    assert groups(1, 4325) == 541 and groups(32, 4325) == 32 and groups(1, pr.MAX_SEL) == 1024


def test_python_layer_refuses_what_it_cannot_run():
    x = torch.zeros(4, 5, 3)
    calls = (metrics.chain_sums, metrics.hydrodynamic_radius, metrics.gyration_tensor, metrics.distance_scaling)
    for call in calls:
        with pytest.raises(RuntimeError, match="must be a CUDA tensor"):
            call(x)
    F = _FakeCuda(x)
    for call in calls:
        with pytest.raises(ValueError, match="non-empty"):
            call(_FakeCuda(torch.zeros(4, 5)))
        with pytest.raises(ValueError, match="outside"):
            call(F, sel=[0, 5])
        with pytest.raises(ValueError, match="sel is empty"):
            call(F, sel=[])
        with pytest.raises(ValueError, match=f"{pr.MAX_SEL} selected atoms, got {pr.MAX_SEL + 1}"):
            call(_FakeCuda(torch.zeros(2, pr.MAX_SEL + 1, 3)))
        if call is not metrics.gyration_tensor:
            with pytest.raises(ValueError, match=f"2 .. {pr.MAX_SEL} selected atoms, got 1"):
                call(F, sel=[3])
    for call in (metrics.hydrodynamic_radius, metrics.distance_scaling):
        for bad, msg in (([1.0] * 3, "one value per structure"), ([1.0, -1.0, 1.0, 1.0], "finite and >= 0"),
                         ([1.0, float("nan"), 1.0, 1.0], "finite and >= 0"), ([0.0] * 4, "every weight is 0")):
            with pytest.raises(ValueError, match=msg):
                call(F, weights=bad)


def test_the_reference_by_hand_rod_cube_and_lagrange():
    for m in (2, 3, 17, 64):
        x = pr.rod(m)
        r2s, invs, inv_sum, finite = pr.chain_sums_ld(x)
        want2, wanti = pr.rod_sums(m)
        assert finite.all() and (r2s[0] == want2).all() and np.abs(invs[0] - wanti).max() <= 1e-14
        assert abs(inv_sum[0] - wanti.sum()) <= 1e-13
        T, e, ree = pr.gyration_ld(x)
        lam = pr.LD(16 * (m * m - 1)) / pr.LD(12)
        assert T[0, 0] == lam and (T[0, 1:] == 0).all() and ree[0] == 4.0 * (m - 1)
        assert e[0].tolist() == [0.0, 0.0, float(lam)]
        asph, acyl, kappa2, prol = pr.shape_numbers(e[0])
        assert kappa2 == 1.0 and abs(prol - 2.0) <= 4 * pr.EPS and acyl == 0.0 and asph == e[0, 2]     # 3 l3 is rounded
    T, e, ree = pr.gyration_ld(pr.cube())
    assert e[0].tolist() == [0.25, 0.25, 0.25] and (T[0, 3:] == 0).all() and ree[0] == np.sqrt(pr.LD(3))
    asph, acyl, kappa2, prol = pr.shape_numbers(e[0])
    assert kappa2 == 0.0 and prol == 0.0 and asph == 0.0 and acyl == 0.0
    # Lagrange's identity: sum_s sep_r2[s] / m^2 = Rg^2 = the trace of the gyration tensor
    for N, m, kind in ((3, 65, "all"), (3, 63, "subset"), (1, 129, "descending")):
        c = pr.case(N, m, kind)
        rg2 = c["tensor"][:, :3].sum(1)
        assert np.abs(c["sep_r2"].sum(1) / pr.LD(m * m) - rg2).max() <= 1e-15 * float(rg2.max())
    # separation s is the s-th diagonal of the distance matrix
    c = pr.case(3, 65, "all")
    p = c["x"][1].astype(pr.LD)
    D2 = ((p[:, None] - p[None]) ** 2).sum(-1)
    for s in (1, 7, 64):
        assert abs(np.diagonal(D2, s).sum() - c["sep_r2"][1, s - 1]) <= 1e-16 * float(c["sep_r2"][1, s - 1])
        assert abs((1 / np.sqrt(np.diagonal(D2, s))).sum() - c["sep_inv"][1, s - 1]) <= 1e-16 * float(c["sep_inv"][1, s - 1])
    # the reversed chain has the same per-separation sums; a structure that is not finite has NaN rows, its neighbours keep theirs
    d = pr.case(1, 129, "descending")
    fwd = pr.chain_sums_ld(d["x"])
    assert np.abs(fwd[0] - d["sep_r2"]).max() <= 1e-15 * float(fwd[0].max()) and abs(fwd[2][0] - d["inv_sum"][0]) <= 1e-15 * float(fwd[2][0])
    x = c["x"].copy()
    x[1, 5, 2] = np.inf
    r2s, invs, inv_sum, finite = pr.chain_sums_ld(x)
    assert finite.tolist() == [True, False, True] and np.isnan(r2s[1]).all() and np.isnan(inv_sum[1])
    assert (r2s[[0, 2]] == c["sep_r2"][[0, 2]]).all() and (inv_sum[[0, 2]] == c["inv_sum"][[0, 2]]).all()
    x = pr.rod(5)
    x[0, 3] = x[0, 1]                                     # two coincident beads, two apart
    r2s, invs, inv_sum, finite = pr.chain_sums_ld(x)
    assert finite.all() and np.isinf(invs[0]).tolist() == [False, True, False, False] and inv_sum[0] == np.inf
    assert {pr.case(N, m)["x"].shape for N in pr.SHAPE_N for m in (2, 257)} == {(N, m, 3) for N in (1, 3, 70) for m in (2, 257)}


def test_flory_fit_recovers_the_exponent_and_the_prefactor():
    s = np.arange(1, 200)
    fit = metrics.flory_fit(s, 5.5 * s ** 0.6)
    assert abs(fit["nu"] - 0.6) <= 1e-12 and abs(fit["r0"] - 5.5) <= 1e-12 and fit["n_points"] == 100 - 5 + 1
    fit = metrics.flory_fit(torch.from_numpy(s), torch.from_numpy(5.5 * s ** 0.6), s_min=10, s_max=50, r0=5.5)
    assert abs(fit["nu"] - 0.6) <= 1e-12 and fit["r0"] == 5.5 and fit["n_points"] == 41
    m = 64                                               # the rod: R(s) = 4 s
    r2s, _i, _s, _f = pr.chain_sums_ld(pr.rod(m))
    sep = np.arange(1, m)
    r_rms = np.sqrt((r2s[0] / (m - sep)).astype(np.float64))
    assert (r_rms == 4.0 * sep).all()
    fit = metrics.flory_fit(sep, r_rms)
    assert abs(fit["nu"] - 1.0) <= 1e-12 and abs(fit["r0"] - 4.0) <= 1e-12 and fit["n_points"] == m // 2 - 5 + 1
    # separations whose R is not a positive finite number are left out
    R = 5.5 * s ** 0.6
    R[[20, 30]] = np.nan, 0.0
    fit = metrics.flory_fit(s, R)
    assert abs(fit["nu"] - 0.6) <= 1e-12 and fit["n_points"] == 94


def test_flory_fit_refuses_a_fit_over_fewer_than_two_separations():
    s = np.arange(1, 200)
    R = 5.5 * s ** 0.6
    for kw in (dict(s_min=7, s_max=7), dict(s_min=50, s_max=40), dict(s_min=500)):
        with pytest.raises(ValueError, match="fewer than two separations"):
            metrics.flory_fit(s, R, **kw)
    with pytest.raises(ValueError, match="fewer than two separations"):
        metrics.flory_fit(np.arange(1, 8), 4.0 * np.arange(1, 8))          # m = 8: s_max = 4 < s_min = 5
    with pytest.raises(ValueError, match="fewer than two separations"):
        metrics.flory_fit(s, np.full(199, np.nan))
    with pytest.raises(ValueError, match="one length"):
        metrics.flory_fit(s, R[:-1])
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="r0 must be a positive finite number"):
            metrics.flory_fit(s, R, r0=bad)
