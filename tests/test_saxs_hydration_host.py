"""CPU checks of the SAXS hydration feature: the C ABI of codlad_saxs_partials and codlad_saxs_hydration_fit (declared,
exported, bad arguments refused before any HIP call), the registers of the new kernels, what the Python layer and the
command line refuse, and the references of tests/saxs_hydration_ref.py - the float64 partials against the analytic two- and
three-atom curves, the identity I(c1 = 1, c2 = 0) = the plain Debye sum, the combination against the direct double sum of
|F|^2, and the grid fit on a planted point.

Figures (printed by every run): dev32 of the cases lies between 1.8e-9 and 2.5e-7 per partial (0 for one atom); the
combination agrees with the direct double sum to 7.7e-15 of the sum of its absolute terms; the planted fit's runner-up has
chi2 = 2.4e-2 against 3.6e-28 at the planted point."""
import argparse
import json
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from codlad_amd.metrics import saxs as saxs_mod
from codlad_amd.utils.cg_input import template_topology
from tests import saxs_hydration_ref as hr
from tests import saxs_ref as sr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, n_args in (("codlad_saxs_partials", 15), ("codlad_saxs_hydration_fit", 16)):
        decl = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19 == _lib.ABI_VERSION
    assert (hr.N_PARTIALS, hr.CHUNK, hr.MAX_GRID) == (_lib.SAXS_HYD_PARTIALS, _lib.SAXS_HYD_Q_CHUNK, _lib.SAXS_HYD_MAX_GRID) == (6, 8, 4096)
    assert (metrics.SAXS_HYD_Q_CHUNK, metrics.SAXS_HYD_MAX_GRID, metrics.SAXS_PARTIAL_NAMES) == (8, 4096, hr.NAMES)
    assert sr.CHUNK == 16                                                            # the plain kernel keeps its own
    assert "saxs_hydration_kernels.hip" in build.SOURCES
    assert build.EXTRA_FLAGS["saxs_hydration_kernels.hip"] == ["-ffp-contract=off"] == build.EXTRA_FLAGS["saxs_kernels.hip"]
    # the sine and the selection of sinc have one home, which both files include
    shared = open(os.path.join(build.CSRC, "saxs_math.h")).read()
    for fn in ("lane_read", "sin_cw", "sinc_term"):
        assert len(re.findall(r"__device__ inline float " + fn + r"\(", shared)) == 1, fn
        for src in ("saxs_kernels.hip", "saxs_hydration_kernels.hip"):
            text = open(os.path.join(build.CSRC, src)).read()
            assert '#include "saxs_math.h"' in text and not re.search(r"float " + fn + r"\(", text), (src, fn)
    # the default grids are FoXS's ranges and hold the neutral point
    c1, c2 = metrics.default_c1(), metrics.default_c2()
    assert c1.shape == (21,) and c2.shape == (61,) and c1.size * c2.size <= hr.MAX_GRID
    assert (c1[0], c1[10], c1[-1]) == (0.95, 1.0, 1.05) and (c2[0], c2[20], c2[-1]) == (-2.0, 0.0, 4.0)
    assert np.allclose(np.diff(c1), 0.005, rtol=0, atol=1e-12) and np.allclose(np.diff(c2), 0.1, rtol=0, atol=1e-12)


def test_new_kernels_use_no_scratch():
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "saxs_hydration_kernels.hip"}
    for kernel in ("saxs_part_kernel", "saxs_part_sum", "saxs_part_mean", "saxs_fit_kernel", "saxs_combine_kernel", "finite_kernel"):
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        if "saxs_part_kernel" in name:
            # 18 accumulators per k at a chunk of 8: the 256-register step, two waves per SIMD
            print(f"saxs_part_kernel: {r['VGPRs']} VGPRs, occupancy {r['Occupancy']}")
            assert r["VGPRs"] <= 256 and r["Occupancy"] >= 2, (name, r)
        else:
            assert r["VGPRs"] <= 128, (name, r)
    # the plain pair kernel is where it was: three waves per SIMD
    pair = [v for k, v in table.items() if "saxs_pair_kernel" in k]
    assert len(pair) == 1 and pair[0]["VGPRs"] <= 168 and pair[0]["ScratchSize"] == 0


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced by these calls
    p = buf.ctypes.data
    ok = [p, 1, 4, p, 2, p, p, p, p, 8, p, p, p, p, None]
    cases = [(k, None) for k in (0, 3, 5, 6, 7, 8, 10, 11, 13)]
    cases += [(1, 0), (1, -1), (2, 0), (2, -3), (4, 0), (4, -1), (4, 33), (9, 0), (9, -1), (9, 513), (1, 2 ** 31 - 1), (2, 2 ** 30)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        if (k, bad) == (1, 2 ** 31 - 1):
            args[2] = 129                                # two workgroups a structure: the grid passes 2^31
        assert lib.codlad_saxs_partials(*args) < 0, (k, bad)
        assert b"codlad_saxs_partials" in lib.codlad_last_error(), (k, bad)
    # the fit: P, n_batch, n_q, f_w, G, n_c1, c2, n_c2, I_exp, sigma, I_grid, scale, chi2, best, I_best, stream
    fit = [p, 1, 8, p, p, 3, p, 4, p, p, None, p, p, p, p, None]
    combine = [p, 1, 8, p, p, 3, p, 4, None, None, p, None, None, None, None, None]
    cases = [(fit, k, None) for k in (0, 3, 4, 6, 8, 9, 11, 12, 13, 14)] + [(combine, k, None) for k in (0, 3, 4, 6, 10)]
    cases += [(combine, 9, p), (combine, 8, p)]                                       # one of I_exp / sigma
    for base in (fit, combine):
        cases += [(base, 1, 0), (base, 1, -1), (base, 2, 0), (base, 2, 513), (base, 5, 0), (base, 7, 0), (base, 7, -2),
                  (base, 5, 1025), (base, 7, 2 ** 30)]                                # 1025 x 4 grid points: over the cap
    cases += [(fit, 2, 1)]                                                            # a fit of one q value has no chi2
    for base, k, bad in cases:
        args = list(base)
        args[k] = bad
        assert lib.codlad_saxs_hydration_fit(*args) < 0, (base is fit, k, bad)
        assert b"codlad_saxs_hydration_fit" in lib.codlad_last_error(), (k, bad)


def test_python_layer_refuses_what_it_cannot_run():
    top = template_topology(["ALA", "GLY", "SER"])
    n = top.n_atoms
    x = torch.zeros(2, n, 3)
    q = np.linspace(0.01, 0.5, 8)
    P = torch.ones(6, 8, dtype=torch.float64)
    for call in (lambda: metrics.saxs_partials(x, top),
                 lambda: metrics.saxs_partials_lists(x, [0] * n, np.ones((1, 8)), np.ones((1, 8)), torch.zeros(2, n), q),
                 lambda: metrics.saxs_combine(P, q, np.ones(8), 1.02, 1.0),
                 lambda: metrics.saxs_hydration_fit(P, q, np.ones(8), np.ones(8), np.ones(8))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    assert "_saxs_hydration_tables" not in top.__dict__ and "_saxs_tables" not in top.__dict__   # refused before any table
    tables = lambda shape=(6, 8), qq=q, fw=np.ones(8), c1=(1.0, 1.02), c2=(0.0, 1.0), r_m=1.62: \
        saxs_mod._hydration_tables("saxs_combine", shape, qq, fw, c1, c2, r_m)              # noqa: E731
    fw, G, g1, g2 = tables()
    assert fw.dtype == G.dtype == np.float64 and G.shape == (2, 8) and (G[0] == 1.0).all() and g1.tolist() == [1.0, 1.02]
    assert np.array_equal(G, hr.expansion64(q, [1.0, 1.02])) and np.array_equal(G, metrics.expansion_factor(q, [1.0, 1.02]))
    for shape in ((8,), (5, 8), (6, 0), (0, 6, 8), (6, 8, 1)):
        with pytest.raises(ValueError, match=r"\[\.\.\., 6, Q\]"):
            tables(shape=shape)
    tables(shape=(3, 2, 6, 8))
    for kw in (dict(qq=q[:-1]), dict(fw=np.ones(9)), dict(shape=(6, 513), qq=np.linspace(0, 0.5, 513), fw=np.ones(513))):
        with pytest.raises(ValueError, match="values of P"):
            tables(**kw)
    limit = metrics.SAXS_Q_LIMIT
    for bad_q in (np.nan, np.inf, -0.1, limit * 1.001):
        qq = q.copy()
        qq[3] = bad_q
        with pytest.raises(ValueError, match="every q"):
            tables(qq=qq)
    tables(qq=np.linspace(0, limit, 8))
    for kw in (dict(c1=[]), dict(c2=[]), dict(c1=np.full(65, 1.0), c2=np.zeros(64))):
        with pytest.raises(ValueError, match="grid"):
            tables(**kw)
    tables(c1=np.full(64, 1.0), c2=np.zeros(64))                                     # 4096 points: the cap itself
    for kw in (dict(c1=[1.0, 0.0]), dict(c1=[-1.0]), dict(c1=[np.nan]), dict(c2=[np.inf]), dict(r_m=-1.0), dict(r_m=np.nan)):
        with pytest.raises(ValueError, match="c1 must be positive"):
            tables(**kw)
    exp, sig = saxs_mod._fit_curves(8, np.ones(8), np.full(8, 0.5))
    assert exp.dtype == sig.dtype == np.float64 and sig.tolist() == [0.5] * 8
    for e, s_, msg in ((np.ones(7), np.ones(8), "values of P"), (np.ones(8), np.ones(9), "values of P"),
                       (np.ones(8), np.zeros(8), "positive"), (np.ones(8), -np.ones(8), "positive"),
                       (np.ones(8), np.full(8, np.nan), "positive")):
        with pytest.raises(ValueError, match=msg):
            saxs_mod._fit_curves(8, e, s_)
    with pytest.raises(ValueError, match=">= 2"):
        saxs_mod._fit_curves(1, np.ones(1), np.ones(1))


def test_float64_partials_equal_the_analytic_two_and_three_atom_curves():
    q = np.linspace(0.0, 0.5, 8).astype(np.float32)
    q64 = q.astype(np.float64)
    ff_t = (np.array([[6.0], [-1.5]]) * np.exp(-q64 ** 2)[None]).astype(np.float32)
    ff_d = (np.array([[3.0], [7.0]]) * np.exp(-2 * q64 ** 2)[None]).astype(np.float32)
    t, d = ff_t.astype(np.float64), ff_d.astype(np.float64)

    def sinc(r):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(q64 * r == 0.0, 1.0, np.sin(q64 * r) / (q64 * r))

    # two atoms 3 A apart, types 0 and 1, exposures 0.25 and 0.75
    x = np.array([[[1.0, 2.0, 3.0], [1.0, 5.0, 3.0]]], dtype=np.float32)
    w = np.array([[0.25, 0.75]], dtype=np.float32)
    P, A = hr.partials64(x, [0, 1], ff_t, ff_d, w, q)
    f = [np.stack([t[0], t[1]]), np.stack([d[0], d[1]]), np.array([[0.25] * 8, [0.75] * 8])]
    for c, (a, b) in enumerate(hr.PAIRS):
        want = f[a][0] * f[b][0] + f[a][1] * f[b][1] + (f[a][0] * f[b][1] + f[b][0] * f[a][1]) * sinc(3.0)
        assert np.abs(P[0, c] - want).max() <= 4 * 2.0 ** -53 * A[0, c].max(), hr.NAMES[c]
        assert (A[0, c] >= np.abs(P[0, c])).all()
    assert np.array_equal(P[0, 0], sr.debye64(x, [0, 1], ff_t, q)[0][0])             # tt is the plain sum
    # three atoms on a 3-4-5 triangle, one of them buried (s = 0): the ss partial is the other two's
    x = np.array([[[0.0, 0.0, 0.0], [3.0, 0.0, 0.0], [0.0, 4.0, 0.0]]], dtype=np.float32)
    w = np.array([[0.5, 0.0, 1.0]], dtype=np.float32)
    P, A = hr.partials64(x, [0, 1, 1], ff_t, ff_d, w, q)
    s01, s02, s12 = sinc(3.0), sinc(4.0), sinc(5.0)
    want_ss = 0.25 + 1.0 + 2 * 0.5 * 1.0 * s02
    want_td = t[0] * d[0] + 2 * t[1] * d[1] + (t[0] * d[1] + d[0] * t[1]) * (s01 + s02) + 2 * t[1] * d[1] * s12
    want_ts = 0.5 * t[0] + t[1] + (t[0] * 1.0 + 0.5 * t[1]) * s02 + 0.5 * t[1] * s01 + t[1] * s12
    for c, want in ((5, want_ss), (1, want_td), (3, want_ts)):
        assert np.abs(P[0, c] - want).max() <= 8 * 2.0 ** -53 * A[0, c].max(), hr.NAMES[c]
    # the restatement of the kernel on the same three atoms, within float32 of it
    r32 = hr.partials32(x[0], [0, 1, 1], ff_t, ff_d, w[0], q)
    assert (np.abs(r32 - P[0]) <= 2.0 ** -20 * A[0]).all()


def test_references_agree_with_each_other_on_every_case():
    worst = 0.0
    for key in hr.case_keys():
        c = hr.case(key)
        plain, A = sr.debye64(c["x"], c["types"], c["ff_t"], c["q"])
        # I(1, 0) is the plain Debye sum: the tt partial itself, bit for bit, and through the combination
        assert np.array_equal(c["P"][:, 0], plain) and np.array_equal(c["A"][:, 0], A)
        assert np.array_equal(hr.combine64(c["P"], c["q"], c["water"], 1.0, 0.0), plain)
        assert (hr.expansion64(c["q"], [1.0]) == 1.0).all()
        # the tt restatement is the plain kernel's restatement
        assert np.array_equal(c["P32"][0, 0], sr.debye32(c["x"][0], c["types"], c["ff_t"], c["q"]))
        # the six-term combination is the double sum of |F|^2
        direct = hr.direct64(c["x"], c["types"], c["ff_t"], c["ff_d"], c["weight"], c["q"], c["water"], 1.03, 2.0)
        got = hr.combine64(c["P"], c["q"], c["water"], 1.03, 2.0)
        coef = np.abs(hr.coefficients64(c["q"], c["water"], 1.03, 2.0))
        scale = (coef[None] * c["A"]).sum(1)
        worst = max(worst, float((np.abs(got - direct) / scale).max()))
        assert (np.abs(got - direct) <= 2.0 ** -53 * (key[0] * (key[0] + 1) / 2 + 16) * scale).all(), key
        assert np.isfinite(c["P"]).all() and np.isfinite(c["P32"]).all() and (c["dev32"] <= 2.0 ** -20).all(), key
        assert (c["ff_d"] > 0).all() and (c["weight"] >= 0).all() and (c["weight"] <= 1).all()
        assert np.array_equal(c["weight"] * 96, np.rint(c["weight"] * 96))           # multiples of 1/96
        for arr in c.values():
            if isinstance(arr, np.ndarray):
                assert not arr.flags.writeable
    big = hr.case(hr.FIT_KEY)
    assert 0.35 < (big["weight"] == 0).mean() < 0.65 and (big["ff_t"] < 0).any() and (big["ff_t"] > 0).any()
    print(f"combination against the direct double sum: max |difference| / sum |coef| A = {worst:.2e}")
    print("dev32 per partial: " + "; ".join(f"{hr.case_id(k)} " + " ".join(f"{d:.1e}" for d in hr.case(k)["dev32"]) for k in hr.case_keys()))


def test_cases_cover_the_sizes_the_issue_names():
    keys = hr.case_keys()
    assert len(keys) == len(sr.case_keys())
    assert {k[0] for k in keys} == {1, 2, 63, 64, 65, 129, 300}
    assert {k[1] for k in keys} == set(hr.Q_SIZES) == {1, hr.CHUNK, hr.CHUNK + 1, 51}
    assert {k[2] for k in keys} == {1, 5, sr.MAX_TYPES}
    assert {k[3] for k in keys} == {0.0, 500.0}
    assert {k[4] for k in keys} == {"plain", "coincident", "q0", "far"}
    c = hr.case(next(k for k in keys if k[4] == "coincident"))
    assert (c["x"][:, 40] == c["x"][:, 7]).all() and (c["x"][1, 64] == c["x"][1, 0]).all()
    assert hr.case(next(k for k in keys if k[4] == "q0"))["q"][0] == 0.0
    far = hr.case(next(k for k in keys if k[4] == "far"))
    d = far["x"].astype(np.float64)
    r_max = max(np.sqrt(((d[s][:, None] - d[s][None]) ** 2).sum(-1)).max() for s in range(3))
    assert 5000.0 < float(far["q"].max()) * r_max < sr.X_MAX


def test_fit64_recovers_a_planted_grid_point():
    c = hr.case(hr.FIT_KEY)
    c1, c2 = metrics.default_c1(), metrics.default_c2()
    assert (c1[14], c2[35]) == (1.02, 1.5)
    exp = 3.7 * hr.combine64(c["P"][0], c["q"], c["water"], 1.02, 1.5)
    sigma = 0.01 * exp + 1e-3 * exp[0]
    fit = hr.fit64(c["P"][0], c["q"], c["water"], exp, sigma, c1, c2)
    order = np.sort(fit["chi2_grid"].reshape(-1))
    print(f"planted (1.02, 1.5): chi2 {order[0]:.3e}, the runner-up's {order[1]:.3e}, scale {float(fit['scale_grid'][14, 35])!r}")
    assert fit["index"] == 14 * 61 + 35 and order[0] < 1e-20 and order[1] > 1e-4
    assert abs(fit["scale_grid"][14, 35] - 3.7) < 1e-12 and np.array_equal(fit["I"], hr.combine64(c["P"][0], c["q"], c["water"], 1.02, 1.5))
    # against numpy's own sums: the same chi2 to rounding
    I = hr.combine64(c["P"][0], c["q"], c["water"], c1[4], c2[16])                  # 0.97, -0.4
    s = (exp * I / sigma ** 2).sum() / (I * I / sigma ** 2).sum()
    chi2 = (((s * I - exp) / sigma) ** 2).sum() / 50
    assert abs(fit["chi2_grid"][4, 16] - chi2) <= 1e-12 * chi2
    # a tie goes to the lowest flat index; a chi2 that is not finite never wins; nothing finite: -1 and a row of NaN
    tie = hr.fit64(c["P"][0], c["q"], c["water"], exp, sigma, [1.0, 1.02, 1.02], [0.5, 1.5, 1.5, 2.0])
    assert tie["index"] == 5 and tie["chi2_grid"][1, 1] == tie["chi2_grid"][2, 2]
    part = hr.fit64(c["P"][0], c["q"], c["water"], exp, sigma, [1.02], [np.nan, 2.0, 1.5])     # the NaN comes first
    assert part["index"] == 2 and np.isnan(part["chi2_grid"][0, 0]) and np.isfinite(part["chi2_grid"][0, 1:]).all()
    none = hr.fit64(np.full((6, 51), np.nan), c["q"], c["water"], exp, sigma, c1, c2)
    assert none["index"] == -1 and np.isnan(none["I"]).all()


def test_cli_allows_saxs_hydration_only_with_saxs_and_fits_only_with_a_curve():
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(saxs=51, saxs_data=None, saxs_hydration=None, experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
        base.update(kw)
        return argparse.Namespace(**base)

    assert cli.check_saxs_hydration(args()) is None and cli.check_saxs_hydration(args(saxs=0)) is None
    a = args(saxs_hydration=[1.02, 1.5])
    assert cli.check_saxs_hydration(a) == (1.02, 1.5) == a.saxs_hydration
    assert cli.check_saxs_hydration(args(saxs_hydration=[], saxs_data="curve.dat")) == ()
    assert cli.check_saxs_hydration(args(saxs_hydration=[1.0, 0.0], saxs_data="curve.dat")) == (1.0, 0.0)
    for saxs in (0, None):
        with pytest.raises(SystemExit, match="--saxs_hydration needs --saxs"):
            cli.check_saxs_hydration(args(saxs=saxs, saxs_hydration=[1.02, 1.5]))
    with pytest.raises(SystemExit, match="needs the curve of --saxs_data"):
        cli.check_saxs_hydration(args(saxs_hydration=[]))
    for bad in ([1.0], [1.0, 2.0, 3.0]):
        with pytest.raises(SystemExit, match="C1 and C2 or nothing"):
            cli.check_saxs_hydration(args(saxs_hydration=bad))
    for bad in ([0.0, 1.0], [-1.0, 1.0], [1.0, float("nan")], [float("inf"), 0.0]):
        with pytest.raises(SystemExit, match="must be positive"):
            cli.check_saxs_hydration(args(saxs_hydration=bad))
