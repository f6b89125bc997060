"""CPU checks of the reweighting feature: the C ABI of codlad_reweight_scratch_bytes, codlad_reweight_solve and
codlad_weighted_mean (declared, exported, bad arguments refused before any HIP call), what the Python layer and the CLI
refuse, and the float64 reference of tests/reweight_ref.py against the theory it restates: the stop rule re-evaluated in
np.longdouble, the weights' normalisation, the large-theta limit, the range of phi_eff, and the secant loop of the fitted
scale."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from tests import reweight_ref as rr
from tests.cli_script import load_cli, option

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTOL = 1e-9


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name, ret, n_args in (("codlad_reweight_scratch_bytes", "long long", 3), ("codlad_reweight_solve", "int", 22),
                              ("codlad_weighted_mean", "int", 7)):
        decl = re.findall(r"\b" + ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert len(decl) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name)
        assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == n_args, name
    for macro, value in (("LADDER", 16), ("SCALARS", 4), ("MAX_PROBLEMS", 4096), ("MAX_ITER", 1000)):
        assert f"#define CODLAD_REWEIGHT_{macro} {value}" in header and getattr(_lib, f"REWEIGHT_{macro}") == value
    for code, word in enumerate(("CONVERGED", "CAP", "STALLED", "FAILED", "NONE")):
        assert f"#define CODLAD_REWEIGHT_{word} {code}\n" in header
    assert _lib.REWEIGHT_STATUS == rr.STATUS == metrics.REWEIGHT_STATUS and rr.LADDER == 16
    assert "#define CODLAD_ABI_VERSION 19\n" in header and _lib.ABI_VERSION == 19
    assert "reweight_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["reweight_kernels.hip"] == ["-ffp-contract=off"]


def test_reweight_kernels_use_no_scratch():
    import json
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "reweight_kernels.hip"}
    for kernel in ("cov_kernel", "chol_kernel", "dot_kernel", "ladder_pick", "mean_kernel"):
        assert any(kernel in k for k in mine), (kernel, sorted(mine))
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced as device memory
    p = buf.ctypes.data
    one = np.ones(2, dtype=np.float64)                   # theta and scale are HOST arrays: these are read
    th = one.ctypes.data
    for bad in ((0, 4, 1), (-1, 4, 1), (4, 0, 1), (4, -2, 1), (4, 513, 1), (4, 4, 0), (4, 4, -1), (4, 4, 4097)):
        assert lib.codlad_reweight_scratch_bytes(*bad) < 0, bad
        assert b"codlad_reweight_scratch_bytes" in lib.codlad_last_error(), bad
    need = lib.codlad_reweight_scratch_bytes(4, 3, 2)
    assert need > 0 and need % 8 == 0 and lib.codlad_reweight_scratch_bytes(4, 512, 1) > 8 * 512 * 512
    assert lib.codlad_reweight_scratch_bytes(100000, 512, 8) < 2 ** 30       # the scan of the cost file stays below 1 GiB
    #     Y  y  sigma w0 N  M  theta scale P  mu0 gtol  max_iter scratch bytes mu w mean scalars n_iter status used stream
    ok = [p, p, p, p, 4, 3, th, th, 2, p, 1e-9, 50, p, need, p, p, p, p, p, p, p, None]
    cases = [(k, None) for k in (0, 1, 2, 6, 7, 12, 14, 15, 16, 17, 18, 19, 20)]
    cases += [(4, 0), (4, -1), (5, 0), (5, -1), (5, 513), (8, 0), (8, -1), (8, 4097), (11, 0), (11, -1), (11, 1001),
              (10, 0.0), (10, -1e-9), (10, float("nan")), (10, float("inf")), (13, need - 8), (13, 0)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_reweight_solve(*args) < 0, (k, bad)
        assert b"codlad_reweight_solve" in lib.codlad_last_error(), (k, bad)
    for slot in (6, 7):                                  # a theta or a scale that is not a positive finite number
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            arr = np.array([1.0, bad])
            args = list(ok)
            args[slot] = arr.ctypes.data
            assert lib.codlad_reweight_solve(*args) < 0, (slot, bad)
            assert b"codlad_reweight_solve" in lib.codlad_last_error() and b"positive finite" in lib.codlad_last_error()
    #     values w S D T out stream
    ok = [p, p, 4, 3, 2, p, None]
    for k, bad in [(0, None), (1, None), (5, None), (2, 0), (2, -1), (3, 0), (3, -1), (4, 0), (4, -1), (4, 65536)]:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_weighted_mean(*args) < 0, (k, bad)
        assert b"codlad_weighted_mean" in lib.codlad_last_error(), (k, bad)


class _FakeCuda:
    """What the refusals that precede every launch read of Y: is_cuda, device, dim and shape (nothing here reaches a launch)."""
    is_cuda, device = True, "cpu"

    def __init__(self, t):
        self.t, self.shape = t, t.shape

    def dim(self):
        return self.t.dim()


def test_python_layer_refuses_what_it_cannot_run():
    Y = torch.ones(4, 3, dtype=torch.float64)
    y, s = np.ones(3), np.ones(3)
    for call in (lambda: metrics.reweight(Y, y, s, 1.0), lambda: metrics.saxs_reweight(Y, y, y, s, 1.0),
                 lambda: metrics.weighted_mean(Y, torch.ones(4))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    F = _FakeCuda(Y)
    for bad_y, bad_s in ((np.array([1, np.nan, 1.0]), s), (np.array([1, np.inf, 1.0]), s), (y, np.array([1, 0, 1.0])),
                         (y, np.array([1, -1, 1.0])), (y, np.array([1, np.nan, 1.0])), (y, np.array([1, np.inf, 1.0]))):
        with pytest.raises(ValueError, match="finite and every sigma positive"):
            metrics.reweight(F, bad_y, bad_s, 1.0)
    with pytest.raises(ValueError, match="must have 3 values"):
        metrics.reweight(F, np.ones(4), s, 1.0)
    for bad in (0.0, -1.0, float("nan"), float("inf"), [], [1.0, 0.0]):
        with pytest.raises(ValueError, match="theta must be"):
            metrics.reweight(F, y, s, bad)
    for bad in (0.0, -2.0, float("nan"), [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError, match="scale must be"):
            metrics.reweight(F, y, s, [1.0, 2.0], scale=bad)
    for bad in (0, -1, 1001, 2.5):
        with pytest.raises(ValueError, match="max_iter"):
            metrics.reweight(F, y, s, 1.0, max_iter=bad)
    for bad in (0.0, -1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gtol"):
            metrics.reweight(F, y, s, 1.0, gtol=bad)
    with pytest.raises(ValueError, match="at most 512 observables"):
        metrics.reweight(_FakeCuda(torch.ones(2, 513, dtype=torch.float64)), np.ones(513), np.ones(513), 1.0)
    with pytest.raises(ValueError, match=r"non-empty \[N, M\]"):
        metrics.reweight(_FakeCuda(torch.ones(4, dtype=torch.float64)), y, s, 1.0)
    with pytest.raises(ValueError, match="fit must be"):
        metrics.saxs_reweight(F, y, y, s, 1.0, fit="offset")
    with pytest.raises(ValueError, match="on the Q values of q"):
        metrics.saxs_reweight(F, np.ones(4), y, s, 1.0)


def test_cases_are_the_shapes_and_thetas_the_issue_names():
    assert rr.SHAPES == ((2, 1), (3, 2), (65, 3), (257, 64), (300, 51), (100, 200), (1000, 129), (2048, 512))
    assert rr.THETAS == (1000.0, 10.0, 1.0, 0.1) and len(rr.case_keys()) == 32
    for N, M in rr.SHAPES:
        c = rr.case(N, M)
        assert c["Y"].shape == (N, M) and c["y"].shape == c["sigma"].shape == (M,) and (c["sigma"] > 0).all()
        assert (15.0 <= c["rg"]).all() and (c["rg"] <= 45.0).all()
        assert (np.abs(c["y"] - c["w_true"] @ c["Y"]) <= 6 * c["sigma"]).all()      # a reachable mean plus its noise
        for arr in c.values():
            assert not arr.flags.writeable


@pytest.mark.parametrize("N,M", rr.SHAPES, ids=lambda v: str(v))
def test_reference_meets_its_stop_rule_in_longdouble(N, M):
    """|g|_inf <= gtol * gscale re-evaluated in np.longdouble at the float64 solver's mu, status 0 within max_iter; the
    weights sum to 1; phi_eff lies in (0, 1]; the iteration counts stay within what the issue's prototype saw (24)."""
    c = rr.case(N, M)
    shown = []
    for theta in rr.THETAS:
        ref = rr.reference(N, M, theta)
        assert ref["status"] == 0 and ref["n_iter"] <= 24, (theta, ref["status"], ref["n_iter"])
        # the float64 stop rule held at rel_64 <= gtol; longdouble sees it within the difference of the two evaluations
        assert ref["rel_64"] <= GTOL and ref["rel_ld"] <= GTOL + 4 * abs(ref["rel_ld"] - ref["rel_64"]), (theta, ref["rel_ld"])
        assert abs(ref["w"].sum() - 1.0) <= 4 * N * rr.EPS and (ref["w"] >= 0).all()
        assert 0.0 < ref["phi_eff"] <= 1.0 and ref["s_rel"] >= -4 * N * rr.EPS
        if M > 1:
            assert ref["chi2"] <= ref["chi2_prior"]
        ev = rr.evaluate(c["Y"], c["y"], c["sigma"], theta, ref["mu"])
        assert float(np.abs(ev["w"] - ref["w"]).max()) <= 1e-10
        shown.append(f"theta {theta:g}: {ref['n_iter']} it, rel {ref['rel_ld']:.1e}, phi {ref['phi_eff']:.3f}")
    print(f"({N}, {M}) " + "; ".join(shown))


def test_reference_excludes_rows_and_tends_to_the_prior():
    N, M = 65, 3
    c = rr.case(N, M)
    w0 = np.random.Generator(np.random.PCG64(3)).uniform(0.5, 1.5, N)
    w0[[0, 17, 64]] = 0.0
    out = rr.solve(c["Y"], c["y"], c["sigma"], 1.0, w0=w0)
    assert out["status"] == 0 and (out["w"][[0, 17, 64]] == 0.0).all() and not out["used"][[0, 17, 64]].any()
    assert abs(out["w"].sum() - 1.0) <= 4 * N * rr.EPS
    prior = w0 / w0.sum()
    gaps = []
    for theta in (1e3, 1e6, 1e9):
        o = rr.solve(c["Y"], c["y"], c["sigma"], theta, w0=w0)
        assert o["status"] == 0
        gaps.append(float(np.abs(o["w"] - prior).max()))
    print("max |w - w0| at theta 1e3, 1e6, 1e9:", gaps)
    assert gaps[0] > gaps[1] and gaps[2] <= gaps[1] / 100 and gaps[2] <= 1e-4 * prior.max()      # |w - w0| falls as 1 / theta
    nothing = rr.solve(c["Y"], c["y"], c["sigma"], 1.0, w0=np.zeros(N))
    assert nothing["status"] == 4 and np.isnan(nothing["w"]).all() and np.isnan(nothing["mu"]).all()


SECANT_FACTOR = 0.37                                      # the calculated intensities' arbitrary unit in the secant cases


def _secant(N, M, theta):
    c = rr.case(N, M)
    Y = c["Y"] * SECANT_FACTOR

    def solve_at(scale, mu):
        out = rr.solve(Y, c["y"], c["sigma"], theta, scale=scale, mu0=mu)
        return out, out["mu"]
    c0 = rr.fit_scale(Y.mean(axis=0), c["y"], c["sigma"])
    return rr.secant(solve_at, lambda out: rr.fit_scale(out["mean"], c["y"], c["sigma"]), c0)


@pytest.mark.parametrize("N,M", [s for s in rr.SHAPES if s[1] >= 2], ids=lambda v: str(v))
def test_secant_loop_finds_the_fixed_point_of_the_scale(N, M):
    """|h| <= 1e-9 |c| within 40 rounds on every case with M >= 2, the profiles in another unit than the curve (x 0.37).
    At theta >= 1 the inner solve of the last round has converged too, within the 20 rounds of the issue's prototype.  At theta = 0.1 a
    scale a few per cent off leaves y outside what the ensemble reaches, |mu| grows and the inner solves end as stalled
    (the regime the issue keeps out of the tests): there only the issue's bound on h is asserted and the status printed."""
    shown = []
    for theta in rr.THETAS:
        c, h, rounds, converged, res = _secant(N, M, theta)
        shown.append(f"theta {theta:g}: c {c:.6f} h {h:.1e} {rounds} rounds, {rr.STATUS[res['status']]}")
        assert rounds <= 40 and abs(h) <= 1e-9 * abs(c), (theta, c, h, rounds)
        if theta >= 1.0:
            assert converged and res["status"] == 0, (theta, res["status"])
            assert rounds <= 20, (theta, c, rounds)
    print(f"({N}, {M}) " + "; ".join(shown))


def test_cli_refuses_each_misuse_of_saxs_reweight():
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(saxs=51, saxs_data="curve.dat", saxs_reweight=None)
        base.update(kw)
        return argparse.Namespace(**base)

    a = args()
    assert cli.check_saxs_reweight(a) == () and a.saxs_reweight == ()
    assert cli.check_saxs_reweight(args(saxs_reweight=[10.0, 1.0])) == (10.0, 1.0)
    assert cli.check_saxs_reweight(args(saxs_reweight=[5])) == (5.0,)
    with pytest.raises(SystemExit, match="needs --saxs:"):
        cli.check_saxs_reweight(args(saxs=0, saxs_reweight=[1.0]))
    with pytest.raises(SystemExit, match="needs --saxs_data"):
        cli.check_saxs_reweight(args(saxs_data=None, saxs_reweight=[1.0]))
    with pytest.raises(SystemExit, match="one THETA or more"):
        cli.check_saxs_reweight(args(saxs_reweight=[]))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(SystemExit, match="positive finite number"):
            cli.check_saxs_reweight(args(saxs_reweight=[1.0, bad]))
    flag = option(cli, "--saxs_reweight")
    assert flag.nargs == "*" and flag.type is float and flag.default is None
    parse = cli.build_parser().parse_args
    assert parse(["--saxs_reweight", "10", "1"]).saxs_reweight == [10.0, 1.0] and parse(["--saxs_reweight"]).saxs_reweight == []
