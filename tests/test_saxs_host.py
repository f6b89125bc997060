"""CPU checks of the SAXS feature: the constants and tables of codlad_amd.metrics.saxs, the C ABI of codlad_saxs_debye
(declared, exported, bad arguments refused before any HIP call), what the Python layer refuses, and the two references of
tests/saxs_ref.py - the restated sine against float64 sin, the float64 Debye sum against the analytic two-atom curve.

Figures (printed by every run): the restated sine stays within 2.2 * 2^-24 of sin(x) on [0, X_MAX] (the header states 5);
dev32 of the cases lies between 1.4e-8 and 9.7e-8 (0 for one atom)."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, build, metrics
from codlad_amd.utils.cg_input import template_topology
from tests import saxs_ref as sr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = {"H": 1, "C": 6, "N": 7, "O": 8, "P": 15, "S": 16}
H_TOTALS = {"GLY": 3, "ALA": 5, "SER": 5, "CYS": 5, "ASP": 4, "ASN": 6, "GLU": 6, "THR": 7, "PRO": 7, "HIS": 7, "GLN": 8,
            "VAL": 9, "MET": 9, "PHE": 9, "TYR": 9, "TRP": 10, "LEU": 11, "ILE": 11, "LYS": 13, "ARG": 13}


def test_cromer_mann_coefficients_sum_to_the_atomic_number():
    assert set(metrics.CROMER_MANN) == set(Z) == set(metrics.ATOMIC_VOLUME)
    for el, (a, b, c) in metrics.CROMER_MANN.items():
        assert len(a) == len(b) == 4 and abs(sum(a) + c - Z[el]) <= 0.01, (el, sum(a) + c)
        # f(0) in vacuo is the same sum
        assert abs(metrics.form_factors([0.0], [(el, 0)], solvent_density=0.0)[0, 0] - (sum(a) + c)) < 1e-12
    assert metrics.ATOMIC_VOLUME == {"H": 5.15, "C": 16.44, "N": 2.49, "O": 9.13, "P": 5.73, "S": 19.86}


def test_form_factors_vacuum_solvent_and_overrides():
    q = np.linspace(0.0, 0.5, 11)
    vac = metrics.form_factors(q, [("C", 0), ("C", 3), ("H", 0)], solvent_density=0.0)
    assert vac.dtype == np.float64 and vac.shape == (3, 11)
    assert np.allclose(vac[1], vac[0] + 3 * vac[2], rtol=0, atol=1e-12)
    assert (np.diff(vac, axis=1) < 0).all()                                        # falls with q
    wet = metrics.form_factors(q, [("C", 3)])
    v = 16.44 + 3 * 5.15
    assert np.allclose(vac[1] - wet[0], 0.334 * v * np.exp(-q * q * v ** (2 / 3) / (4 * np.pi)), rtol=0, atol=1e-12)
    assert wet[0, 0] < 0 < metrics.form_factors(q, [("O", 0)])[0, 0]                # a methyl is below the solvent, an O above
    double = metrics.form_factors(q, [("C", 0)], 0.0, cromer_mann={"C": ((1, 1, 1, 1), (0, 0, 0, 0), 2.0)}, volumes={"C": 1.0})
    assert np.array_equal(double, np.full((1, 11), 6.0))
    with pytest.raises(ValueError, match="SE"):
        metrics.form_factors(q, [("C", 0), ("SE", 0)])
    with pytest.raises(ValueError, match="non-negative"):
        metrics.form_factors(q, [("C", -1)])


def test_implicit_hydrogens_hold_the_residue_totals():
    for res, want in H_TOTALS.items():
        top = template_topology(["ALA", res, "ALA"])
        h = metrics.implicit_hydrogens(top)
        assert h.shape == (top.n_atoms,) and (h >= 0).all()
        lo, hi = top.first_atom[1], top.first_atom[2]
        assert int(h[lo:hi].sum()) == want, (res, int(h[lo:hi].sum()))
        assert int(h[:top.first_atom[1]].sum()) == 5 + 2                           # the chain's first residue: NH3+
        assert int(h[hi:].sum()) == 5
    h = dict(zip(template_topology(["ARG"]).atom_names[0], metrics.implicit_hydrogens(template_topology(["ARG"]))))
    assert (h["N"], h["NE"], h["NH1"], h["NH2"], h["CZ"]) == (3, 1, 2, 2, 0)
    top = template_topology(["PRO", "LYS", "HIS", "SEP", "TPO", "GLY"], chain_ids=[0, 0, 0, 1, 1, 1])
    h = metrics.implicit_hydrogens(top)
    at = lambda r, name: int(h[top.atom(r, name)])                                 # noqa: E731
    assert at(0, "N") == 2 and at(1, "NZ") == 3 and (at(2, "ND1"), at(2, "NE2")) == (0, 1)
    assert at(3, "N") == 3 and at(4, "N") == 1 and at(5, "CA") == 2
    assert [at(3, n) for n in ("OG", "P", "OE1", "OE2", "OE3")] == [0] * 5 and at(4, "OG1") == 0 and at(4, "CG2") == 3
    from codlad_amd.utils.dataset_builder import Topology
    with pytest.raises(ValueError, match="XD9"):
        metrics.implicit_hydrogens(Topology(["ALA"], [["N", "CA", "C", "O", "XD9"]]))
    with pytest.raises(ValueError, match="MSE"):
        metrics.implicit_hydrogens(Topology(["MSE"], [["N", "CA", "C", "O"]]))
    groups, types = metrics.saxs_groups(top)
    assert len(groups) <= _lib.SAXS_MAX_TYPES and types.shape == (top.n_atoms,)
    assert all(groups[t] == (e, k) for t, e, k in zip(types, top.element, h))


def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    name = "codlad_saxs_debye"
    decl = re.findall(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert len(decl) == 1 and not name.startswith("codlad_ens_")
    assert name in _lib.exported_symbols() and hasattr(lib, name)
    assert len(_lib._SIGS[name][1]) == decl[0].count(",") + 1 == 13
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19
    assert (sr.MAX_Q, sr.MAX_TYPES, sr.CHUNK) == (_lib.SAXS_MAX_Q, _lib.SAXS_MAX_TYPES, _lib.SAXS_Q_CHUNK) == (512, 32, 16)
    assert (sr.X_MAX, sr.X_SMALL, sr.SIN_ULPS) == (_lib.SAXS_X_MAX, _lib.SAXS_X_SMALL, _lib.SAXS_SIN_ULPS)
    for c in ("INV_PI", "P1", "P2", "P3", "S3", "S5", "S7", "S9", "S11", "C6", "C20", "X_MAX", "X_SMALL"):
        assert re.search(r"#define CODLAD_SAXS_" + c + r" -?0x1(\.[0-9a-f]+)?p[+-]\d+f", header), c    # hex floats
    assert "saxs_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["saxs_kernels.hip"] == ["-ffp-contract=off"]


def test_reduction_constants_make_the_leading_products_exact():
    k = sr.K
    p1, p2, p3 = (float(k[c]) for c in ("P1", "P2", "P3"))
    assert abs(p1 + p2 + p3 - np.pi) < 2.0 ** -46
    k_max = int(np.rint(sr.X_MAX / np.pi))
    for p, bits in ((p1, 8), (p2, 11)):
        m = p / 2.0 ** np.floor(np.log2(p))
        assert m * 2 ** (bits - 1) == int(m * 2 ** (bits - 1))                     # `bits` significant bits
        assert k_max < 2 ** (24 - bits)
    ks = np.arange(k_max + 1, dtype=np.float32)
    for c in ("P1", "P2"):
        assert np.array_equal((ks * k[c]).astype(np.float64), ks.astype(np.float64) * float(k[c]))
    assert float(k["C6"]) == float(np.float32(1 / 6)) and float(k["C20"]) == float(np.float32(0.05))
    assert float(k["INV_PI"]) == float(np.float32(1 / np.pi))


def test_saxs_kernels_use_no_scratch():
    import json
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "saxs_kernels.hip"}
    assert any("saxs_pair_kernel" in k for k in mine) and any("saxs_sum_kernel" in k for k in mine), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0, (name, r)
        if "saxs_pair_kernel" in name:
            assert r["VGPRs"] <= 168, (name, r)                                    # three waves per SIMD


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced by these calls
    p = buf.ctypes.data
    ok = [p, 1, 4, p, 2, p, p, 8, p, p, p, p, None]
    cases = [(0, None), (3, None), (5, None), (6, None), (8, None), (9, None), (11, None), (1, 0), (1, -1), (2, 0), (2, -3),
             (4, 0), (4, -1), (4, 33), (7, 0), (7, -1), (7, 513), (1, 2 ** 31 - 1), (2, 2 ** 30)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        if (k, bad) == (1, 2 ** 31 - 1):
            args[2] = 129                                # two workgroups a structure: the grid passes 2^31
        assert lib.codlad_saxs_debye(*args) < 0, (k, bad)
        assert b"codlad_saxs_debye" in lib.codlad_last_error(), (k, bad)


def test_python_layer_refuses_what_it_cannot_run():
    top = template_topology(["ALA", "GLY", "SER"])
    x = torch.zeros(2, top.n_atoms, 3)
    q = np.linspace(0.01, 0.5, 8)
    for call in (lambda: metrics.saxs_profile(x, top), lambda: metrics.saxs_profile_lists(x, [0] * top.n_atoms, np.ones((1, 8)), q),
                 lambda: metrics.saxs_fit(torch.ones(8), q, np.ones(8), np.ones(8))):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    assert "_saxs_tables" not in top.__dict__                                       # refused before any table was built
    tables = lambda t, f, qq: metrics._saxs_tables(t, f, qq, "cpu")                # noqa: E731
    typ, ff, qd = tables([0, 1, 1], np.ones((2, 8)), q)
    assert (typ.dtype, ff.dtype, qd.dtype) == (torch.int32, torch.float32, torch.float32) and tuple(ff.shape) == (2, 8)
    for bad_types in ([0, 2], [-1, 0], []):
        with pytest.raises(ValueError, match="atom type"):
            tables(bad_types, np.ones((2, 8)), q)
    limit = metrics.SAXS_Q_LIMIT
    assert limit == sr.X_MAX / metrics.SAXS_MAX_EXTENT
    for bad_q in (np.nan, np.inf, -0.1, limit * 1.001):
        qq = q.copy()
        qq[3] = bad_q
        with pytest.raises(ValueError, match="every q"):
            tables([0, 1], np.ones((2, 8)), qq)
    tables([0, 1], np.ones((2, 8)), np.linspace(0, limit, 8))
    for bad_entry in (np.nan, np.inf, 1e39):
        f = np.ones((2, 8))
        f[1, 5] = bad_entry
        with pytest.raises(ValueError, match="table entry"):
            tables([0, 1], f, q)
    with pytest.raises(ValueError, match="at most"):
        tables([0], np.ones((1, 513)), np.linspace(0.0, 0.5, 513))
    with pytest.raises(ValueError, match="at most"):
        tables([0], np.ones((33, 8)), q)
    with pytest.raises(ValueError, match=r"\[T, Q\]"):
        tables([0], np.ones((2, 7)), q)
    assert metrics.default_q().shape == (51,) and metrics.default_q()[0] == 0.0 and metrics.default_q()[-1] == 0.5


def test_restated_sine_stays_within_the_stated_ulps_of_float64_sin():
    """|sin32(x) - sin(x)| <= CODLAD_SAXS_SIN_ULPS * 2^-24 for the float32 x of a dense sweep of [0, X_MAX], of every float
    within 8 of a multiple of pi / 2, and of every float within 4096 of X_SMALL, where the two branches of sinc meet."""
    def err(x):
        return np.abs(sr.sin32(x).astype(np.float64) - np.sin(x.astype(np.float64))) / 2.0 ** -24

    rng = np.random.default_rng(0)
    sweep = np.concatenate([rng.uniform(0, sr.X_MAX, 2_000_000), np.linspace(0, sr.X_MAX, 1_000_001),
                            rng.uniform(0, 8.0, 500_000)]).astype(np.float32)
    base = (np.arange(0, int(sr.X_MAX / (np.pi / 2)) + 1) * (np.pi / 2)).astype(np.float32).view(np.uint32).astype(np.int64)
    near = np.concatenate([(base + d) for d in range(-8, 9)])
    near = near[near >= 0].astype(np.uint32).view(np.float32)
    near = near[near <= sr.X_MAX]
    worst = max(err(sweep).max(), err(near).max())
    print(f"restated sine: max |error| {worst:.3f} * 2^-24 over {sweep.size + near.size} arguments up to {sr.X_MAX}")
    assert worst <= sr.SIN_ULPS
    assert (sr.sin32(np.float32([0.0])) == 0).all()
    # the seam of sinc: both branches within 2^-22 relative of float64 sinc on every float around X_SMALL
    xs = (np.float32(sr.X_SMALL).view(np.uint32).astype(np.int64) + np.arange(-4096, 4097)).astype(np.uint32).view(np.float32)
    r = np.float32(3.7)
    q = xs / r
    x = q * r
    got = sr.sinc32(x, np.float32(1) / r, np.float32(1) / q).astype(np.float64)
    want = np.sin(x.astype(np.float64)) / x.astype(np.float64)
    assert (x < np.float32(sr.X_SMALL)).any() and (x >= np.float32(sr.X_SMALL)).any()
    assert np.abs(got / want - 1).max() <= 2.0 ** -22
    # r = 0 and q = 0 take the series and give exactly 1
    with np.errstate(divide="ignore"):
        assert sr.sinc32(np.float32([0.0, 0.0]), np.float32([np.inf, 0.25]), np.float32([2.0, np.inf])).tolist() == [1.0, 1.0]


def test_float64_reference_equals_the_analytic_two_atom_curve_and_the_forward_value():
    q = np.linspace(0.0, 0.5, 8).astype(np.float32)
    ff = np.array([[6.0] * 8, [-1.5] * 8], dtype=np.float32) * np.exp(-q.astype(np.float64) ** 2).astype(np.float32)[None]
    x = np.array([[[1.0, 2.0, 3.0], [1.0, 5.0, 3.0]]], dtype=np.float32)            # 3 A apart
    I, A = sr.debye64(x, [0, 1], ff, q)
    want = sr.two_atoms(ff[0].astype(np.float64), ff[1].astype(np.float64), 3.0, q)
    assert np.abs(I[0] - want).max() <= 4 * 2.0 ** -53 * A.max()
    assert (A >= np.abs(I)).all()
    for key in sr.case_keys():
        c = sr.case(key)
        f = c["ff"].astype(np.float64)[c["types"]]
        if key[4] == "q0":                                                           # I(0) = (sum f)^2
            assert np.abs(c["I"][:, 0] - f[:, 0].sum() ** 2).max() <= len(f) ** 2 * 2.0 ** -52 * c["A"][:, 0].max()
        assert np.isfinite(c["I"]).all() and np.isfinite(c["I32"]).all() and (c["A"] > 0).all()
        assert c["dev32"] <= 2.0 ** -20, key                                         # the restatement is a float32 Debye sum
        if key[0] > 1:
            d = c["x"].astype(np.float64)
            r_max = max(np.sqrt(((d[s][:, None] - d[s][None]) ** 2).sum(-1)).max() for s in range(d.shape[0]))
            assert float(c["q"].max()) * r_max < sr.X_MAX
            if key[4] == "far":
                assert float(c["q"].max()) * r_max > 5000.0
        for arr in c.values():
            if isinstance(arr, np.ndarray):
                assert not arr.flags.writeable
    print("dev32: " + ", ".join(f"{sr.case_id(k)} {sr.case(k)['dev32']:.2e}" for k in sr.case_keys()))


def test_cases_cover_the_sizes_the_issue_names():
    keys = sr.case_keys()
    assert {k[0] for k in keys} == set(sr.SIZES) == {1, 2, 63, 64, 65, 129, 300}
    assert {k[1] for k in keys} == set(sr.Q_SIZES) == {1, sr.CHUNK, sr.CHUNK + 1, 51}
    assert {k[2] for k in keys} == set(sr.T_SIZES) == {1, 5, sr.MAX_TYPES}
    assert {k[3] for k in keys} == set(sr.SHIFTS) == {0.0, 500.0}
    assert {k[4] for k in keys} == {"plain", "coincident", "q0", "far"}
    c = sr.case(next(k for k in keys if k[4] == "coincident"))
    assert (c["x"][:, 40] == c["x"][:, 7]).all() and (c["x"][1, 64] == c["x"][1, 0]).all()
    assert sr.case(next(k for k in keys if k[4] == "q0"))["q"][0] == 0.0


def test_cli_allows_saxs_exactly_where_observables_are_allowed(tmp_path):
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(saxs=None, saxs_data=None, experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
        base.update(kw)
        return argparse.Namespace(**base)

    a = args()
    assert cli.check_saxs(a) == 0 and a.saxs == 0
    assert cli.check_saxs(args(saxs=51)) == 51 and cli.check_saxs(args(saxs=16, experiment="recon")) == 16
    for bad in (0, 513, -5):
        with pytest.raises(SystemExit, match="q values"):
            cli.check_saxs(args(saxs=bad))
    for exp in ("bpd", "fmloss"):
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_saxs(args(saxs=51, experiment=exp))
    with pytest.raises(SystemExit, match="topology"):
        cli.check_saxs(args(saxs=51, data_process=True, synthetic=False))
    assert cli.check_saxs(args(saxs=51, cg_pdb=["x.pdb"], synthetic=False)) == 51
    with pytest.raises(SystemExit, match="--saxs_data needs --saxs"):
        cli.check_saxs(args(saxs_data="curve.dat"))
    path = tmp_path / "curve.dat"
    path.write_text("# q I sigma\n0.01 100.0 1.0\n0.02 90.5 0.9  # a comment\n\n0.03 80 0.8\n")
    q, I, sig = cli.read_saxs_data(str(path))
    assert q.tolist() == [0.01, 0.02, 0.03] and I.tolist() == [100.0, 90.5, 80.0] and sig.tolist() == [1.0, 0.9, 0.8]
    path.write_text("0.01 100.0\n")
    with pytest.raises(SystemExit, match="three columns"):
        cli.read_saxs_data(str(path))
