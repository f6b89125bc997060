"""CPU checks of the ensemble observables: the float64 references of tests/observables_ref.py satisfy the conditions the
GPU tests (tests/test_observables.py) rely on, the C ABI declares and exports the two entry points and rejects bad arguments
before any HIP call, and the Python layer refuses what it cannot run.

Figures of the references (printed by every run): ref_dev 7.27e-6 A^2, 7 undecided of 4 009 630 points (1.7e-6), no
float32 / float64 flip; the contact inputs' float32 deviation 3.3e-5 .. 3.9e-5 A^2 against a margin of 1e-3."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from codlad_amd import _lib, metrics
from tests import observables_ref as obr
from tests.cli_script import load_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("codlad_sasa", "codlad_contact_counts")


def test_margins_leave_at_most_one_point_in_1e5_undecided():
    """The condition of the decision tests, over all cases together: |m64| <= 4 ref_dev for at most 1 point in 10^5, and
    the float32 restatement itself flips no decided point."""
    dev = obr.ref_dev()
    total = undecided = flips = 0
    for key in obr.sasa_keys():
        c = obr.sasa_case(*key)
        _exp, und = obr.sasa_expected(key)
        total += c["m64"].size
        undecided += int(und.sum())
        flip = (c["m64"] >= 0) != (c["m32"] >= 0)
        flips += int(flip.sum())
        assert not (flip & (np.abs(c["m64"]) > 4.0 * dev)).any(), key
    print(f"ref_dev {dev:.3e} A^2, undecided {undecided} of {total} points ({undecided / total:.2e}), float32 flips {flips}")
    # |e|^2 and R_j^2 stay below (2 * 3.2 + 1)^2 = 55 A^2 where a decision is open: five roundings of 2^-24 each
    assert 0 < dev <= 5 * 55 * 2.0 ** -24
    assert undecided <= 1e-5 * total


def test_cases_cover_the_sizes_and_both_outcomes():
    keys = obr.sasa_keys()
    assert {k[1] for k in keys if k[2] == 96} == set(obr.SIZES)
    assert {(k[1], k[2]) for k in keys} >= {(n, p) for n in obr.POINT_SIZES for p in obr.POINTS}
    assert {k[3] for k in keys} == {False, True} and {k[0] for k in keys} == {"chain", "ball"}
    for key in keys:
        c = obr.sasa_case(*key)
        exp, _und = obr.sasa_expected(key)
        n, P = key[1], key[2]
        assert c["x"].dtype == np.float32 and c["x"].shape[1:] == (n, 3) and c["m64"].shape[1:] == (n, P)
        if n == 1:
            assert (exp == P).all()
        if n >= 63 and P >= 63:
            assert (exp == 0).any() and (exp > 0).any(), key                       # buried atoms and surface atoms
        assert c["res_ptr"][0] == 0 and c["res_ptr"][-1] == n and (np.diff(c["res_ptr"]) >= 0).all()
    # the shifted case is the same structure moved and rounded again: the float64 counts move in a handful of atoms at most
    a, b = obr.sasa_expected(("ball", 600, 96, False))[0], obr.sasa_expected(("ball", 600, 96, True))[0]
    assert a.shape == b.shape and (a != b).mean() < 0.05


def test_ball_keeps_its_density_and_separation():
    rng = np.random.default_rng(3)
    p = obr.ball(600, rng)
    d2 = ((p[:, None] - p[None]) ** 2).sum(-1) + 1e9 * np.eye(600)
    assert d2.min() >= obr.MIN_SEP ** 2
    rad = np.sqrt((p ** 2).sum(1)).max()
    assert abs(600 / (4 / 3 * np.pi * rad ** 3) - obr.DENSITY) < 0.1 * obr.DENSITY


def test_sphere_points_are_unit_vectors_that_sum_to_nearly_zero():
    for n in (1, 2, 63, 64, 65, 96, 960, 1024):
        p = metrics.sphere_points(n)
        assert p.dtype == torch.float32 and tuple(p.shape) == (n, 3)
        assert np.array_equal(p.numpy(), obr.sphere_points(n))                    # the restatement, bit for bit
        norm = np.sqrt((p.numpy().astype(np.float64) ** 2).sum(1))
        assert np.abs(norm - 1.0).max() <= 2.0 ** -22
        s = p.numpy().astype(np.float64).sum(0)
        # z_k = -z_(n-1-k): the z sum is rounding only; the spiral's x, y sum stays O(1) for any n, so the mean is O(1 / n)
        assert abs(s[2]) <= n * 2.0 ** -23 and np.hypot(s[0], s[1]) <= 1.0 + 1e-6, (n, s)
    for bad in (0, 1025, -3):
        with pytest.raises(ValueError, match="n_points"):
            metrics.sphere_points(bad)


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "codlad_hip.h")).read()
    lib = _lib.lib()
    for name in ENTRY_POINTS:
        assert len(re.findall(r"\bint\s+" + name + r"\s*\(", header)) == 1, name
        assert name in _lib.exported_symbols() and hasattr(lib, name), name
        assert not name.startswith("codlad_ens_")
    assert "#define CODLAD_SASA_MAX_POINTS 1024\n" in header and _lib.SASA_MAX_POINTS == 1024
    assert "#define CODLAD_ABI_VERSION 19\n" in header and lib.codlad_abi_version() == 19
    from codlad_amd import build
    assert "observables_kernels.hip" in build.SOURCES and build.EXTRA_FLAGS["observables_kernels.hip"] == ["-ffp-contract=off"]


def test_observables_kernels_use_no_scratch():
    """The SASA kernel keeps up to 16 points per lane (48 registers) and their alive bits in registers: an array that
    went to scratch would turn every burial test into memory traffic.  The build records what hipcc made."""
    import json
    from codlad_amd import build
    build.build(force=False, verbose=False)
    if not os.path.exists(build.RESOURCES):
        build.build(force=True, verbose=False)
    with open(build.RESOURCES) as f:
        table = json.load(f)
    mine = {k: v for k, v in table.items() if v.get("source") == "observables_kernels.hip"}
    assert sum("sasa_kernel" in k for k in mine) == 5 and any("contact_kernel" in k for k in mine), sorted(mine)
    for name, r in mine.items():
        assert r["ScratchSize"] == 0, (name, r)
        if "sasa_kernelILi16" in name:
            assert r["VGPRs"] <= 128, (name, r)                                   # four waves per SIMD


def test_argument_errors_return_a_negative_code_before_any_hip_call():
    """No GPU here: a call that got as far as a launch would return a positive hipError_t (or crash)."""
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.float64)                 # any non-null host address: never dereferenced by these calls
    p = buf.ctypes.data
    res = np.array([0, 2, 4], dtype=np.int32)
    rp = res.ctypes.data
    ok = [p, 1, 4, p, p, p, 96, rp, 2, p, p, p, p, p, None]
    cases = [(6, 0), (6, 1025), (6, -1), (1, 0), (1, -2), (2, 0), (0, None), (3, None), (4, None), (5, None), (9, None),
             (10, None), (11, None), (12, None), (13, None), (7, None), (8, 0), (8, -1)]
    for k, bad in cases:
        args = list(ok)
        args[k] = bad
        assert lib.codlad_sasa(*args) < 0, (k, bad)
        assert b"codlad_sasa" in lib.codlad_last_error(), (k, bad)
    for table in ([0, 3, 2], [-1, 2, 4], [0, 2, 5], [1, 0, 4]):                   # not non-decreasing within [0, n_atoms]
        t = np.array(table, dtype=np.int32)
        args = list(ok)
        args[7] = t.ctypes.data
        assert lib.codlad_sasa(*args) < 0, table
        assert b"res_ptr" in lib.codlad_last_error()
    # residues are all or nothing
    assert lib.codlad_sasa(p, 1, 4, p, p, p, 96, None, 0, p, p, p, p, p, None) < 0
    f = C.c_float
    okc = [p, 1, 4, None, 0, f(64.0), p, None]
    for k, bad in ((0, None), (6, None), (1, 0), (2, 0), (2, -1), (4, 3), (4, -1), (3, p), (5, f(-1.0)), (5, f(float("nan")))):
        args = list(okc)
        args[k] = bad
        assert lib.codlad_contact_counts(*args) < 0, (k, bad)
        assert b"codlad_contact_counts" in lib.codlad_last_error(), (k, bad)
    assert lib.codlad_contact_counts(p, 1, 16 * 65535 + 1, None, 0, f(64.0), p, None) < 0


def test_python_layer_rejects_cpu_tensors_bad_shapes_and_unknown_elements():
    from codlad_amd.utils.cg_input import template_topology
    top = template_topology(["ALA", "GLY", "SER"])
    x = torch.zeros(2, top.n_atoms, 3)
    for call in (lambda: metrics.sasa(x, top), lambda: metrics.sasa_lists(x, [1.7] * top.n_atoms),
                 lambda: metrics.radius_of_gyration(x), lambda: metrics.contact_map(x)):
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            call()
    assert metrics.VDW_RADII == {"C": 1.70, "N": 1.55, "O": 1.52, "S": 1.80, "P": 1.80, "H": 1.20}
    assert metrics.vdw_radii(["c", "N", "O", "S", "P", "H"]).tolist() == [1.70, 1.55, 1.52, 1.80, 1.80, 1.20]
    with pytest.raises(ValueError, match="SE"):
        metrics.vdw_radii(["C", "SE"])
    for table in ([0, 3, 2], [0, 2, 9], [-1, 4], [4]):
        with pytest.raises(ValueError, match="res_ptr"):
            metrics._res_table(table, 4)
    assert metrics._res_table(None, 4) is None and metrics._res_table(top.first_atom, top.n_atoms).dtype == np.int32
    with pytest.raises(ValueError, match="radii"):
        metrics._sasa_atom_tables([1.7, -1.0], 1.4, 96, "cpu")
    radius, unit, dirs = metrics._sasa_atom_tables([1.7, 1.52], 1.4, 96, "cpu")
    assert radius.dtype == unit.dtype == dirs.dtype == torch.float32 and tuple(dirs.shape) == (96, 3)
    want = (4.0 * np.pi * radius.numpy().astype(np.float64) ** 2 / 96).astype(np.float32)
    assert np.array_equal(unit.numpy(), want)


def test_contact_inputs_keep_their_margin():
    """Every |d^2 - cut^2| exceeds 4 x the float32 restatement's deviation (CONTACT_MARGIN covers it), so the counts of the
    device must equal the float64 reference's exactly."""
    cut2 = float(np.float32(obr.CUTOFF ** 2))
    for m in obr.CONTACT_SIZES:
        c = obr.contact_case(m)
        print(f"m={m}: float32 deviation of d^2 {c['dev']:.3e} A^2, margin {obr.CONTACT_MARGIN:.0e}")
        assert 4.0 * c["dev"] <= obr.CONTACT_MARGIN
        assert not any(len(b) for b in obr.too_close_to_the_cutoff(c["x"]))
        assert np.abs(obr._d2(c["x"], np.float64) - cut2).min() > obr.CONTACT_MARGIN
        for counts in (c["counts_sel"], c["counts_all"]):
            assert counts.shape == (m, m) and (counts == counts.T).all() and not np.diag(counts).any()
        if m >= 64:
            assert 0 < c["counts_sel"].max() <= obr.CONTACT_STRUCT and (c["counts_sel"] == 0).any()


def test_cli_allows_observables_exactly_where_the_geometry_check_is_allowed():
    cli = load_cli("codlad_cli")

    def args(**kw):
        base = dict(observables=None, experiment="latent", data_process=False, synthetic=True, cg_pdb=None)
        base.update(kw)
        return argparse.Namespace(**base)

    a = args()
    assert cli.check_observables(a) == 0 and a.observables == 0
    assert cli.check_observables(args(observables=960)) == 960
    assert cli.check_observables(args(observables=96, experiment="recon")) == 96
    for bad in (0, 1025, -5):
        with pytest.raises(SystemExit, match="test points"):
            cli.check_observables(args(observables=bad))
    for exp in ("bpd", "fmloss"):
        with pytest.raises(SystemExit, match="generates none"):
            cli.check_observables(args(observables=96, experiment=exp))
    with pytest.raises(SystemExit, match="topology"):
        cli.check_observables(args(observables=96, data_process=True, synthetic=False))
    assert cli.check_observables(args(observables=96, cg_pdb=["x.pdb"], synthetic=False)) == 96
